"""The three discriminators the LSGAN objective trains (basic + sigmoid, pixel + sigmoid, multi) in fp32
mode, on fan-in weights at 32^2 and 64^2, batch 2:

  * outputs and least-squares losses (labels False / True) against the reference's own fp64 values
    (tests/golden/golden_v5.npz, gen_golden_v5.py): 1e-5 relative;
  * weight, bias and input gradients of the label-True loss against a torch-fp64 restatement of the
    network written here (DSGAN/models/networks.py:533-699 in functional form): per-tensor relative
    error <= max(1e-5, 8 x the error of the same restatement run in torch fp32) -- the 8x is the
    project's conditioning margin; torch's CPU fp32 is <= 5.1e-6 off at these shapes;
  * the conv biases ahead of an InstanceNorm have analytic gradient 0 and are held to
    |delta| <= 2e-6 * ||g_weight|| of their layer, as tests/test_dbatch_gpu.py holds them (the CPU
    fp32 value is 5e-8).
"""
import json
import os
from collections import OrderedDict

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from oracle.recipe import make_params, synth_pair

pytestmark = pytest.mark.gpu

G5 = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "golden_v5.npz"))
IN_BIAS = {"basic": ["model.%d.bias" % i for i in (2, 5, 8)], "pixel": ["net.2.bias"],
           "multi": ["layer%d.%d.bias" % (s, i) for s in range(3) for i in (2, 5, 8)]}


def _rel(a, b):
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    return ((a - b).norm() / max(b.norm().item(), 1e-30)).item()


def _params(kind):
    spec = [(str(k), tuple(json.loads(str(s)))) for k, s in zip(G5["D5_%s_keys" % kind], G5["D5_%s_shapes" % kind])]
    return make_params(spec, "fanin", 5000)


def _patch(x, p, prefix, pad):
    """One PatchGAN Sequential (conv indices 0, 2, 5, 8, 11) + sigmoid, in torch ops."""
    h = F.leaky_relu(F.conv2d(x, p[prefix + "0.weight"], p[prefix + "0.bias"], stride=2, padding=pad), 0.2)
    for i, s in ((2, 2), (5, 2), (8, 1)):
        h = F.conv2d(h, p[prefix + "%d.weight" % i], p[prefix + "%d.bias" % i], stride=s, padding=pad)
        h = F.leaky_relu(F.instance_norm(h, eps=1e-5), 0.2)
    return torch.sigmoid(F.conv2d(h, p[prefix + "11.weight"], p[prefix + "11.bias"], stride=1, padding=pad))


def _restated(kind, x, p):
    """The discriminator's outputs (one per scale) as the reference computes them."""
    if kind == "basic":
        return [_patch(x, p, "model.", 1)]
    if kind == "pixel":
        h = F.leaky_relu(F.conv2d(x, p["net.0.weight"], p["net.0.bias"]), 0.2)
        h = F.leaky_relu(F.instance_norm(F.conv2d(h, p["net.2.weight"], p["net.2.bias"]), eps=1e-5), 0.2)
        return [torch.sigmoid(F.conv2d(h, p["net.5.weight"], p["net.5.bias"]))]
    outs = []
    for i in range(3):
        outs.append(_patch(x, p, "layer%d." % (2 - i), 2))
        if i < 2:
            x = F.avg_pool2d(x, 3, 2, 1, count_include_pad=False)
    return outs


def _restated_grads(kind, x, params, dtype):
    p = OrderedDict((k, v.detach().clone().to(dtype).requires_grad_()) for k, v in params.items())
    x = x.detach().clone().to(dtype).requires_grad_()
    loss = 0
    for o in _restated(kind, x, p):
        loss = loss + torch.mean((o - 1.0) ** 2)
    loss.backward()
    g = OrderedDict((k, v.grad.double()) for k, v in p.items())
    g["input"] = x.grad.double()
    return g


@pytest.fixture(scope="module")
def refs():
    """The torch restatement's gradients (fp64, and fp32 for its own error), computed once per case."""
    cache = {}

    def get(kind, size):
        if (kind, size) not in cache:
            A, B = synth_pair(2, size, seed=int(G5["N5_input_seed"]))
            x = torch.cat((A, B), 1)
            pr = _params(kind)
            cache[(kind, size)] = (x, pr, _restated_grads(kind, x, pr, torch.float64),
                                   _restated_grads(kind, x, pr, torch.float32))
        return cache[(kind, size)]
    return get


@pytest.mark.parametrize("size", [32, 64])
@pytest.mark.parametrize("kind", ["basic", "pixel", "multi"])
def test_discriminator_outputs_losses_and_grads(kind, size, refs):
    import dsgan_hip
    from dsgan_hip import functional as HF
    from models.networks import define_D, GANLoss, GANLoss_multi
    dsgan_hip.require_gpu()
    HF.set_precision("fp32")
    x, pr, g64, g32 = refs(kind, size)
    net = define_D(6, int(G5["N5_ndf"]), kind, 3, "instance", True, "normal", [0])
    with torch.no_grad():
        sd = net.state_dict()
        assert list(sd.keys()) == list(pr.keys())
        for k, v in sd.items():
            v.copy_(pr[k])
    crit = GANLoss_multi(use_lsgan=True) if kind == "multi" else GANLoss(use_lsgan=True).cuda()
    xd = x.detach().clone().cuda().requires_grad_(True)
    assert xd.is_leaf
    y = net(xd)
    outs = [s[-1] for s in y] if kind == "multi" else [y]
    if kind == "multi":
        assert isinstance(y, list) and all(isinstance(s, list) and len(s) == 1 for s in y) and len(y) == 3
    pre = "N5_%s_%d_f64_" % (kind, size)
    msg = []
    for i, o in enumerate(outs):
        want = torch.from_numpy(G5[pre + "out%d" % i])
        assert tuple(o.shape) == tuple(want.shape), (i, o.shape, want.shape)
        e = _rel(o, want)
        msg.append("out%d %.1e" % (i, e))
        assert e <= 1e-5, (kind, size, i, e)
    l_false, l_true = crit(y, False), crit(y, True)
    for got, want in zip((l_false.item(), l_true.item()), G5[pre + "loss"]):
        msg.append("loss %.1e" % (abs(got - want) / abs(want)))
        assert abs(got - want) <= 1e-5 * abs(want), (kind, size, got, want)
    l_true.backward()
    torch.cuda.synchronize()
    got = OrderedDict((k, p.grad) for k, p in net.named_parameters())
    got["input"] = xd.grad
    for k, g in got.items():
        assert torch.isfinite(g).all(), k
        if k in IN_BIAS[kind]:
            gw = g64[k.replace("bias", "weight")].norm().item()
            d = (g.double().cpu() - g64[k]).norm().item()
            msg.append("%s |d| %.1e (%.1e |gw|)" % (k, d, d / gw))
            assert d <= 2e-6 * gw, (kind, size, k, d, gw)
            continue
        own = _rel(g32[k], g64[k])
        e = _rel(g, g64[k])
        msg.append("%s %.1e (torch fp32 %.1e)" % (k, e, own))
        assert e <= max(1e-5, 8 * own), (kind, size, k, e, own)
    print("\n[%s %d^2] %s" % (kind, size, ", ".join(msg)))
