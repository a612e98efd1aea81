"""The BatchNorm2d PatchGAN (``--norm batch``: ``basic`` with 3 layers and ``n_layers`` with 2, with and
without the trailing sigmoid) in fp32 mode and training mode, on the recipe of tests/bn_fixture.py
at 32^2 and 64^2, batch 2:

  * the state_dict keys equal the reference's (tests/golden/golden_v6.npz, gen_golden_v6.py);
  * outputs and both loss values (labels False / True; BCE-with-logits without the sigmoid, least
    squares with it) against the reference's own fp64 values: 1e-5 relative;
  * every BatchNorm's running buffers after that one forward against the reference's: 1e-5, and
    every counter == 1;
  * every parameter gradient and the input gradient of the label-True loss against a torch-fp64
    restatement of the network (tests/bn_fixture.py torch_patchgan_bn): per-tensor relative error
    <= max(1e-5, 8 x the error of the same restatement run in torch fp32) -- the 8x is the project's
    conditioning margin; torch's CPU fp32 is <= 1.5e-6 off on every tensor at these shapes.
"""
import os
import sys
from collections import OrderedDict

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from bn_fixture import d_spec_bn, d_params_bn, bn_indices, torch_patchgan_bn_grads  # noqa: E402
from oracle.recipe import synth_pair  # noqa: E402

pytestmark = pytest.mark.gpu

G6 = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "golden_v6.npz"))
NETS = {"basic": 3, "n_layers": 2}


def _rel(a, b):
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    return ((a - b).norm() / max(b.norm().item(), 1e-30)).item()


@pytest.fixture(scope="module")
def refs():
    """The torch restatement's gradients (fp64, and fp32 for its own error), computed once per case."""
    cache = {}

    def get(kind, sig, size):
        if (kind, sig, size) not in cache:
            A, B = synth_pair(2, size, seed=int(G6["N6_input_seed"]))
            x = torch.cat((A, B), 1)
            pr = d_params_bn(d_spec_bn(6, int(G6["N6_ndf"]), NETS[kind]))
            cache[(kind, sig, size)] = (x, pr, torch_patchgan_bn_grads(x, pr, torch.float64, bool(sig))[1],
                                        torch_patchgan_bn_grads(x, pr, torch.float32, bool(sig))[1])
        return cache[(kind, sig, size)]
    return get


@pytest.mark.parametrize("size", [32, 64])
@pytest.mark.parametrize("sig", [0, 1])
@pytest.mark.parametrize("kind", ["basic", "n_layers"])
def test_discriminator_outputs_losses_buffers_and_grads(kind, sig, size, refs):
    import dsgan_hip
    from dsgan_hip import functional as HF
    from models.networks import define_D, GANLoss
    dsgan_hip.require_gpu()
    HF.set_precision("fp32")
    x, pr, g64, g32 = refs(kind, sig, size)
    net = define_D(6, int(G6["N6_ndf"]), kind, NETS[kind], "batch", bool(sig), "normal", [0])
    assert net.training
    with torch.no_grad():
        sd = net.state_dict()
        assert list(sd.keys()) == list(G6["D6_%s_%d_keys" % (kind, sig)]) == list(pr.keys())
        for k, v in sd.items():
            v.copy_(pr[k])
    crit = GANLoss(use_lsgan=bool(sig)).cuda()
    xd = x.detach().clone().cuda().requires_grad_(True)
    y = net(xd)
    pre = "N6_%s_%d_%d_f64_" % (kind, sig, size)
    want = torch.from_numpy(G6[pre + "out"])
    assert tuple(y.shape) == tuple(want.shape)
    msg = ["out %.1e" % _rel(y, want)]
    assert _rel(y, want) <= 1e-5, (kind, sig, size, _rel(y, want))
    l_false, l_true = crit(y, False), crit(y, True)
    for got, w in zip((l_false.item(), l_true.item()), G6[pre + "loss"]):
        msg.append("loss %.1e" % (abs(got - w) / abs(w)))
        assert abs(got - w) <= 1e-5 * abs(w), (kind, sig, size, got, w)
    idx = bn_indices(d_spec_bn(6, int(G6["N6_ndf"]), NETS[kind]))
    rm = torch.cat([net.model[i].running_mean for i in idx])
    rv = torch.cat([net.model[i].running_var for i in idx])
    e_rm, e_rv = _rel(rm, torch.from_numpy(G6[pre + "rm"])), _rel(rv, torch.from_numpy(G6[pre + "rv"]))
    msg.append("running_mean %.1e running_var %.1e" % (e_rm, e_rv))
    assert e_rm <= 1e-5 and e_rv <= 1e-5
    assert [int(net.model[i].num_batches_tracked) for i in idx] == [1] * len(idx)
    l_true.backward()
    torch.cuda.synchronize()
    got = OrderedDict((k, p.grad) for k, p in net.named_parameters())
    got["input"] = xd.grad
    assert list(got) == list(g64)
    for k, g in got.items():
        assert torch.isfinite(g).all(), k
        own, e = _rel(g32[k], g64[k]), _rel(g, g64[k])
        msg.append("%s %.1e (torch fp32 %.1e)" % (k, e, own))
        assert e <= max(1e-5, 8 * own), (kind, sig, size, k, e, own)
    print("\n[batch-norm %s sigmoid %d %d^2] %s" % (kind, sig, size, ", ".join(msg)))
