"""The U-Net generator on HIP kernels against the reference (tests/golden/golden_v7.npz) and the fp64
restatement of tests/unet_fixture.py, batch 2, training mode, both norms:

  UnetGenerator(3, 3, 5, 8) at 32^2, (3, 3, 6, 8) at 64^2 (the smallest net with a dropout block) and
  (3, 3, 5, 32) at 32^2 (its outer levels take the MFMA families in the 16-bit modes).

fp32 mode: the output against the reference's fp64 output at 1e-5 relative; the BatchNorm running
buffers after the forward at 1e-5 and every counter == 1; every parameter gradient (the PReLU slopes
included) and the input gradient against the fp64 fixture at max(1e-5, 8 x the fixture's own fp32
error) -- the bars of tests/test_batchnorm_nets_gpu.py.  A conv bias directly in front of an
InstanceNorm has a mathematically zero gradient (what is computed is rounding noise): those tensors are
compared by absolute error against the norm of the same layer's weight gradient.  With dropout on, the
fixture is fed HF.dropout_mask for the counter the forward used, and the bars are the same.
One size below the smallest, torch raises (InstanceNorm: one spatial element; BatchNorm: the 4x4 kernel
on a 3x3 padded input) and so does the port, with the same error type.
16-bit modes: the nets run and are finite; the 6-deep ngf-32 net's output error at 64^2 against its own
fp32-mode output is at most 4x the same figure of MixConvNeXtML at 64^2, batch 2 (the factor the
BatchNorm PatchGAN used against the instance D); both figures are printed.  Measured on an MI355X:
bf16 6.5e-3 (instance) / 5.9e-3 (batch) against 4.2e-3; fp16 8.0e-4 / 6.8e-4 against 1.9e-3.
"""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from unet_fixture import (unet_spec, unet_params, unet_levels, torch_unet_grads, loss_probe,  # noqa: E402
                          conv_bias_before_instnorm, out_view)
from oracle import dsgan_cpu as O  # noqa: E402
from oracle.recipe import make_params, synth_pair  # noqa: E402

pytestmark = pytest.mark.gpu

DEV = "cuda"
G7 = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "golden_v7.npz"))
NETS = [(5, 8, 32), (6, 8, 64), (5, 32, 32)]


@pytest.fixture(scope="module", autouse=True)
def _lib():
    import dsgan_hip
    dsgan_hip.require_gpu()
    dsgan_hip.set_precision("fp32")
    yield
    dsgan_hip.set_precision("fp32")


def rel(a, b):
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    return ((a - b).norm() / max(b.norm().item(), 1e-30)).item()


def _net(norm, nd, ngf, drop=False):
    from models.networks import get_norm_layer
    from models.unet import UnetGenerator
    spec = unet_spec(3, 3, nd, ngf, norm, drop)
    params = unet_params(spec)
    net = UnetGenerator(3, 3, nd, ngf, norm_layer=get_norm_layer(norm), use_dropout=drop).to(DEV).train()
    sd = net.state_dict()
    assert [(k, tuple(v.shape)) for k, v in sd.items()] == spec
    with torch.no_grad():
        for k, v in sd.items():
            v.copy_(params[k])
    return net, params


_FIX = {}


def _fixture(norm, nd, ngf, size, seed, masks_key, masks):
    """fp64 and fp32 runs of the restatement, computed once per case."""
    key = (norm, nd, ngf, size, seed, masks_key)
    if key not in _FIX:
        params = unet_params(unet_spec(3, 3, nd, ngf, norm, masks is not None))
        A, _ = synth_pair(2, size, seed=seed)
        lv = unet_levels(3, 3, nd, ngf, masks is not None)
        _FIX[key] = (torch_unet_grads(A, params, lv, norm, torch.float64, masks),
                     torch_unet_grads(A, params, lv, norm, torch.float32, masks))
    return _FIX[key]


@pytest.mark.parametrize("nd,ngf,size,drop", [n + (False,) for n in NETS] + [(6, 8, 64, True)])
@pytest.mark.parametrize("norm", ["instance", "batch"])
def test_unet_fp32_against_reference_and_fixture(norm, nd, ngf, size, drop):
    from dsgan_hip import functional as HF
    pre = "N7_%s_%d_%d_%d_" % (norm, nd, ngf, size)
    seed = int(G7[pre + "input_seed"])
    net, params = _net(norm, nd, ngf, drop)
    masks = None
    if drop:
        (blk,) = net.dropout_blocks()
        blk.drop_seed = int(G7["N7_drop_seed"])
        assert blk.drop_stream == 0 and int(blk.drop_counter) == 0
        masks = [HF.dropout_mask((2, ngf * 8, size >> 4, size >> 4), blk.drop_seed, 0, 0).cpu()]
    A, _ = synth_pair(2, size, seed=seed)
    x = A.to(DEV).requires_grad_()
    out = net(x)
    (out * loss_probe(out.shape).float().to(DEV)).sum().div(out.numel()).backward()
    torch.cuda.synchronize()
    if drop:
        assert int(blk.drop_counter) == 1
    key = pre + ("f64_dout" if drop else "f64_out")
    e_out = rel(out_view(out), torch.from_numpy(G7[key]))
    e_norm = abs(float(out.detach().double().norm()) - float(G7[key + "_norm"])) / float(G7[key + "_norm"])
    report = ["out %.2e (norm %.2e)" % (e_out, e_norm)]
    assert e_out <= 1e-5 and e_norm <= 1e-5
    (o64, g64, b64), (o32, g32, _) = _fixture(norm, nd, ngf, size, seed, drop, masks)
    assert rel(out_view(o64), torch.from_numpy(G7[key])) <= 1e-12
    if norm == "batch":
        sd = net.state_dict()
        for k, v in b64.items():
            if k.endswith("num_batches_tracked"):
                assert int(sd[k]) == 1 == int(v)
            else:
                assert rel(sd[k], v) <= 1e-5, k
        if not drop:
            rm = torch.cat([v.flatten() for k, v in sd.items() if k.endswith("running_mean")])
            rv = torch.cat([v.flatten() for k, v in sd.items() if k.endswith("running_var")])
            assert rel(rm, torch.from_numpy(G7[pre + "f64_rm"])) <= 1e-5
            assert rel(rv, torch.from_numpy(G7[pre + "f64_rv"])) <= 1e-5
    zero_bias = set(conv_bias_before_instnorm(unet_spec(3, 3, nd, ngf, norm, drop), norm))
    got = dict(net.named_parameters())
    worst = 0.0
    for k, gr in g64.items():
        mine = x.grad if k == "input" else got[k].grad
        if k in zero_bias:
            wn = float(g64[k[:-len("bias")] + "weight"].norm())
            e, bar = float((mine.double().cpu() - gr).norm()) / wn, max(1e-5, 8 * float((g32[k] - gr).norm()) / wn)
        else:
            e, bar = rel(mine, gr), max(1e-5, 8 * rel(g32[k], gr))
        worst = max(worst, e / bar)
        assert e <= bar, (k, e, bar)
    report.append("worst gradient error / bar %.2f over %d tensors" % (worst, len(g64)))
    print("\n[unet %s %d-deep ngf %d %d^2%s fp32] " % (norm, nd, ngf, size, " dropout" if drop else "") + "; ".join(report))


@pytest.mark.parametrize("norm,err", [("instance", ValueError), ("batch", RuntimeError)])
def test_sizes_where_torch_raises(norm, err):
    net, _ = _net(norm, 5, 8)
    A, _ = synth_pair(2, 16, seed=43)
    with pytest.raises(err):
        net(A.to(DEV))


@pytest.mark.parametrize("prec", ["bf16", "fp16"])
def test_16bit_modes_finite_and_output_error(prec):
    from dsgan_hip import functional as HF
    from models.networks import define_G
    for norm in ("instance", "batch"):
        for nd, ngf, size in NETS:
            net, _ = _net(norm, nd, ngf, nd > 5)
            A, _ = synth_pair(2, size, seed=43)
            x = A.to(DEV).requires_grad_()
            with HF.precision(prec):
                out = net(x)
                out.sum().backward()
            torch.cuda.synchronize()
            assert torch.isfinite(out).all() and torch.isfinite(x.grad).all()
            assert all(torch.isfinite(p.grad).all() for p in net.parameters())
    A, _ = synth_pair(2, 64, seed=51)
    x = A.to(DEV)
    errs = {}
    for norm in ("instance", "batch"):
        net, _ = _net(norm, 6, 32)
        outs = {}
        for p in ("fp32", prec):
            with torch.no_grad(), HF.precision(p):
                outs[p] = net(x).clone()   # (training mode: normalised by the batch, whatever the buffers hold)
        errs[norm] = rel(outs[prec], outs["fp32"])
    torch.manual_seed(20)
    g = define_G(3, 3, 64, "MixConvNeXtML", "instance", False, "normal", [0])
    gp = make_params(O.g_param_spec(), "fanin", 1000)
    with torch.no_grad():
        for k, v in g.state_dict().items():
            v.copy_(gp[k])
        outs = {}
        for p in ("fp32", prec):
            with HF.precision(p):
                outs[p] = g(x).clone()
    base = rel(outs[prec], outs["fp32"])
    print("\n[%s] output vs fp32 mode at 64^2, batch 2: unet (6-deep, ngf 32) instance %.3e, batch %.3e; MixConvNeXtML %.3e"
          % (prec, errs["instance"], errs["batch"], base))
    assert errs["instance"] <= 4 * base and errs["batch"] <= 4 * base, (errs, base)
