"""HF.conv_transpose4s2 (nn.ConvTranspose2d(k4, s2, p1), the U-Net's up convs): forward, dx, dw, db
against F.conv_transpose2d in fp64, in every precision mode, with TOL of tests/test_ops_gpu.py used as
its test_conv_transpose uses it for the 3x3 form (the 16-bit modes see pre-rounded x and w; the
gradients carry one more in-kernel rounding, of dy: 2 x TOL; the bias grad is a plain fp32 sum: 1e-5).

Shapes: the 1x1 bottleneck, 2x2 from a 128-channel concatenation, 4x4 without a bias, the 3-channel head
with its bias, and a 16 -> 8 channel layer no MFMA family takes.  conv_transpose3s2 is untouched by the
generalisation (ConvT4s2Fn is ConvT3s2Fn, which reads the kernel size off the weight): the 4x4 entry on a
3x3-shaped problem is refused, and the 3x3 entry gives the same bits through either class name.
"""
import math

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

DEV = "cuda"
TOL = {"fp32": 2e-5, "bf16": 1.5e-2, "fp16": 3e-3}   # tests/test_ops_gpu.py
HDT = {"bf16": torch.bfloat16, "fp16": torch.float16}


@pytest.fixture(scope="module", autouse=True)
def _lib():
    import dsgan_hip
    dsgan_hip.require_gpu()
    yield
    dsgan_hip.set_precision("fp32")


def rel(a, b):
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    return ((a - b).norm() / max(b.norm().item(), 1e-30)).item()


def _q(t, prec):
    return t.to(HDT[prec]).float() if prec in HDT else t


def _param(t):
    p = torch.nn.Parameter(t.detach().clone().to(DEV))
    p.grad = torch.zeros_like(p)
    return p


@pytest.mark.parametrize("prec", ["fp32", "bf16", "fp16"])
@pytest.mark.parametrize("N,Ci,H,Co,bias", [(2, 64, 1, 64, True), (2, 128, 2, 64, True), (2, 32, 4, 32, False),
                                            (1, 64, 8, 3, True), (2, 16, 4, 8, True)])
def test_conv_transpose4s2(prec, N, Ci, H, Co, bias):
    from dsgan_hip import functional as HF
    HF.set_precision(prec)
    g = torch.Generator().manual_seed(Ci + Co + H)
    x = _q(torch.randn(N, Ci, H, H, generator=g), prec)
    w = _q(torch.randn(Ci, Co, 4, 4, generator=g) / math.sqrt(Ci * 4), prec)
    b = torch.randn(Co, generator=g) * 0.1 if bias else None
    xr, wr = x.double().requires_grad_(), w.double().requires_grad_()
    br = b.double().requires_grad_() if bias else None
    y_ref = F.conv_transpose2d(xr, wr, br, stride=2, padding=1)
    gy = torch.randn(y_ref.shape, generator=g)
    y_ref.backward(gy.double())
    xd, wd, bd = x.clone().to(DEV).requires_grad_(), _param(w), (_param(b) if bias else None)
    y = HF.conv_transpose4s2(xd, wd, bd)
    y.backward(gy.to(DEV))
    torch.cuda.synchronize()
    tol = TOL[prec]
    assert tuple(y.shape) == (N, Co, 2 * H, 2 * H) == tuple(y_ref.shape)
    assert rel(y, y_ref) < tol
    assert rel(xd.grad, xr.grad) < 2 * tol
    assert rel(wd.grad, wr.grad) < 2 * tol
    if bias:
        assert rel(bd.grad, br.grad) < 1e-5


def test_conv_transpose3s2_keeps_its_bits():
    from dsgan_hip import functional as HF
    HF.set_precision("bf16")
    g = torch.Generator().manual_seed(104)
    x = torch.randn(2, 64, 8, 9, generator=g).to(DEV)
    w = torch.randn(64, 32, 3, 3, generator=g) / 24.0
    b = torch.randn(32, generator=g) * 0.1
    gy = torch.randn(2, 32, 16, 18, generator=g).to(DEV)
    outs = []
    for fn in (HF.conv_transpose3s2, HF.ConvT3s2Fn.apply, HF.ConvT4s2Fn.apply):
        xd, wd, bd = x.clone().requires_grad_(), _param(w), _param(b)
        y = fn(xd, wd, bd)
        y.backward(gy)
        torch.cuda.synchronize()
        outs.append((y.detach().clone(), xd.grad.clone(), wd.grad.clone(), bd.grad.clone()))
    for other in outs[1:]:
        for a, c in zip(outs[0], other):
            assert torch.equal(a, c)
    # the value tests/test_ops_gpu.py::test_conv_transpose checks for this op, on its (2, 64, 32, 8) shape
    y_ref = F.conv_transpose2d(x.cpu().to(torch.bfloat16).double(), w.to(torch.bfloat16).double(), b.double(), stride=2,
                               padding=1, output_padding=1)
    assert rel(outs[0][0], y_ref) < TOL["bf16"]
    with pytest.raises(ValueError):
        HF.conv_transpose4s2(x, _param(w), None)
