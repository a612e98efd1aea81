"""pconvt.hip's LDS-DMA ring form (pconvt_ring_kernel) against the register-staged pconvt_kernel
(equal bits: same operand rounding, same MFMA sequence, same order of sums) and against torch's
conv2d_input in float64 on the rounded operands (the bar of test_ops_gpu.py::test_pconvt_bf16, inputs
drawn the same way).  dsgan_pconvt_tune key 0 forces either form; key 1 reports the form a launch took.
"""
import math

import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = "cuda"
HALVES = ["bf16", "fp16"]

# (N, K input channels, M output channels, Hi, Wi, KS)
CASES = [
    (1, 32, 64, 8, 16, 3),     # one K block, one tile, every halo is image border
    (2, 64, 64, 16, 32, 3),    # two K blocks (both ring slots), 2x2 tiles: interior halos, batch stride
    (1, 96, 96, 8, 16, 3),     # odd block count (slot reuse), partial second M tile
    (1, 64, 32, 12, 20, 3),    # Hi no multiple of 8, Wi a multiple of 4 but not of 16, M below the tile
    (2, 64, 32, 16, 16, 4),    # KS 4: top / left halo, the BM = 32 instantiation
    (1, 96, 64, 8, 20, 4),
]


@pytest.fixture(scope="module", autouse=True)
def _lib():
    import dsgan_hip
    dsgan_hip.require_gpu()
    yield
    dsgan_hip.set_precision("fp32")


def rel(a, b):
    a = a.detach().double().cpu()
    b = b.detach().double().cpu()
    return ((a - b).norm() / max(b.norm().item(), 1e-30)).item()


def _q(t, half):
    return t.to(torch.float16 if half == "fp16" else torch.bfloat16).float()


_REF = {}


def _case(half, N, K, M, Hi, Wi, KS):
    """Rounded operands, bias and the float64 reference of one case: computed once, shared, read only."""
    key = (half, N, K, M, Hi, Wi, KS)
    if key not in _REF:
        g = torch.Generator().manual_seed(K + M + KS + Hi)
        dy = _q(torch.randn(N, K, Hi, Wi, generator=g), half)
        w = _q(torch.randn(K, M, KS, KS, generator=g) / math.sqrt(K * KS * KS / 4), half)
        b = torch.randn(M, generator=g) * 0.1
        ref = torch.nn.grad.conv2d_input((N, M, 2 * Hi, 2 * Wi), w.double(), dy.double(), stride=2, padding=1)
        _REF[key] = (dy, w, b, ref)
    return _REF[key]


def _both(run):
    """run() under the register-staged kernel and under the ring; returns (parent, ring, form of the ring run)."""
    from dsgan_hip import _lib as L
    lib = L.load()
    old = lib.dsgan_pconvt_tune(0, -1)
    try:
        lib.dsgan_pconvt_tune(0, 2)
        a = run()
        assert lib.dsgan_pconvt_tune(1, -1) == 0
        lib.dsgan_pconvt_tune(0, 1)
        b = run()
        form = lib.dsgan_pconvt_tune(1, -1)
    finally:
        lib.dsgan_pconvt_tune(0, old)
    return a, b, form


@pytest.mark.parametrize("N,K,M,Hi,Wi,KS", CASES)
@pytest.mark.parametrize("half", HALVES)
def test_pconvt_ring(half, N, K, M, Hi, Wi, KS):
    from dsgan_hip import functional as HF
    HF.set_precision(half)
    dy, w, b, ref = _case(half, N, K, M, Hi, Wi, KS)
    dyd, wd, bd = dy.to(DEV), w.to(DEV), b.to(DEV)
    shape = (N, M, 2 * Hi, 2 * Wi)
    par, ring, form = _both(lambda: HF.conv_dgrad_raw(dyd, wd, shape, 2, 1, bias=bd))
    assert form == 1
    assert torch.equal(par, ring)
    assert rel(ring, ref + b.double().view(1, -1, 1, 1)) < 1e-5


@pytest.mark.parametrize("half", HALVES)
def test_pconvt_ring_channel_slices(half):
    """x and y are channel slices of larger buffers: x_bs / y_bs larger than dense."""
    from dsgan_hip import functional as HF
    HF.set_precision(half)
    N, K, M, Hi, Wi, KS = CASES[1]
    dy, w, b, ref = _case(half, N, K, M, Hi, Wi, KS)
    xbuf = torch.zeros(N, K + 32, Hi, Wi, device=DEV)
    xbuf[:, 32:] = dy.to(DEV)
    wd, bd = w.to(DEV), b.to(DEV)
    shape = (N, M, 2 * Hi, 2 * Wi)

    def run():
        ybuf = torch.full((N, M + 8, 2 * Hi, 2 * Wi), 7.0, device=DEV)
        HF.conv_dgrad_raw(xbuf[:, 32:], wd, shape, 2, 1, bias=bd, out=ybuf[:, 8:])
        return ybuf

    par, ring, form = _both(run)
    assert form == 1
    assert torch.equal(par, ring)
    assert torch.equal(ring[:, :8].cpu(), torch.full((N, 8, 2 * Hi, 2 * Wi), 7.0))
    assert rel(ring[:, 8:], ref + b.double().view(1, -1, 1, 1)) < 1e-5


@pytest.mark.parametrize("half", HALVES)
def test_pconvt_ring_gpre_accumulate(half):
    """act'(gpre) (lrelu) and accumulate, as test_pconvt_bf16 does."""
    from dsgan_hip import functional as HF
    HF.set_precision(half)
    N, K, M, Hi, Wi, KS = CASES[4]
    dy, w, b, ref = _case(half, N, K, M, Hi, Wi, KS)
    g = torch.Generator().manual_seed(11)
    shape = (N, M, 2 * Hi, 2 * Wi)
    pre = torch.randn(shape, generator=g)
    y0 = torch.randn(shape, generator=g)
    dyd, wd, pred = dy.to(DEV), w.to(DEV), pre.to(DEV)

    def run():
        out = y0.to(DEV)
        HF.conv_dgrad_raw(dyd, wd, shape, 2, 1, gpre=pred, gact="lrelu", out=out, accumulate=True)
        return out

    par, ring, form = _both(run)
    assert form == 1
    assert torch.equal(par, ring)
    want = y0.double() + ref * torch.where(pre > 0, 1.0, 0.2).double()
    assert rel(ring, want) < 1e-5


def test_pconvt_ring_ineligible_falls_back():
    """Wi = 18 (no multiple of 4): the knob cannot put the shape on the ring; equal bits either way."""
    from dsgan_hip import functional as HF
    HF.set_precision("bf16")
    N, K, M, Hi, Wi, KS = 2, 64, 32, 17, 18, 4
    dy, w, b, ref = _case("bf16", N, K, M, Hi, Wi, KS)
    dyd, wd = dy.to(DEV), w.to(DEV)
    par, ring, form = _both(lambda: HF.conv_dgrad_raw(dyd, wd, (N, M, 2 * Hi, 2 * Wi), 2, 1))
    assert form == 0
    assert torch.equal(par, ring)
    assert rel(ring, ref) < 1e-5
