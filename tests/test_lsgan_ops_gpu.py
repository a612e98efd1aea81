"""Per-kernel parity of lsgan.hip against torch CPU fp64: the fp32 sigmoid, the MSE against a constant
label (the least-squares GANLoss, DSGAN/models/networks.py:148-149) and AvgPool2d(3, 2, 1,
count_include_pad=False) (MultiscaleDiscriminator.downsample, :675), forward and backward.

Bars: sigmoid and mse_const 1e-5 relative, the bar tests/test_ops_gpu.py::test_losses holds the BCE
loss to; the pool 1e-6 relative in norm both ways (a sum of <= 9 fp32 terms and one divide), its two
launch forms and two runs of either bitwise equal.
"""
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

DEV = "cuda"


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


def _leaf(t):
    return t.detach().clone().to(DEV).requires_grad_(True)


def _inputs():
    g = torch.Generator().manual_seed(11)
    yield torch.randn(2, 1, 30, 30, generator=g) * 3
    for n in (1, 1003, 1 << 20):
        yield torch.randn(n, generator=g) * 3


def test_sigmoid_matches_fp64():
    from dsgan_hip import functional as HF
    g = torch.Generator().manual_seed(12)
    for x in _inputs():
        up = torch.randn(x.shape, generator=g)
        xr = x.double().requires_grad_()
        yr = torch.sigmoid(xr)
        yr.backward(up.double())
        xd = _leaf(x)
        y = HF.sigmoid(xd)
        y.backward(up.to(DEV))
        assert y.dtype == torch.float32 and y.shape == x.shape
        assert rel(y, yr) < 1e-5, (tuple(x.shape), rel(y, yr))
        assert rel(xd.grad, xr.grad) < 1e-5, (tuple(x.shape), rel(xd.grad, xr.grad))


def test_sigmoid_finite_at_extremes():
    from dsgan_hip import functional as HF
    x = torch.tensor([40.0, -40.0, 100.0, -100.0, 0.0])
    xd = _leaf(x)
    y = HF.sigmoid(xd)
    y.backward(torch.ones_like(y))
    assert torch.isfinite(y).all() and torch.isfinite(xd.grad).all(), (y, xd.grad)
    assert ((y >= 0) & (y <= 1)).all() and y[4].item() == 0.5
    assert rel(y, torch.sigmoid(x.double())) < 1e-6
    assert (xd.grad >= 0).all() and xd.grad[4].item() == 0.25


def test_mse_const_matches_fp64():
    from dsgan_hip import functional as HF
    for x in _inputs():
        for t in (0.0, 1.0):
            xr = x.double().requires_grad_()
            lr = torch.mean((xr - t) ** 2)
            (lr * 0.75).backward()
            xd = _leaf(x)
            l = HF.mse_const(xd, t)
            (l * 0.75).backward()
            assert l.dim() == 0 and l.dtype == torch.float32
            assert abs(l.item() - lr.item()) <= 1e-5 * abs(lr.item()), (tuple(x.shape), t, l.item(), lr.item())
            assert rel(xd.grad, xr.grad) < 1e-5, (tuple(x.shape), t)
            assert HF.mse_const(xd.detach(), t).item() == l.item()   # fixed-order reduction


def test_elementwise_backwards_accumulate():
    """accumulate=1 adds to the buffer: old + new, the same fp32 add torch does."""
    from dsgan_hip._lib import call, ptr, stream
    g = torch.Generator().manual_seed(13)
    n = 1003
    x, dy, old = (torch.randn(n, generator=g).to(DEV) for _ in range(3))
    y = torch.sigmoid(x)
    gout = torch.tensor(0.5, device=DEV)
    for name, args in (("dsgan_sigmoid_bwd", lambda d, a: (ptr(y), ptr(dy), n, ptr(d), a, stream())),
                       ("dsgan_mse_const_bwd", lambda d, a: (ptr(x), n, 1.0, ptr(gout), ptr(d), a, stream()))):
        new, acc = torch.empty_like(x), old.clone()
        call(name, *args(new, 0))
        call(name, *args(acc, 1))
        assert torch.equal(acc, old + new), name


# every divisor case (4 / 6 / 9 taps, 2 / 3 per axis at a ragged end, 1x1) and both launch forms
POOL_SHAPES = [(2, 6, 8, 8), (1, 3, 7, 9), (1, 1, 1, 1), (1, 2, 2, 3), (2, 6, 64, 64), (1, 3, 5, 8), (1, 2, 6, 12)]


def _pool_ref(x, up):
    xr = x.double().requires_grad_()
    yr = F.avg_pool2d(xr, 3, 2, 1, count_include_pad=False)
    yr.backward(up.double())
    return yr.detach(), xr.grad


def _pool_case(name):
    """(leaf on the device, the view of it the pool reads, the same values on the CPU)"""
    g = torch.Generator().manual_seed(14)
    if name in ("sliced", "sliced_b2"):     # a channel slice of a wider buffer: batch stride != C*H*W
        big = torch.randn(2 if name == "sliced_b2" else 1, 10, 16, 24, generator=g)
        leaf = _leaf(big)
        return leaf, leaf[:, 2:8], big[:, 2:8]
    if name == "offset":     # the pointer one float past a 16-byte boundary
        flat = torch.randn(2 * 3 * 8 * 16 + 1, generator=g)
        leaf = _leaf(flat)
        return leaf, leaf[1:].view(2, 3, 8, 16), flat[1:].view(2, 3, 8, 16)
    x = torch.randn(*name, generator=g)
    leaf = _leaf(x)
    return leaf, leaf, x


def _run_pool(name, fast):
    from dsgan_hip import functional as HF
    leaf, xv, xc = _pool_case(name)
    up = torch.randn(xc.shape[0], xc.shape[1], (xc.shape[2] - 1) // 2 + 1, (xc.shape[3] - 1) // 2 + 1,
                     generator=torch.Generator().manual_seed(15))
    old = HF.AVGPOOL_FAST[0]
    HF.AVGPOOL_FAST[0] = fast
    try:
        y = HF.avg_pool3s2(xv)
        y.backward(up.to(DEV))
    finally:
        HF.AVGPOOL_FAST[0] = old
    dx = leaf.grad
    if name in ("sliced", "sliced_b2"):
        assert dx[:, :2].abs().max().item() == 0 and dx[:, 8:].abs().max().item() == 0
        dx = dx[:, 2:8]
    elif name == "offset":
        dx = dx[1:].view(xc.shape)
    return y.detach(), dx.detach().clone(), xc, up, xv


@pytest.mark.parametrize("name", POOL_SHAPES + ["sliced", "sliced_b2", "offset"], ids=str)
def test_avg_pool3s2_matches_fp64(name):
    y, dx, xc, up, _ = _run_pool(name, True)
    yr, dxr = _pool_ref(xc, up)
    assert y.shape == yr.shape and dx.shape == dxr.shape
    assert rel(y, yr) <= 1e-6, (name, rel(y, yr))
    assert rel(dx, dxr) <= 1e-6, (name, rel(dx, dxr))
    y2, dx2, *_ = _run_pool(name, True)
    assert torch.equal(y, y2) and torch.equal(dx, dx2)


@pytest.mark.parametrize("name", [(2, 6, 8, 8), (2, 6, 64, 64), (1, 2, 6, 12), "sliced", "sliced_b2"], ids=str)
def test_avg_pool3s2_forms_agree_bitwise(name):
    from dsgan_hip import _lib
    yf, dxf, xc, _, xv = _run_pool(name, True)
    ys, dxs, *_ = _run_pool(name, False)
    assert torch.equal(yf, ys) and torch.equal(dxf, dxs)
    # the 16-byte form did apply to the forward wherever W % 8 == 0 (else the comparison is empty)
    N, C, H, W = xc.shape
    xbs = xv.stride(0)
    sup = _lib.load().dsgan_avgpool3s2_fast_supported(xv.data_ptr(), xbs, yf.data_ptr(), yf.stride(0), C, H, W)
    assert bool(sup) == (W % 8 == 0)


def test_avg_pool3s2_forced_form_and_accumulate():
    from dsgan_hip._lib import call, ptr, stream
    g = torch.Generator().manual_seed(16)
    x = torch.randn(2, 3, 10, 16, generator=g).to(DEV)
    ys = [torch.empty(2, 3, 5, 8, device=DEV) for _ in range(3)]
    for form, y in enumerate(ys):
        call("dsgan_avgpool3s2_fwd", ptr(x), 480, ptr(y), 120, 2, 3, 10, 16, form, stream())
    assert torch.equal(ys[0], ys[1]) and torch.equal(ys[0], ys[2])
    odd = torch.randn(1, 1, 5, 7, generator=g).to(DEV)
    with pytest.raises(RuntimeError, match="fast form"):
        call("dsgan_avgpool3s2_fwd", ptr(odd), 35, ptr(torch.empty(1, 1, 3, 4, device=DEV)), 12, 1, 1, 5, 7, 2, stream())
    dy = torch.randn(2, 3, 5, 8, generator=g).to(DEV)
    old = torch.randn(2, 3, 10, 16, generator=g).to(DEV)
    for form in (1, 2):
        new, acc = torch.empty_like(old), old.clone()
        call("dsgan_avgpool3s2_bwd", ptr(dy), 120, ptr(new), 480, 2, 3, 10, 16, 0, form, stream())
        call("dsgan_avgpool3s2_bwd", ptr(dy), 120, ptr(acc), 480, 2, 3, 10, 16, 1, form, stream())
        assert torch.equal(acc, old + new), form


def test_avg_pool3s2_shared_input_sums_both_consumers():
    """An input shared by two consumers (HF.share, as the multi-scale D's input is): the pool's
    backward accumulates into the one gradient buffer."""
    from dsgan_hip import functional as HF
    g = torch.Generator().manual_seed(17)
    x = torch.randn(2, 6, 16, 16, generator=g)
    up = torch.randn(2, 6, 8, 8, generator=g)
    _, dxr = _pool_ref(x, up)
    leaf = _leaf(x)
    s = HF.share(leaf)
    y1, y2 = HF.avg_pool3s2(s), HF.avg_pool3s2(s)
    ((y1 * up.to(DEV)).sum() + (y2 * (2 * up).to(DEV)).sum()).backward()
    assert rel(leaf.grad, 3 * dxr) <= 1e-6
