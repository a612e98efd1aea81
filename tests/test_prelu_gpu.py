"""HF.prelu_cat / HF.prelu (unet.hip) against torch in fp64: y = prelu(cat(a, b), alpha), da, db and
d alpha, with torch CPU's conventions at zero pinned: forward x > 0 ? x : alpha x, dx x > 0 ? g : alpha g,
d alpha sums x g over x <= 0 (an exact 0 adds 0).

Shapes: the single-input form on 1x1 planes, a 2x2 concatenation, 3x3 planes (the 4-byte path), 4x4 with
the tail at a CatSlot offset that is not 16-byte aligned (7 * 16 floats is, so the slot is [N, 7+9, 4, 4]
read through views shifted by one float), and 64x64 with 128 channels (many workgroups per sample).
Bar: TOL["fp32"] = 2e-5 of tests/test_ops_gpu.py for the tensors, and the same for d alpha relative to
sum |x g| (the scale of its summands: the sum itself may cancel).  Two identical calls give identical
bits (the d alpha reduction has a fixed order, no float atomics), and d alpha accumulates into a non-zero
gradient buffer.
"""
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

DEV = "cuda"
TOL = 2e-5

SHAPES = [  # (N, Ca, Cb, H, W, layout)
    (2, 8, 0, 1, 1, "plain"),
    (3, 16, 16, 2, 2, "plain"),
    (2, 5, 3, 3, 3, "plain"),
    (2, 7, 9, 4, 4, "offset"),
    (2, 64, 64, 64, 64, "slot"),
]


@pytest.fixture(scope="module", autouse=True)
def _lib():
    import dsgan_hip
    dsgan_hip.require_gpu()
    yield
    dsgan_hip.set_precision("fp32")


def rel(a, b):
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    return ((a - b).norm() / max(b.norm().item(), 1e-30)).item()


def _inputs(N, Ca, Cb, H, W, seed):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(N, Ca + Cb, H, W, generator=g)
    x.view(-1)[::5] = 0.0          # exact zeros, in both halves
    x.view(-1)[1::7] *= -1.0
    gy = torch.randn(N, Ca + Cb, H, W, generator=g)
    return x, gy


def _place(x, Ca, Cb, layout):
    """(a, b) on the device: plain tensors, the halves of one concatenation buffer ("slot"), or halves
    that start one float past a 16-byte boundary with batch strides that are no multiple of 4 ("offset")."""
    N, _, H, W = x.shape
    if Cb == 0:
        return x.to(DEV).requires_grad_(), None
    if layout == "plain":
        return x[:, :Ca].contiguous().to(DEV).requires_grad_(), x[:, Ca:].contiguous().to(DEV).requires_grad_()
    if layout == "slot":
        from dsgan_hip import functional as HF
        slot = HF.CatSlot(N, Ca, Cb, H, W, torch.empty(0, device=DEV))
        slot.buf.copy_(x.to(DEV))
        return slot.buf[:, :Ca].detach().requires_grad_(), slot.tail().requires_grad_()
    E = (Ca + Cb) * H * W
    store = torch.zeros(N * (E + 1) + 1, device=DEV)
    buf = store[1:1 + N * (E + 1)].view(N, E + 1)[:, :E].view(N, Ca + Cb, H, W)   # batch stride E + 1, base + 4 bytes
    buf.copy_(x.to(DEV))
    assert buf.data_ptr() % 16 == 4 and buf[:, Ca:].data_ptr() % 16 != 0
    return buf[:, :Ca].detach().requires_grad_(), buf[:, Ca:].detach().requires_grad_()


@pytest.mark.parametrize("alpha", [0.25, -0.6])
@pytest.mark.parametrize("N,Ca,Cb,H,W,layout", SHAPES)
def test_prelu_cat_against_fp64(N, Ca, Cb, H, W, layout, alpha):
    from dsgan_hip import functional as HF
    x, gy = _inputs(N, Ca, Cb, H, W, 11 * Ca + Cb + H)
    xr = x.double().requires_grad_()
    ar = torch.tensor([alpha], dtype=torch.float64, requires_grad=True)
    yr = F.prelu(xr, ar)
    yr.backward(gy.double())
    # the conventions at zero, stated independently of torch's kernels
    xd_, gd_ = x.double(), gy.double()
    assert torch.equal(yr.detach(), torch.where(xd_ > 0, xd_, alpha * xd_))
    assert torch.equal(xr.grad, torch.where(xd_ > 0, gd_, alpha * gd_))
    assert abs(float(ar.grad) - float((xd_ * gd_)[xd_ <= 0].sum())) <= 1e-9 * float((xd_ * gd_).abs().sum())

    outs = []
    for rep in range(2):
        a, b = _place(x, Ca, Cb, layout)
        w = torch.nn.Parameter(torch.tensor([alpha], device=DEV))
        w.grad = torch.full((1,), 3.5, device=DEV)   # d alpha is accumulated into what is there
        y = HF.prelu_cat(a, b, w) if b is not None else HF.prelu(a, w)
        y.backward(gy.to(DEV))
        torch.cuda.synchronize()
        outs.append((y.detach().clone(), a.grad.clone(), None if b is None else b.grad.clone(), w.grad.clone()))
    y, da, db, dw = outs[0]
    assert tuple(y.shape) == (N, Ca + Cb, H, W)
    assert rel(y, yr) < TOL
    # exact where nothing is multiplied, and exact zeros stay zeros
    assert torch.equal(y.cpu()[x > 0], x[x > 0]) and (y.cpu()[x == 0] == 0).all()
    dx = da if db is None else torch.cat((da, db), 1)
    assert rel(dx, xr.grad) < TOL
    assert torch.equal(dx.cpu()[x > 0], gy[x > 0])
    scale = float((xd_ * gd_).abs().sum())
    assert abs(float(dw) - 3.5 - float(ar.grad)) <= TOL * scale + 3.5 * 2.0 ** -23, (float(dw) - 3.5, float(ar.grad), scale)
    for t0, t1 in zip(outs[0], outs[1]):
        assert (t0 is None and t1 is None) or torch.equal(t0, t1)


def test_prelu_slope_read_from_device_memory_each_call():
    """The slope is a parameter the optimizer changes in place (under graph replay too): a second call
    after an in-place change of the weight sees the new value."""
    from dsgan_hip import functional as HF
    x = -torch.ones(1, 4, 2, 2, device=DEV)
    w = torch.nn.Parameter(torch.tensor([0.25], device=DEV))
    with torch.no_grad():
        y0 = HF.prelu(x, w).clone()
        w.fill_(-2.0)
        y1 = HF.prelu(x, w)
    assert (y0 == -0.25).all() and (y1 == 2.0).all()
