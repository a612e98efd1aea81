"""The generator's moving average fused into the Adam kernel (dsgan_adam_ema / dsgan_adam_amp_ema), the
in-place exchange dsgan_swap, and FlatAdam(ema_decay=...) on them.

Bars.  p, m, v: bitwise those of dsgan_adam / dsgan_adam_amp.  The average against the float64 recurrence
e <- e + (1 - d)(p_k - e) driven by the kernel's own p_k: K * 2^-22 * max(|p|, |e|) after K steps -- one
step's lerp rounds three times (the difference, the product, the sum; two with a contracted multiply-add)
on operands no larger than 2 * max, each rounding at most 2^-24 relative, and the error carried over
from earlier steps shrinks by d.  The decay is 0.5 (at 0.999 and lr 2e-4 one step moves the average by
about 2e-7 of its size, the size of fp32 rounding: a missing update could hide inside the bar), and 0.9
so that both branches of at::lerp's form (weight below / not below 0.5) run.
"""
import pytest
import torch

gpu = pytest.mark.gpu
DEV = "cuda"
LR, B1, B2, EPS = 1e-2, 0.5, 0.999, 1e-8
SENTINEL = -77.25


def _call(name, *a):
    from dsgan_hip import _lib
    _lib.call(name, *a)


class Bufs:
    """p, g, m, v, ema as runs of n elements at element offset ``off`` of sentinel-filled device
    buffers (off 0: 16-byte aligned, the float4 body; off 1: the one-element-per-lane body)."""
    NAMES = ("p", "g", "m", "v", "ema")

    def __init__(self, n, off, seed):
        gen = torch.Generator().manual_seed(seed)
        self.n, self.off = n, off
        self.big = {}
        for k in self.NAMES:
            b = torch.full((n + 8,), SENTINEL, dtype=torch.float32)
            x = torch.randn(n, generator=gen)
            if k == "v":
                x = x * x * 1e-2
            elif k == "m":
                x = x * 0.1
            b[off:off + n] = x
            self.big[k] = b.to(DEV)
        assert all(b.data_ptr() % 16 == 0 for b in self.big.values())

    def ptr(self, k):
        return self.big[k].data_ptr() + 4 * self.off

    def get(self, k):
        return self.big[k][self.off:self.off + self.n]

    def set_grad(self, g):
        self.big["g"][self.off:self.off + self.n] = g.to(DEV)

    def guards_intact(self):
        for b in self.big.values():
            rest = torch.cat((b[:self.off], b[self.off + self.n:]))
            if not bool((rest == SENTINEL).all()):
                return False
        return True

    def clone(self):
        c = Bufs.__new__(Bufs)
        c.n, c.off = self.n, self.off
        c.big = {k: v.clone() for k, v in self.big.items()}
        return c


def _state(k, skip=0.0, scale=4.0):
    """The scaler's device state ahead of applied step k: {scale, skip, clean steps, 1/scale, steps}."""
    return torch.tensor([scale, skip, 0.0, 1.0 / scale, float(k)], device=DEV, dtype=torch.float32)


def _step(b, k, amp, ema_decay=None, skip=0.0):
    """Step k on the buffers ``b`` through the plain (ema_decay None) or the _ema entry point."""
    head = (b.ptr("p"), b.ptr("g"), b.ptr("m"), b.ptr("v"))
    if amp:
        st = _state(k, skip)
        if ema_decay is None:
            _call("dsgan_adam_amp", *head, b.n, LR, B1, B2, EPS, st.data_ptr(), None)
        else:
            _call("dsgan_adam_amp_ema", *head, b.ptr("ema"), b.n, LR, B1, B2, EPS, ema_decay, st.data_ptr(), None)
        torch.cuda.synchronize()
    elif ema_decay is None:
        _call("dsgan_adam", *head, b.n, LR, B1, B2, EPS, k, None)
    else:
        _call("dsgan_adam_ema", *head, b.ptr("ema"), b.n, LR, B1, B2, EPS, ema_decay, k, None)


def _trajectory(n, off, amp, decay, K=5, seed=3):
    """K steps on twin buffers: the plain entry point on one, the _ema one on the other.  Returns the
    _ema buffers, the initial average and the p snapshots, after asserting p, m, v bitwise equal."""
    a = Bufs(n, off, seed)
    b = a.clone()
    e0 = b.get("ema").clone()
    snaps = []
    gen = torch.Generator().manual_seed(seed + 100)
    for k in range(1, K + 1):
        g = torch.randn(n, generator=gen) * (4.0 if amp else 1.0)   # (the AMP form divides by its scale, 4)
        a.set_grad(g)
        b.set_grad(g)
        _step(a, k, amp)
        _step(b, k, amp, decay)
        for name in ("p", "m", "v"):
            assert torch.equal(a.get(name), b.get(name)), (name, k)
        assert torch.equal(a.get("ema"), e0)   # the plain form never touches it
        snaps.append(b.get("p").clone())
    assert a.guards_intact() and b.guards_intact()
    return b, e0, snaps


@gpu
@pytest.mark.parametrize("decay", [0.5, 0.9])
@pytest.mark.parametrize("amp", [False, True])
def test_ema_entry_points(amp, decay):
    n, K = 1027, 5
    b, e0, snaps = _trajectory(n, 0, amp, decay, K)
    ema = b.get("ema")
    assert not torch.equal(ema, e0)
    assert not torch.equal(ema, snaps[-1])
    ref = e0.double()
    big = float(e0.abs().max())
    for p in snaps:
        ref = ref + (1.0 - decay) * (p.double() - ref)
        big = max(big, float(p.abs().max()), float(ref.abs().max()))
    err = float((ema.double() - ref).abs().max())
    moved = float((ema - e0).abs().max())
    print("amp %d decay %g: max|ema - ref64| = %.3g, bar %.3g, moved by %.3g" % (amp, decay, err, K * 2.0 ** -22 * big, moved))
    assert err <= K * 2.0 ** -22 * big
    assert moved > 1e3 * K * 2.0 ** -22 * big   # the bar could not hide a missing update


@gpu
@pytest.mark.parametrize("amp", [False, True])
@pytest.mark.parametrize("n", [1027, 3, 0])
def test_vector_and_scalar_paths_same_bits(n, amp):
    """The same data at a 16-byte-aligned base (float4 body + tail) and one element further on."""
    va, e0, _ = _trajectory(n, 0, amp, 0.5, K=2)
    sc, _, _ = _trajectory(n, 1, amp, 0.5, K=2)
    for name in Bufs.NAMES:
        assert torch.equal(va.get(name), sc.get(name)), name
    if n:
        assert not torch.equal(va.get("ema"), e0)


@gpu
@pytest.mark.parametrize("off", [0, 1])
def test_skipped_amp_step_leaves_everything(off):
    b = Bufs(1027, off, 5)
    before = b.clone()
    _step(b, 1, True, 0.5, skip=1.0)
    for name in Bufs.NAMES:
        assert torch.equal(b.big[name], before.big[name]), name
    _step(b, 1, True, 0.5)   # the same call, not skipped, does move them
    for name in ("p", "m", "v", "ema"):
        assert not torch.equal(b.get(name), before.get(name)), name
    assert b.guards_intact()


@gpu
def test_flat_adam_guard_skips_the_average_too():
    from dsgan_hip.amp import LossScaler
    from dsgan_hip.flat import FlatAdam, FlatParams
    torch.manual_seed(1)
    net = torch.nn.Sequential(torch.nn.Linear(7, 5), torch.nn.Linear(5, 3))
    flat = FlatParams(net, torch.device(DEV))
    assert FlatAdam(flat, lr=1e-2).ema is None   # off: nothing allocated
    opt = FlatAdam(flat, lr=1e-2, betas=(0.5, 0.999), scaler=LossScaler.guard(torch.device(DEV)), ema_decay=0.5)
    assert opt.ema.shape == flat.data.shape and opt.ema.data_ptr() != flat.data.data_ptr()
    assert torch.equal(opt.ema, flat.data)
    p0 = flat.data.clone()
    flat.grad.copy_(torch.randn(flat.numel))
    flat.grad[3] = float("inf")
    opt.scaler.check(flat.grad)
    opt.step()
    assert torch.equal(flat.data, p0) and torch.equal(opt.ema, p0)
    assert opt.scaler.applied_steps() == 0
    flat.grad.copy_(torch.randn(flat.numel))
    opt.scaler.check(flat.grad)
    opt.step()
    assert opt.scaler.applied_steps() == 1
    assert not torch.equal(flat.data, p0) and not torch.equal(opt.ema, p0) and not torch.equal(opt.ema, flat.data)
    ref = p0.double() + 0.5 * (flat.data.double() - p0.double())
    assert float((opt.ema.double() - ref).abs().max()) <= 2.0 ** -22 * float(torch.maximum(p0.abs(), flat.data.abs()).max())
    # the views follow the layout: each parameter's run of the buffer, in its shape
    views = list(opt.ema_views(net))
    assert [id(p) for p, _ in views] == [id(p) for p in net.parameters()]
    for p, e in views:
        assert e.shape == p.shape and e.data_ptr() - opt.ema.data_ptr() == p.data_ptr() - flat.data.data_ptr()
    opt.reset_ema()
    assert torch.equal(opt.ema, flat.data)
    with pytest.raises(ValueError):
        FlatAdam(flat, ema_decay=1.0)


@gpu
@pytest.mark.parametrize("off", [0, 1])
@pytest.mark.parametrize("n", [1027, 3, 0])
def test_swap(n, off):
    gen = torch.Generator().manual_seed(n + off)
    a = torch.full((n + 8,), SENTINEL)
    b = torch.full((n + 8,), SENTINEL)
    a[off:off + n] = torch.randn(n, generator=gen)
    b[off:off + n] = torch.randn(n, generator=gen)
    a0, b0 = a.clone(), b.clone()
    a, b = a.to(DEV), b.to(DEV)
    _call("dsgan_swap", a.data_ptr() + 4 * off, b.data_ptr() + 4 * off, n, None)
    assert torch.equal(a.cpu(), b0) and torch.equal(b.cpu(), a0)   # the runs exchanged, the sentinels untouched
    _call("dsgan_swap", a.data_ptr() + 4 * off, b.data_ptr() + 4 * off, n, None)
    assert torch.equal(a.cpu(), a0) and torch.equal(b.cpu(), b0)


def test_argument_validation_runs_on_the_host():
    """No device memory and no launch: the pointers are never read."""
    x = 4096
    for name, tail in (("dsgan_adam_ema", (1, None)), ("dsgan_adam_amp_ema", (x, None))):
        with pytest.raises(RuntimeError, match="ema is null"):
            _call(name, x, x, x, x, None, 8, LR, B1, B2, EPS, 0.5, *tail)
        for bad in (1.0, -0.1, float("nan")):
            with pytest.raises(RuntimeError, match="ema_decay"):
                _call(name, x, x, x, x, x, 8, LR, B1, B2, EPS, bad, *tail)
    with pytest.raises(RuntimeError, match="bad args"):
        _call("dsgan_swap", None, x, 8, None)
    with pytest.raises(RuntimeError, match="overlap"):
        _call("dsgan_swap", x, x + 16, 8, None)
