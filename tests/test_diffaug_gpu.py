"""The --diffaug kernels (csrc/diffaug.hip through functional.diffaug_cat) against dsgan_hip/diffaug.py:
the draws bit for bit, the copy-and-zero ops exactly, the colour arithmetic to the fp32 parity criterion of
the README (1e-3 of the reference's largest magnitude) against float64, and the properties the train step
leans on -- the transpose, the `group` form of a stacked launch, the device-side call counter.

Shapes are the smallest that take every path: W = 24 (16-byte units) and W = 13 (dword units), an even and
an odd cutout size, a non-square image, Cb = 3 and 1 (channels in registers) and Cb = 2, 4 (the generic
channel loop), W = 64 for a shift that is a non-zero multiple of four columns (an aligned shifted unit)."""
import functools

import numpy as np
import pytest
import torch

from dsgan_hip import diffaug as DA

pytestmark = pytest.mark.gpu

FULL, EXACT = "color,translation,cutout", "translation,cutout"
SEED, STREAM = 20, 0xFFFF
CALLS = (0, 1, 2 ** 32 - 1)
# (N, Ca, Cb, H, W)
SHAPES = [(3, Ca, 3, H, W) for Ca in (0, 1, 3) for H, W in ((16, 24), (10, 13))]
SHAPES += [(3, 1, 1, 16, 24), (3, 2, 2, 16, 24), (3, 0, 4, 10, 13), (3, 1, 3, 6, 64)]
PARITY = 1e-3   # README: fp32 parity criterion, relative to the reference's largest magnitude


def _hf():
    import dsgan_hip
    from dsgan_hip import functional as HF
    dsgan_hip.require_gpu()
    return HF


def _state(k=0):
    return _hf().DiffAugState(SEED, STREAM, torch.tensor([k], dtype=torch.int64, device="cuda"))


@functools.lru_cache(maxsize=None)
def _inputs(N, Ca, Cb, H, W):
    """(a, b, dy) on the CPU in fp32: a/b random, dy small integers (exact in any order of addition)."""
    g = torch.Generator().manual_seed(1000 * H + W + 10 * Ca + Cb)
    a = torch.randn((N, Ca, H, W), generator=g) if Ca else None
    b = torch.randn((N, Cb, H, W), generator=g)
    dy = torch.randint(-4, 5, (N, Ca + Cb, H, W), generator=g).float()
    return a, b, dy


@functools.lru_cache(maxsize=None)
def _reference(shape, policy, call):
    """float64 forward and input gradient (w.r.t. the image) of the reference for one call's draws."""
    N, Ca, Cb, H, W = shape
    a, b, dy = _inputs(*shape)
    p = DA.draw_params(SEED, STREAM, call, N, H, W)
    xb = b.double().requires_grad_(True)
    x = torch.cat([a.double(), xb], 1) if Ca else xb
    y = DA.augment_reference(x, Ca, policy, p)
    (g,) = torch.autograd.grad(y, xb, dy.double())
    return y.detach(), g


def _run(shape, policy, call, group=None):
    """(y, db, counter after) from the HIP path."""
    HF = _hf()
    a, b, dy = _inputs(*shape)
    st = _state(call)
    a = a.cuda() if a is not None else None
    b = b.cuda().requires_grad_(True)
    y = HF.diffaug_cat(a, b, policy, st, group=group)
    (g,) = torch.autograd.grad(y, b, dy.cuda())
    torch.cuda.synchronize()
    return y.detach().cpu(), g.cpu(), int(st.counter.item())


def test_the_cases_cover_every_path():
    """What the shapes and calls above are chosen for, checked on the draws themselves (CPU arithmetic)."""
    tx24 = np.concatenate([DA.draw_params(SEED, STREAM, k, 3, 16, 24)["tx"] for k in CALLS])
    assert (tx24 == 0).any() and (tx24 % 4 != 0).any()          # whole 16-byte units and misaligned rows
    tx64 = np.concatenate([DA.draw_params(SEED, STREAM, k, 3, 6, 64)["tx"] for k in CALLS])
    assert ((tx64 % 4 == 0) & (tx64 != 0)).any()                 # an aligned unit of a shifted row
    p = DA.concat_params(*[DA.draw_params(SEED, STREAM, k, 3, 10, 13) for k in CALLS])
    boxes = [DA.cutout_box(oy, ox, 10, 13) for oy, ox in zip(p["oy"], p["ox"])]
    assert any(y1 - y0 < 5 or x1 - x0 < 7 for y0, y1, x0, x1 in boxes)       # a cutout clipped by the border
    assert any(y1 - y0 == 5 and x1 - x0 == 7 for y0, y1, x0, x1 in boxes)    # and a whole one
    assert (p["ty"] < 0).any() and (p["ty"] > 0).any()


@pytest.mark.parametrize("call", CALLS + (2 ** 32 + 5,))
def test_params_equal_the_cpu_draw_bit_for_bit(call):
    HF = _hf()
    for H, W in ((16, 24), (10, 13), (256, 256)):
        got = HF.diffaug_params(SEED, STREAM, call, 300, H, W)
        want = DA.draw_params(SEED, STREAM, call, 300, H, W)
        for f in DA.PARAM_FIELDS:
            assert got[f].dtype == want[f].dtype
            assert np.array_equal(got[f].view(np.int32), want[f].view(np.int32)), (f, H, W)
    other = HF.diffaug_params(SEED + (1 << 40), STREAM, call, 8, 16, 24)   # the key's high word is in use
    assert not np.array_equal(other["b"], DA.draw_params(SEED, STREAM, call, 8, 16, 24)["b"])


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_translation_and_cutout_are_exact(shape):
    """Pure copies and zeros: the forward equals the reference bit for bit, and so does the backward of an
    integer dy."""
    N = shape[0]
    for call in CALLS:
        y, g, ctr = _run(shape, EXACT, call)
        ry, rg = _reference(shape, EXACT, call)
        assert torch.equal(y, ry.float()), call
        assert torch.equal(g, rg.float()), call
        assert ctr == call + 1
    for single in ("translation", "cutout"):
        y, g, _ = _run(shape, single, 1)
        ry, rg = _reference(shape, single, 1)
        assert torch.equal(y, ry.float()) and torch.equal(g, rg.float()), single
    assert N == 3


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_full_policy_meets_fp32_parity(shape):
    worst = [0.0, 0.0]
    for policy in (FULL, "color"):
        for call in CALLS:
            y, g, _ = _run(shape, policy, call)
            ry, rg = _reference(shape, policy, call)
            for i, (got, ref) in enumerate(((y, ry), (g, rg))):
                assert torch.isfinite(got).all()
                worst[i] = max(worst[i], ((got.double() - ref).abs().max() / ref.abs().max()).item())
    print("diffaug %s: max rel err forward %.3g backward %.3g" % (shape, worst[0], worst[1]))
    assert worst[0] <= PARITY and worst[1] <= PARITY, worst
    # zeros are exact zeros, whatever the colour arithmetic does around them
    y, _, _ = _run(shape, FULL, 0)
    ry, _ = _reference(shape, FULL, 0)
    assert torch.equal(y == 0, ry == 0)


@pytest.mark.parametrize("shape", [(3, 1, 3, 16, 24), (3, 0, 3, 10, 13), (3, 2, 2, 16, 24)],
                         ids=lambda s: "x".join(map(str, s)))
def test_backward_is_the_adjoint_of_the_forward(shape):
    """<fwd(a, x) - fwd(a, 0), dy> == <x, bwd(dy)> from the kernels' own outputs (the forward is affine in the
    image: brightness adds a constant), in float64, to the parity criterion of the products' magnitude."""
    HF = _hf()
    N, Ca, Cb, H, W = shape
    a, b, _ = _inputs(*shape)
    g = torch.Generator().manual_seed(5)
    dy = torch.randn((N, Ca + Cb, H, W), generator=g)
    y, gb, _ = _run_with(HF, a, b, dy, FULL, 2)
    y0, _, _ = _run_with(HF, a, torch.zeros_like(b), dy, FULL, 2)
    lhs = ((y.double() - y0.double()) * dy.double()).sum().item()
    rhs = (b.double() * gb.double()).sum().item()
    scale = (b.double() * gb.double()).abs().sum().item()
    print("adjoint %s: lhs %.9g rhs %.9g (|.| sum %.3g): rel %.3g" % (shape, lhs, rhs, scale, abs(lhs - rhs) / scale))
    assert abs(lhs - rhs) <= PARITY * scale


def _run_with(HF, a, b, dy, policy, call, group=None, out=None):
    st = _state(call)
    bb = b.cuda().requires_grad_(True)
    y = HF.diffaug_cat(a.cuda() if a is not None else None, bb, policy, st, group=group, out=out)
    (g,) = torch.autograd.grad(y, bb, dy.cuda())
    torch.cuda.synchronize()
    return y.detach().cpu(), g.cpu(), int(st.counter.item())


@pytest.mark.parametrize("H,W", [(16, 24), (10, 13)])
def test_group_makes_a_stacked_launch_draw_what_two_launches_draw(H, W):
    HF = _hf()
    N, Ca, Cb = 3, 1, 3
    g = torch.Generator().manual_seed(8)
    a, b = torch.randn((2 * N, Ca, H, W), generator=g), torch.randn((2 * N, Cb, H, W), generator=g)
    dy = torch.randn((2 * N, Ca + Cb, H, W), generator=g)
    k = 7
    for policy in (FULL, EXACT):
        y2, g2, c2 = _run_with(HF, a, b, dy, policy, k, group=N)
        st = _state(k)   # two launches from one counter: calls k and k + 1
        halves = []
        for h in (slice(0, N), slice(N, 2 * N)):
            bb = b[h].cuda().requires_grad_(True)
            y = HF.diffaug_cat(a[h].cuda(), bb, policy, st)
            (gg,) = torch.autograd.grad(y, bb, dy[h].cuda())
            halves.append((y.detach().cpu(), gg.cpu()))
        assert c2 == k + 2 and int(st.counter.item()) == k + 2
        assert torch.equal(y2, torch.cat([h[0] for h in halves])) and torch.equal(g2, torch.cat([h[1] for h in halves]))
        assert not torch.equal(y2[:N], _run_with(HF, a[:N], b[:N], dy[:N], policy, k + 1)[0])   # the calls differ
    # N = 3, group = 2: ceil(3 / 2) = 2 calls; samples 0, 1 are indices 0, 1 of call k, sample 2 index 0 of k + 1
    y, gb, c = _run_with(HF, a[:N], b[:N], dy[:N], FULL, k, group=2)
    assert c == k + 2
    y01, g01, _ = _run_with(HF, a[:2], b[:2], dy[:2], FULL, k)
    y2_, g2_, _ = _run_with(HF, a[2:3], b[2:3], dy[2:3], FULL, k + 1)
    assert torch.equal(y, torch.cat([y01, y2_])) and torch.equal(gb, torch.cat([g01, g2_]))
    p = DA.concat_params(DA.draw_params(SEED, STREAM, k, 2, H, W), DA.draw_params(SEED, STREAM, k + 1, 1, H, W))
    ye, _, _ = _run_with(HF, a[:N], b[:N], dy[:N], EXACT, k, group=2)
    assert torch.equal(ye, DA.augment_reference(torch.cat([a[:N], b[:N]], 1), Ca, EXACT, p))


def test_destination_half_of_a_stacked_buffer_and_sliced_source():
    HF = _hf()
    shape = (3, 1, 3, 16, 24)
    N, Ca, Cb, H, W = shape
    a, b, dy = _inputs(*shape)
    want, gwant, _ = _run(shape, FULL, 4)
    # the destination is AB[N:] of a 2N buffer: batch stride == C*H*W, another base; AB[:N] is left alone
    AB = torch.full((2 * N, Ca + Cb, H, W), -7.0, device="cuda")
    y, gb, _ = _run_with(HF, a, b, dy, FULL, 4, out=AB[N:])
    assert torch.equal(y, want) and torch.equal(AB[N:].cpu(), want) and torch.equal(gb, gwant)
    assert (AB[:N] == -7.0).all()
    # ... and a destination whose batch stride exceeds C*H*W: the image channels' worth of a wider buffer
    wide = torch.full((N, Ca + Cb + 2, H, W), -7.0, device="cuda")
    _run_with(HF, a, b, dy, FULL, 4, out=wide[:, :Ca + Cb])
    assert torch.equal(wide[:, :Ca + Cb].cpu(), want) and (wide[:, Ca + Cb:] == -7.0).all()
    # the sources are the channel slices of one concatenated tensor (batch stride (Ca+Cb)*H*W each)
    cat = torch.cat([a, b], 1).cuda()
    st = _state(4)
    bb = cat[:, Ca:].requires_grad_(True)
    y = HF.diffaug_cat(cat[:, :Ca], bb, FULL, st)
    (g,) = torch.autograd.grad(y, bb, dy.cuda())
    assert torch.equal(y.detach().cpu(), want) and torch.equal(g.cpu(), gwant)
    # a dy that is itself a slice of a wider buffer
    st = _state(4)
    bb = b.cuda().requires_grad_(True)
    y = HF.diffaug_cat(a.cuda(), bb, FULL, st)
    dyw = torch.zeros((N, Ca + Cb + 1, H, W), device="cuda")
    dyw[:, :Ca + Cb] = dy.cuda()
    (g,) = torch.autograd.grad(y, bb, dyw[:, :Ca + Cb])
    assert torch.equal(g.cpu(), gwant)


def test_counter_lives_on_the_device():
    HF = _hf()
    shape = (3, 1, 3, 10, 13)
    a, b, _ = _inputs(*shape)
    a, b = a.cuda(), b.cuda()
    st = _state(0)
    with torch.no_grad():
        y0 = HF.diffaug_cat(a, b, FULL, st)
        y1 = HF.diffaug_cat(a, b, FULL, st)
        assert int(st.counter.item()) == 2 and not torch.equal(y0, y1)
        st.counter.zero_()
        assert torch.equal(HF.diffaug_cat(a, b, FULL, st), y0)
        assert torch.equal(HF.diffaug_cat(a, b, FULL, st), y1) and int(st.counter.item()) == 2
        # with the colour off the counter advances all the same (its own small launch)
        HF.diffaug_cat(a, b, "cutout", st)
        assert int(st.counter.item()) == 3
    # the condition gets no gradient, the image does
    aa, bb = a.clone().requires_grad_(True), b.clone().requires_grad_(True)
    HF.diffaug_cat(aa, bb, FULL, st).sum().backward()
    assert aa.grad is None and bb.grad is not None


def test_gradient_box_convention():
    """A shared image (HF.share) collects this op's gradient with its other consumers' in one buffer."""
    HF = _hf()
    shape = (3, 1, 3, 16, 24)
    a, b, dy = _inputs(*shape)
    _, g_aug, _ = _run(shape, FULL, 3)
    leaf = b.cuda().requires_grad_(True)
    (g_tanh,) = torch.autograd.grad(HF.tanh(leaf), leaf, dy[:, 1:].cuda())
    leaf = b.cuda().requires_grad_(True)
    fB = HF.share(leaf)
    y = HF.diffaug_cat(a.cuda(), fB, FULL, _state(3))
    z = HF.tanh(fB)
    ((y * dy.cuda()).sum() + (z * dy[:, 1:].cuda()).sum()).backward()
    assert torch.equal(leaf.grad.cpu(), g_aug + g_tanh.cpu())


def test_host_validation_raises_before_any_launch():
    HF = _hf()
    from dsgan_hip import _lib
    shape = (3, 1, 3, 16, 24)
    N, Ca, Cb, H, W = shape
    a, b, _ = _inputs(*shape)
    a, b = a.cuda(), b.cuda()
    st = _state(5)
    with pytest.raises(RuntimeError, match="group 0"):
        HF.diffaug_cat(a, b, FULL, st, group=0)
    y = torch.zeros((N, Ca + Cb, H, W), device="cuda")
    used = torch.full((1,), -1, dtype=torch.int64, device="cuda")
    ws = torch.empty(_lib.load().dsgan_diffaug_workspace(N, Cb, H, W), device="cuda")
    E = (Ca + Cb) * H * W

    def fwd(ybs=E, bbs=Cb * H * W, ws_elems=ws.numel(), n=N, hh=H):
        _lib.call("dsgan_diffaug_fwd", _lib.ptr(a), Ca * H * W, _lib.ptr(b), bbs, _lib.ptr(y), ybs, n, Ca, Cb, hh, W, 7,
                  SEED, STREAM, _lib.ptr(st.counter), _lib.ptr(used), N, _lib.ptr(ws), ws_elems, _lib.stream())

    with pytest.raises(RuntimeError, match="batch stride below"):
        fwd(ybs=E - 1)
    with pytest.raises(RuntimeError, match="batch stride below"):
        fwd(bbs=Cb * H * W - 4)
    with pytest.raises(RuntimeError, match="scratch of"):
        fwd(ws_elems=ws.numel() - 1)
    with pytest.raises(RuntimeError, match="bad args"):
        fwd(n=0)
    with pytest.raises(RuntimeError, match="bad args"):
        fwd(hh=1)
    with pytest.raises(RuntimeError, match="batch stride below"):
        _lib.call("dsgan_diffaug_bwd", _lib.ptr(y), E - 1, _lib.ptr(b), Cb * H * W, N, Ca, Cb, H, W, 7, SEED, STREAM,
                  _lib.ptr(used), N, _lib.ptr(ws), ws.numel(), _lib.stream())
    cat = torch.cat([a, b], 1)   # a destination that is the source itself: shifted rows would be read after being written
    with pytest.raises(RuntimeError, match="overlaps a source"):
        HF.diffaug_cat(cat[:, :Ca], cat[:, Ca:], FULL, st, out=cat)
    assert torch.equal(cat[:, Ca:], b)
    with pytest.raises(ValueError, match="empty policy"):
        HF.diffaug_cat(a, b, "", st)
    torch.cuda.synchronize()
    assert int(st.counter.item()) == 5 and int(used.item()) == -1 and not y.any()   # nothing ran
    fwd()
    torch.cuda.synchronize()
    assert int(st.counter.item()) == 6 and int(used.item()) == 5 and y.any()
