"""The fused BatchNorm2d + LeakyReLU op (batchnorm.hip, HF.batch_norm) against torch CPU fp64
``F.batch_norm`` + ``leaky_relu(0.2)``, from non-trivial running buffers and gamma / beta.

Shapes: the smallest BatchNorm of the 32x32 net (m = 18), odd unaligned planes with C % 4 != 0 and
N = 3, few channels with a reduction split over workgroups (16-byte and 4-byte accesses), many
channels with short planes, a batch-strided channel slice, and the planner's thresholds (4096 values:
the last shape of the one-workgroup form at few channels; 4608: the first split one).  Together they
take both launch forms (tests/test_batchnorm_cpu.py::test_planner_rules_and_refusals).

Bars: forward tensors 1e-5 relative (torch's CPU fp32 is <= 1.5e-6 on them); backward tensors
max(1e-5, 8 x torch CPU fp32's own error against fp64), 8 being the project's conditioning margin.

LeakyReLU's sign at z ~ 0: one flipped sign changes one element by O(1), which no norm bar survives,
so the fp64 backward reference takes its mask from the GPU forward's ``y > 0`` and a separate
assertion bounds the disagreement between that mask and fp64's own: at most 1e-5 of the elements,
and only where fp64 |z| < 1e-5.  That is a condition on the data, not a measurement: the seeds below
are ones for which torch's CPU fp32 forward itself stays inside it (checked on the CPU for every
case; ``_mask_ok(torch fp32 y, z64)`` holds).  With the offset inputs (x = 30 + N(0, 1)) the mean's
rounding makes flips certain (torch fp32 is 3e-3 off there), so that backward is checked without the
activation.
"""
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

SLOPE = 0.2
# (N, C, H, W), input seed
SHAPES = [((2, 64, 3, 3), 11), ((3, 5, 31, 31), 12), ((2, 4, 128, 128), 13), ((16, 256, 7, 7), 14),
          ((4, 6, 32, 32), 15), ((2, 6, 48, 48), 16), ((2, 3, 129, 129), 17)]
STRIDED = ((2, 12, 31, 31), slice(3, 8), 18)
OFFSET = [((2, 4, 128, 128), 21), ((3, 5, 3, 3), 22)]


def _rel(a, b):
    a, b = a.double().cpu(), b.double().cpu()
    return ((a - b).norm() / max(b.norm().item(), 1e-300)).item()


def _params(C, seed):
    g = torch.Generator().manual_seed(1000 + seed)
    return dict(weight=1.0 + 0.2 * torch.randn(C, generator=g), bias=0.1 * torch.randn(C, generator=g),
                running_mean=0.1 * torch.randn(C, generator=g), running_var=1.0 + 0.2 * torch.rand(C, generator=g))


def _inputs(shape, seed, offset=0.0, n=2):
    g = torch.Generator().manual_seed(seed)
    xs = [offset + torch.randn(shape, generator=g) for _ in range(n)]
    return xs, torch.randn(shape, generator=g)


def _module(C, p, device="cuda"):
    bn = torch.nn.BatchNorm2d(C)
    with torch.no_grad():
        for k, v in p.items():
            getattr(bn, k).copy_(v)
    return bn.to(device)


def _ref_fwd(x, p, dtype, training, act=True):
    """(y, z, mean, rstd, running_mean, running_var) of one forward in ``dtype`` on the CPU."""
    rm, rv = p["running_mean"].clone().to(dtype), p["running_var"].clone().to(dtype)
    x = x.to(dtype)
    z = F.batch_norm(x, rm, rv, p["weight"].to(dtype), p["bias"].to(dtype), training, 0.1, 1e-5)
    if training:
        mean, var = x.mean((0, 2, 3)), x.var((0, 2, 3), unbiased=False)
    else:
        mean, var = p["running_mean"].to(dtype), p["running_var"].to(dtype)
    y = F.leaky_relu(z, SLOPE) if act else z
    return y, z, mean, (var + 1e-5).rsqrt(), rm, rv


def _ref_bwd64(x, dy, p, mask, training):
    """The issue's backward in fp64 with the LeakyReLU mask given (None: no activation)."""
    x, dy = x.double(), dy.double()
    w = p["weight"].double().view(1, -1, 1, 1)
    if training:
        mean, var = x.mean((0, 2, 3), keepdim=True), x.var((0, 2, 3), unbiased=False, keepdim=True)
    else:
        mean, var = p["running_mean"].double().view(1, -1, 1, 1), p["running_var"].double().view(1, -1, 1, 1)
    rstd = (var + 1e-5).rsqrt()
    xh = (x - mean) * rstd
    dz = dy if mask is None else dy * torch.where(mask, 1.0, SLOPE)
    db, dg = dz.sum((0, 2, 3)), (dz * xh).sum((0, 2, 3))
    m = x.numel() / x.shape[1]
    if training:
        dx = w * rstd * (dz - db.view(1, -1, 1, 1) / m - xh * dg.view(1, -1, 1, 1) / m)
    else:
        dx = w * rstd * dz
    return dx, dg, db


def _torch_bwd(x, dy, p, dtype, training, act=True):
    x = x.clone().to(dtype).requires_grad_()
    w, b = p["weight"].clone().to(dtype).requires_grad_(), p["bias"].clone().to(dtype).requires_grad_()
    z = F.batch_norm(x, p["running_mean"].clone().to(dtype), p["running_var"].clone().to(dtype), w, b, training, 0.1, 1e-5)
    (F.leaky_relu(z, SLOPE) if act else z).backward(dy.to(dtype))
    return x.grad.double(), w.grad.double(), b.grad.double()


def _mask_ok(y, z64):
    mism = (y.cpu() > 0) != (z64 > 0)
    return mism.double().mean().item() <= 1e-5 and bool((z64[mism].abs() < 1e-5).all())


def _bars(x, dy, p, training, act=True):
    g32, g64 = _torch_bwd(x, dy, p, torch.float32, training, act), _torch_bwd(x, dy, p, torch.float64, training, act)
    return [max(1e-5, 8 * _rel(a, b)) for a, b in zip(g32, g64)]


def _check_case(x_of, shape, seed, C, training=True):
    """Two training forwards on different inputs, then a backward of the second, through HF.batch_norm.
    x_of(cpu tensor) -> the device tensor the op is given."""
    from dsgan_hip import functional as HF
    p = _params(C, seed)
    (x1, x2), dy = _inputs(shape, seed)
    bn = _module(C, p)
    if not training:
        bn.eval()
    g = torch.Generator().manual_seed(5000 + seed)
    pre_w, pre_b = torch.randn(C, generator=g), torch.randn(C, generator=g)
    bn.weight.grad, bn.bias.grad = pre_w.cuda(), pre_b.cuda()
    before = {k: v.clone() for k, v in bn.state_dict().items()}
    with torch.no_grad():
        HF.batch_norm(x_of(x1), bn, act="lrelu")
    xd = x_of(x2).requires_grad_()
    y = HF.batch_norm(xd, bn, act="lrelu")
    _, mean, rstd = HF.batchnorm_raw(x_of(x2), bn.weight, bn.bias, bn.running_mean.clone(), bn.running_var.clone(),
                                     None, training, 0.1, 1e-5, "lrelu")
    y.backward(dy.cuda())
    torch.cuda.synchronize()
    # fp64 reference of the same two calls
    q = dict(p)
    if training:
        _, _, _, _, q["running_mean"], q["running_var"] = _ref_fwd(x1, p, torch.float64, True)
    y64, z64, mean64, rstd64, rm64, rv64 = _ref_fwd(x2, q, torch.float64, training)
    errs = dict(y=_rel(y, y64), mean=_rel(mean, mean64), rstd=_rel(rstd, rstd64), rm=_rel(bn.running_mean, rm64),
                rv=_rel(bn.running_var, rv64))
    assert _mask_ok(_ref_fwd(x2, q, torch.float32, training)[0], z64), "the seed breaks the mask condition in torch fp32"
    assert _mask_ok(y.detach(), z64)
    dx64, dg64, db64 = _ref_bwd64(x2, dy, q, y.detach().cpu() > 0, training)
    bars = _bars(x2, dy, q, training)
    gerr = [_rel(xd.grad, dx64), _rel(bn.weight.grad, pre_w.double() + dg64), _rel(bn.bias.grad, pre_b.double() + db64)]
    print("\n[batchnorm %s %s] fwd %s; bwd dx %.2e dgamma %.2e dbeta %.2e (bars %.1e %.1e %.1e)" % (
        shape, "train" if training else "eval", " ".join("%s %.2e" % kv for kv in errs.items()), *gerr, *bars))
    assert all(e <= 1e-5 for e in errs.values()), errs
    assert all(e <= b for e, b in zip(gerr, bars)), (gerr, bars)
    if training:
        assert int(bn.num_batches_tracked) == 2 and bn.num_batches_tracked.dtype == torch.int64
    else:
        for k, v in bn.state_dict().items():
            assert torch.equal(v, before[k]), k


@pytest.mark.parametrize("shape,seed", SHAPES)
def test_training_forward_backward(shape, seed):
    _check_case(lambda t: t.cuda(), shape, seed, shape[1])


def test_batch_strided_input():
    shape, sl, seed = STRIDED
    C = sl.stop - sl.start

    def x_of(t):   # t is the slice's data: place it inside a wider buffer
        big = torch.full(shape, 7.0, device="cuda")
        big[:, sl] = t.cuda()
        v = big[:, sl]
        assert not v.is_contiguous()
        return v.detach()

    _check_case(x_of, (shape[0], C) + shape[2:], seed, C)


@pytest.mark.parametrize("shape,seed", [SHAPES[1], SHAPES[2], SHAPES[3]])
def test_eval_mode(shape, seed):
    _check_case(lambda t: t.cuda(), shape, seed, shape[1], training=False)


@pytest.mark.parametrize("shape,seed", OFFSET)
def test_channel_mean_offset(shape, seed):
    """x = 30 + N(0, 1): E[x^2] - E[x]^2 on raw fp32 values is >= 2.4e-5 off here."""
    from dsgan_hip import functional as HF
    C = shape[1]
    p = _params(C, seed)
    (x,), dy = _inputs(shape, seed, offset=30.0, n=1)
    bn = _module(C, p)
    y = HF.batch_norm(x.cuda(), bn, act="lrelu")
    torch.cuda.synchronize()
    y64, _, _, _, rm64, rv64 = _ref_fwd(x, p, torch.float64, True)
    errs = dict(y=_rel(y, y64), rm=_rel(bn.running_mean, rm64), rv=_rel(bn.running_var, rv64))
    bn2 = _module(C, p)
    xd = x.cuda().requires_grad_()
    HF.batch_norm(xd, bn2, act=None).backward(dy.cuda())
    torch.cuda.synchronize()
    dx64, dg64, db64 = _ref_bwd64(x, dy, p, None, True)
    bars = _bars(x, dy, p, True, act=False)
    gerr = [_rel(xd.grad, dx64), _rel(bn2.weight.grad, dg64), _rel(bn2.bias.grad, db64)]
    print("\n[batchnorm offset %s] fwd %s; bwd (no act) dx %.2e dgamma %.2e dbeta %.2e (bars %.1e %.1e %.1e)" % (
        shape, " ".join("%s %.2e" % kv for kv in errs.items()), *gerr, *bars))
    assert all(e <= 1e-5 for e in errs.values()), errs
    assert all(e <= b for e, b in zip(gerr, bars)), (gerr, bars)


@pytest.mark.parametrize("shape,seed", [SHAPES[1], SHAPES[5]])
def test_identical_calls_give_identical_bits(shape, seed):
    from dsgan_hip import functional as HF
    C = shape[1]
    p = _params(C, seed)
    (x,), dy = _inputs(shape, seed, n=1)
    res = []
    for _ in range(2):
        bn = _module(C, p)
        xd = x.cuda().requires_grad_()
        y = HF.batch_norm(xd, bn, act="lrelu")
        y.backward(dy.cuda())
        torch.cuda.synchronize()
        res.append([y.detach(), xd.grad, bn.weight.grad, bn.bias.grad, bn.running_mean, bn.running_var])
    for a, b in zip(*res):
        assert torch.equal(a, b)


@pytest.mark.parametrize("shape,seed", [SHAPES[1], SHAPES[5]])
def test_frozen_parameters(shape, seed):
    """gamma / beta that need no gradient (the G step): their .grad keeps its bits, dx is still right."""
    from dsgan_hip import functional as HF
    C = shape[1]
    p = _params(C, seed)
    (x,), dy = _inputs(shape, seed, n=1)
    bn = _module(C, p)
    bn.weight.grad, bn.bias.grad = torch.randn(C, device="cuda"), torch.randn(C, device="cuda")
    keep = bn.weight.grad.clone(), bn.bias.grad.clone()
    for q in bn.parameters():
        q.requires_grad = False
    xd = x.cuda().requires_grad_()
    y = HF.batch_norm(xd, bn, act="lrelu")
    y.backward(dy.cuda())
    torch.cuda.synchronize()
    assert torch.equal(bn.weight.grad, keep[0]) and torch.equal(bn.bias.grad, keep[1])
    dx64, _, _ = _ref_bwd64(x, dy, p, y.detach().cpu() > 0, True)
    assert _rel(xd.grad, dx64) <= _bars(x, dy, p, True)[0]


def test_one_value_per_channel_raises_before_any_launch():
    from dsgan_hip import functional as HF
    bn = _module(4, _params(4, 1))
    before = {k: v.clone() for k, v in bn.state_dict().items()}
    out = torch.full((1, 4, 1, 1), 7.0, device="cuda")
    x = torch.randn(1, 4, 1, 1, device="cuda")
    with pytest.raises(ValueError, match="Expected more than 1 value per channel when training"):
        HF.batch_norm(x, bn, act="lrelu")
    with pytest.raises(ValueError, match="Expected more than 1 value per channel when training"):
        HF.batchnorm_raw(x, bn.weight, bn.bias, bn.running_mean, bn.running_var, bn.num_batches_tracked, True, out=out)
    torch.cuda.synchronize()
    assert bool((out == 7.0).all())
    for k, v in bn.state_dict().items():
        assert torch.equal(v, before[k]), k
    bn.eval()   # one value per channel is fine with the running statistics
    y = HF.batch_norm(x, bn, act="lrelu")
    want = F.leaky_relu(F.batch_norm(x.cpu().double(), before["running_mean"].cpu().double(),
                                     before["running_var"].cpu().double(), bn.weight.detach().cpu().double(),
                                     bn.bias.detach().cpu().double(), False, 0.1, 1e-5), SLOPE)
    assert _rel(y, want) <= 1e-5
