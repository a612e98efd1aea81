"""The ConvNeXt block tail (mlp.hip): the forward that takes the block's 1x1 shortcut into the MLP
kernel (dsgan_mlp_fwd_sc) against the shortcut GEMM + dsgan_mlp_fwd pair."""
import math

import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = "cuda"
HALVES = ["bf16", "fp16"]


@pytest.fixture(scope="module", autouse=True)
def _lib():
    import dsgan_hip
    dsgan_hip.require_gpu()
    yield
    dsgan_hip.set_precision("fp32")


def _hdt(half):
    return torch.float16 if half == "fp16" else torch.bfloat16


def _leaf(t):
    return t.detach().clone().to(DEV).requires_grad_(True)


def _param(t):
    p = torch.nn.Parameter(t.detach().clone().to(DEV))
    p.grad = torch.zeros_like(p)
    return p


def _tail_inputs(half, N, C, P, H, seed):
    g = torch.Generator().manual_seed(seed)
    t = dict(h=torch.randn(N, C, H, H, generator=g), x=torch.randn(N, C, H, H, generator=g),
             w1=torch.randn(4 * C, C, generator=g) / math.sqrt(C), b1=torch.randn(4 * C, generator=g) * 0.1,
             w2=torch.randn(P, 4 * C, generator=g) / math.sqrt(4 * C), b2=torch.randn(P, generator=g) * 0.1,
             ws=torch.randn(P, C, 1, 1, generator=g) / math.sqrt(C), acc=torch.randn(N, P, H, H, generator=g),
             gy=torch.randn(N, P, H, H, generator=g))
    return t


def _tail_ref(t, half, with_acc):
    """fp64 on the 16-bit-rounded operands (h, x and the three weights): shortcut + MLP, exact erf GELU"""
    hd = _hdt(half)
    r = lambda v: v.to(DEV).to(hd).double()
    h, x, w1, w2 = r(t["h"]), r(t["x"]), r(t["w1"]), r(t["w2"])
    ws = r(t["ws"])[:, :, 0, 0]
    z = torch.einsum("kc,nchw->nkhw", w1, h) + t["b1"].to(DEV).double()[None, :, None, None]
    gz = 0.5 * z * (1 + torch.erf(z / math.sqrt(2)))
    out = torch.einsum("pk,nkhw->nphw", w2, gz) + t["b2"].to(DEV).double()[None, :, None, None]
    out = out + torch.einsum("pc,nchw->nphw", ws, x)
    return out + t["acc"].to(DEV).double() if with_acc else out


def _run_tail(HF, t, form, fold, misalign=False):
    """One forward + backward of pw_mlp; returns (y, [grads], names of the C-ABI calls made)."""
    N, C, H, _ = t["h"].shape
    P = t["w2"].shape[0]
    hd_, Q = _leaf(t["h"]), [_param(t[k]) for k in ("w1", "b1", "w2", "b2", "ws")]
    leaves = [hd_]
    slot = acc = None
    if form == "slot":
        # out is the channel tail of a [N, 2P] buffer, x the channel tail of a [N, 2C] one: both batch
        # strides are twice the dense ones
        xw = _leaf(torch.cat([torch.zeros_like(t["x"]), t["x"]], 1))
        xd = xw[:, C:]
        assert xd.stride(0) == 2 * C * H * H and xd.data_ptr() % 16 == 0
        slot = HF.CatSlot(N, P, P, H, H, hd_)
        leaves.append(xw)
    elif misalign:
        flat = _leaf(torch.cat([torch.zeros(1), t["x"].reshape(-1), torch.zeros(3)]))
        xd = flat[1:1 + t["x"].numel()].view(N, C, H, H)
        assert xd.data_ptr() % 16 == 4
        leaves.append(flat)
    else:
        xd = _leaf(t["x"])
        leaves.append(xd)
    if form == "acc":
        ad = _leaf(t["acc"])
        acc = ad * 1.0   # a non-leaf acc, as the local branch's output is
        leaves.append(ad)
    names, orig, old = [], HF.call, HF.MLP_FOLD_SC[0]

    def rec(name, *a):
        names.append(name)
        return orig(name, *a)

    HF.call, HF.MLP_FOLD_SC[0] = rec, fold
    try:
        y = HF.pw_mlp(hd_, xd, *Q, slot=slot, acc=acc)
        if form == "slot":
            assert slot.holds(y, P) and y.stride(0) == 2 * P * H * H
        fwd_names = list(names)
        y.backward(t["gy"].to(DEV))
        torch.cuda.synchronize()
    finally:
        HF.call, HF.MLP_FOLD_SC[0] = orig, old
    return y.detach().clone(), [v.grad.clone() for v in leaves] + [q.grad.clone() for q in Q], fwd_names


SHAPES = [(64, 128, 2, 16), (128, 256, 2, 16), (256, 128, 2, 16), (128, 64, 2, 16), (128, 64, 3, 32)]


@pytest.mark.parametrize("half", HALVES)
@pytest.mark.parametrize("form", ["dense", "slot", "acc"])
@pytest.mark.parametrize("C,P,N,H", SHAPES)
def test_mlp_fwd_folded_shortcut(half, form, C, P, N, H):
    """pw_mlp with the shortcut inside the MLP forward kernel, for a dense out, out / x as channel
    tails of wider buffers, and out summed into acc.
    (a) Its error against fp64 on the same 16-bit-rounded operands is at most twice the error of the
        two-launch path against that reference, measured here (L2-relative and max-abs): the two
        can differ only in the association of the same fp32 partial sums.
        The kernel forms Ws x the way the pointwise GEMM does (one accumulator from zero, channel
        steps ascending) and adds it where the GEMM's output was added, so wherever that GEMM runs
        its whole K in one workgroup the output is bitwise the two-launch one.  That holds for
        C <= 128 at these sizes and is asserted; at C = 256 the small test shapes make the GEMM split
        K (the step's 128^2 shape does not: tools/mlp_micro.py prints the comparison there).
    (b) Every gradient is bitwise that of the two-launch run: the backward never reads out.
    Measured on MI355X (profiles/r07/tail_tests.txt), C=128 P=64 N=3 H=32, dense, L2-relative / max-abs:
    bf16 two-launch 9.047e-04 / 7.604e-03, folded the same bits; C=256 P=128 N=2 H=16 bf16: 9.073e-04 /
    5.789e-03 both ways; fp16 two-launch 1.130e-04 / 7.310e-04, folded 1.130e-04 / 7.309e-04."""
    from dsgan_hip import functional as HF
    HF.set_precision(half)
    t = _tail_inputs(half, N, C, P, H, seed=C + P + H + N)
    ref = _tail_ref(t, half, form == "acc")
    y0, g0, n0 = _run_tail(HF, t, form, fold=False)
    y1, g1, n1 = _run_tail(HF, t, form, fold=True)
    assert "dsgan_mlp_fwd" in n0 and "dsgan_mlp_fwd_sc" not in n0, n0
    assert n1.count("dsgan_mlp_fwd_sc") == 1 and "dsgan_mlp_fwd" not in n1, n1
    assert not any(n.startswith("dsgan_pw_") for n in n1), n1   # no shortcut GEMM beside it
    scale = ref.norm().item()
    e0 = ((y0.double() - ref).norm().item() / scale, (y0.double() - ref).abs().max().item())
    e1 = ((y1.double() - ref).norm().item() / scale, (y1.double() - ref).abs().max().item())
    print("tail %s %s C=%d P=%d N=%d H=%d: two-launch rel %.3e max %.3e | folded rel %.3e max %.3e | same bits %s"
          % (half, form, C, P, N, H, e0[0], e0[1], e1[0], e1[1], torch.equal(y0, y1)))
    assert e1[0] <= 2 * e0[0] and e1[1] <= 2 * e0[1], (e0, e1)
    if C <= 128:
        assert torch.equal(y1, y0)
    for i, (a, b) in enumerate(zip(g1, g0)):
        assert torch.equal(a, b), i


@pytest.mark.parametrize("half", HALVES)
@pytest.mark.parametrize("C,P,N,H", SHAPES[:4])
def test_mlp_fwd_misaligned_x_takes_two_launches(half, C, P, N, H):
    """(c) An x whose pointer is 4 bytes off a 16-byte boundary never reaches dsgan_mlp_fwd_sc, and
    the result and every gradient are bitwise what the toggle-off run gives."""
    from dsgan_hip import functional as HF
    HF.set_precision(half)
    t = _tail_inputs(half, N, C, P, H, seed=C + P + H + N)
    y0, g0, n0 = _run_tail(HF, t, "dense", fold=False, misalign=True)
    y1, g1, n1 = _run_tail(HF, t, "dense", fold=True, misalign=True)
    assert "dsgan_mlp_fwd_sc" not in n1 and n1 == n0, (n0, n1)
    assert torch.equal(y1, y0)
    for i, (a, b) in enumerate(zip(g1, g0)):
        assert torch.equal(a, b), i
