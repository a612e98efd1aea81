"""dsgan_sn_refresh / dsgan_sn_backward (csrc/spectral.hip) against dsgan_hip.spectral's float64 reference on
the same fp32 inputs, layer by layer and all layers in one batched call.

Only the fp32 summation order separates kernel and reference, so the bar is the format's own cost: the
test runs the reference in numpy float32 too, measures its deviation from float64 per quantity, and allows
the kernels 8x the largest such deviation over the shapes (the device adds in another order, over the same
lengths).  Measured on these inputs: numpy fp32 is off by 5.4e-8 (sigma, relative), 3.6e-8 / 4.5e-8 (u / v),
1.1e-7 (W_sn, of its max) and 1.2e-7 (projected gradient, of its max); the kernels by 8.8e-8, 3.4e-8 / 2.9e-8,
1.2e-7 and 1.4e-7 ("Spectral normalisation").
Determinism is checked bit for bit: batched against single calls, two runs, iterate=False after an iterating
call, the zeroed scratch, and two accumulating backwards."""
import numpy as np
import pytest
import torch

from dsgan_hip import spectral as SN

pytestmark = pytest.mark.gpu

# R = 1; nothing divides anything; the stem; C = 640; the size at which the elementwise phases split into chunks
SHAPES = [(1, 8, 4, 4), (3, 5, 1, 1), (32, 6, 4, 4), (96, 40, 4, 4), (256, 128, 4, 4)]
MARGIN = 8.0


def _inputs(i, shape):
    g = torch.Generator().manual_seed(900 + i)
    W = 0.02 * torch.randn(shape, generator=g, dtype=torch.float32)   # init_weights' N(0, 0.02)
    G = torch.randn(shape, generator=g, dtype=torch.float32)
    return W, SN.initial_u(i, shape[0]), G


def _dev(quantities64, quantities32):
    """Per quantity: sigma relative, u / v absolute (unit vectors), W_sn and dW relative to their max."""
    w64, u64, v64, s64, d64 = quantities64
    w32, u32, v32, s32, d32 = quantities32
    return {"sigma": abs(float(s32) - float(s64)) / abs(float(s64)),
            "u": np.abs(u32 - u64).max(), "v": np.abs(v32 - v64).max(),
            "W_sn": np.abs(w32 - w64).max() / np.abs(w64).max(),
            "dW": np.abs(d32 - d64).max() / np.abs(d64).max()}


@pytest.fixture(scope="module")
def cases():
    """Inputs, the float64 reference and the float32 reference's deviation from it, computed once."""
    out = []
    for i, shape in enumerate(SHAPES):
        W, u0, G = _inputs(i, shape)
        ref = {}
        for dt in (np.float64, np.float32):
            w, u, v, s = SN.refresh(W.numpy().astype(dt), u0.numpy().astype(dt))
            d = SN.backward(G.numpy().astype(dt), w, u, v, s)
            ref[dt] = (w.astype(np.float64), u.astype(np.float64), v.astype(np.float64), float(s), d.astype(np.float64))
        out.append(dict(shape=shape, W=W, u0=u0, G=G, ref=ref[np.float64], cpu32=_dev(ref[np.float64], ref[np.float32])))
    return out


@pytest.fixture(scope="module")
def bars(cases):
    worst = {k: max(c["cpu32"][k] for c in cases) for k in cases[0]["cpu32"]}
    print("\nnumpy fp32 vs float64 over the shapes (the bars are %gx these): %s"
          % (MARGIN, ", ".join("%s %.2e" % kv for kv in worst.items())))
    return {k: MARGIN * v for k, v in worst.items()}


def _layer(c):
    """Fresh device tensors of one case: (W, W_sn, u, v, G scratch, dW)."""
    W = c["W"].cuda()
    R, C = W.shape[0], W[0].numel()
    return (W, torch.full_like(W, float("nan")), c["u0"].cuda(), torch.zeros(C, device="cuda"),
            c["G"].cuda(), torch.zeros_like(W))


def _run(cs):
    """One table over the cases ``cs``: refresh (iterating), then the backward.  Everything it left, on the CPU."""
    import dsgan_hip
    from dsgan_hip import functional as HF
    dsgan_hip.require_gpu()
    layers = [_layer(c) for c in cs]
    tab = HF.SpectralTable(layers)
    tab.refresh(iterate=True)
    tab.backward()
    torch.cuda.synchronize()
    return tab, layers, [dict(W_sn=l[1].cpu(), u=l[2].cpu(), v=l[3].cpu(), sigma=tab.sigma[i].cpu(), G=l[4].cpu(), dW=l[5].cpu())
                         for i, l in enumerate(layers)]


@pytest.fixture(scope="module")
def single(cases):
    return [_run([c])[2][0] for c in cases]


@pytest.fixture(scope="module")
def batched(cases):
    return _run(cases)


@pytest.mark.parametrize("i", range(len(SHAPES)), ids=["x".join(map(str, s)) for s in SHAPES])
def test_single_layer_against_float64(i, cases, single, bars):
    c, got = cases[i], single[i]
    w64, u64, v64, s64, d64 = c["ref"]
    got64 = (got["W_sn"].double().numpy(), got["u"].double().numpy(), got["v"].double().numpy(), float(got["sigma"]),
             got["dW"].double().numpy())
    assert all(np.isfinite(x).all() for x in got64)
    dev = _dev(c["ref"], got64)
    print("\n%s: kernel vs float64 %s | numpy fp32 vs float64 %s" % (
        c["shape"], ", ".join("%s %.2e" % kv for kv in dev.items()), ", ".join("%s %.2e" % kv for kv in c["cpu32"].items())))
    for k, e in dev.items():
        assert e <= bars[k], (c["shape"], k, e, bars[k])
    assert not got["G"].any()   # the scratch is left zeroed


def test_batched_equals_single_bit_for_bit(single, batched):
    for one, many in zip(single, batched[2]):
        for k in one:
            assert torch.equal(one[k], many[k]), k


def test_two_runs_are_equal(cases, batched):
    again = _run(cases)[2]
    for a, b in zip(batched[2], again):
        for k in a:
            assert torch.equal(a[k], b[k]), k


def test_recompute_reproduces_sigma_and_w_sn(cases):
    tab, layers, first = _run(cases)
    for l in layers:
        l[1].fill_(float("nan"))
    tab.sigma.fill_(float("nan"))
    tab.refresh(iterate=False)
    torch.cuda.synchronize()
    for i, (l, f) in enumerate(zip(layers, first)):
        assert torch.equal(l[2].cpu(), f["u"]) and torch.equal(l[3].cpu(), f["v"])   # (u, v) kept
        assert torch.equal(tab.sigma[i].cpu(), f["sigma"]), i
        assert torch.equal(l[1].cpu(), f["W_sn"]), i
    # a second iteration moves u and v on (sigma can only grow towards the top singular value)
    tab.refresh(iterate=True)
    torch.cuda.synchronize()
    assert not torch.equal(layers[3][2].cpu(), first[3]["u"])
    assert float(tab.sigma[3]) >= float(first[3]["sigma"]) * (1 - 1e-6)


def test_backward_accumulates_and_zeroes(cases):
    tab, layers, first = _run(cases)
    for l, c in zip(layers, cases):
        assert not l[4].any()
        l[4].copy_(c["G"])   # refill the scratch
    tab.backward()
    torch.cuda.synchronize()
    for l, f in zip(layers, first):
        assert not l[4].any()
        assert torch.equal(l[5].cpu(), 2 * f["dW"])


def test_bad_tables_are_refused():
    import dsgan_hip
    from dsgan_hip import functional as HF
    from dsgan_hip import _lib
    dsgan_hip.require_gpu()
    W = torch.zeros(4, 3, 1, 1, device="cuda")
    with pytest.raises(ValueError, match="v must be a dense fp32 tensor of 3 elements"):
        HF.SpectralTable([(W, W.clone(), torch.zeros(4, device="cuda"), torch.zeros(4, device="cuda"), None, None)])
    tab = HF.SpectralTable([(W, W.clone(), torch.zeros(4, device="cuda"), torch.zeros(3, device="cuda"), None, None)])
    with pytest.raises(RuntimeError, match="without G / dW"):
        tab.backward()
    with pytest.raises(RuntimeError, match="bad args"):
        _lib.call("dsgan_sn_refresh", None, 1, 4, 3, 1, _lib.stream())
    with pytest.raises(RuntimeError, match="bad args"):
        _lib.call("dsgan_sn_backward", _lib.ptr(tab.desc), 0, 4, 3, _lib.stream())
