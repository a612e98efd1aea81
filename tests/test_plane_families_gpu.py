"""The plane-wise kernels per launch form, against fp64, inside guard bands (tests/plane_cases.py: the
case tables, the bundles, the judges).

InstanceNorm: each test is one case x bundle.  It asserts the launch form the plan query names for
the forward and the backward (the case's own, or the scalar kernels under shifted views), runs the
forward and the backward through the C ABI on views whose surroundings hold NaN (inputs) or a fixed
bit pattern (outputs, the per-plane vectors and the scratch included), then checks the moats bit for
bit and every output elementwise against fp64 within the derived bound of plane_cases.in_bounds_*.

Depthwise: each test is one case x bundle x judge through HF.dwconv_raw, HF._dw_wgrad and the two
four-quarter entry points, with the tile configuration (and for the weight-grads the split and the
prefetch form) asserted from dsgan_dwconv_plan; "int" is bitwise against fp64 on integer operands,
"rnd" elementwise within n * 2^-23 * A.

Recorded on an MI355X: 838 tests, 9.4 s for the module; slowest 0.93 s (the depthwise weight-grad at
(16, 512, 8, 128): its fp64 reference walks 49 taps of 8M products), every InstanceNorm test under
0.2 s.

The largest observed ratio to the bound per entry points ("one" dsgan_instnorm_fwd / _bwd, "ws" the
_ws pair, "h16" dsgan_instnorm_fwd_bf16 / _bwd_h), pass, form, rung and precision, over every output
the launch writes (y, mean, rstd, dx, dres, dscale, dxsum).  Two kinds of output end in a single
rounding that is judged against that rounding's own half ulp, so their ratio approaches 1 by
construction; they are listed apart, in brackets: "r16", the 16-bit yh / dxh (round-to-nearest of a
value just above a power of two is U16 |y| / (1 + U16) off), and "mul", dres = dy * slope under
LeakyReLU (one fp32 product against u |g|; 0 under ReLU, where the product is exact).  No other ratio
is above 0.24.

    h16  bwd v4     wave    bf16 0.1863 (r16 0.9855)  fp16 0.2029 (r16 0.9648)
    h16  bwd v4     256x4   bf16 0.2339 (r16 0.9908)  fp16 0.2102 (r16 0.9667)
    h16  bwd v4     256x16  bf16 0.1910 (r16 0.9938)  fp16 0.1969 (r16 0.9814)
    h16  bwd v4     1024    bf16 0.1149 (r16 0.9917)  fp16 0.1118 (r16 0.9736)
    h16  bwd v4     stream  bf16 0.1186 (r16 0.9917)  fp16 0.1068 (r16 0.9721)
    h16  fwd v4     wave    bf16 0.1547 (r16 0.9879)  fp16 0.1387 (r16 0.9682)
    h16  fwd v4     256x4   bf16 0.1571 (r16 0.9928)  fp16 0.1501 (r16 0.9785)
    h16  fwd v4     256x16  bf16 0.1420 (r16 0.9931)  fp16 0.1494 (r16 0.9796)
    h16  fwd v4     1024    bf16 0.0959 (r16 0.9926)  fp16 0.1058 (r16 0.9766)
    h16  fwd v4     stream  bf16 0.0989 (r16 0.9924)  fp16 0.0977 (r16 0.9775)
    one  bwd scalar wave    fp32 0.1299 (mul 0.9493)
    one  bwd scalar 256x4   fp32 0.1595 (mul 0.9500)
    one  bwd scalar 1024    fp32 0.1428 (mul 0.9500)
    one  bwd scalar stream  fp32 0.1268 (mul 0.9500)
    one  bwd v4     wave    fp32 0.1349
    one  bwd v4     256x4   fp32 0.1513 (mul 0.0000)
    one  bwd v4     256x16  fp32 0.1581
    one  bwd v4     1024    fp32 0.1294
    one  bwd v4     stream  fp32 0.0727
    one  fwd scalar wave    fp32 0.1872
    one  fwd scalar 256x4   fp32 0.1476
    one  fwd scalar 1024    fp32 0.1641
    one  fwd scalar stream  fp32 0.1381
    one  fwd v4     wave    fp32 0.1823
    one  fwd v4     256x4   fp32 0.1604
    one  fwd v4     256x16  fp32 0.1538
    one  fwd v4     1024    fp32 0.1276
    one  fwd v4     stream  fp32 0.0846
    ws   bwd split  S       fp32 0.1267
    ws   bwd v4     256x16  fp32 0.0393
    ws   fwd split  S       fp32 0.1605
    ws   fwd v4     256x16  fp32 0.0365

Depthwise, judge "rnd" (the integer judge is exact), per op, tile configuration and prefetch form:

    fwd    cfg 0 0.1765   cfg 1 0.1996   cfg 2 0.1737   cfg 3 0.1384
    mfwd                  cfg 1 0.1802   cfg 2 0.1359   cfg 3 0.1331
    wgrad  cfg 0 0.0447   cfg 1 0.0001   cfg 2 0.0002   cfg 3 0.0004   cfg 3 prefetch 0.0000
    mwgrad                cfg 1 0.0001   cfg 2 0.0002   cfg 3 0.0006
"""
import pytest

import plane_cases as PC

pytestmark = pytest.mark.gpu

DEV = "cuda"
IN_PROBLEMS = PC.in_problems()
DW_PROBLEMS = PC.dw_problems()
IN_RATIOS, DW_RATIOS = {}, {}


@pytest.fixture(scope="module", autouse=True)
def _lib():
    import dsgan_hip
    dsgan_hip.require_gpu()
    yield
    dsgan_hip.set_precision("fp32")


def _faulted(e):
    return any(s in str(e) for s in ("illegal memory access", "HIP error", "hipError"))


@pytest.mark.parametrize("case,bundle", [p[1:] for p in IN_PROBLEMS], ids=[p[0] for p in IN_PROBLEMS])
def test_instnorm_form(case, bundle):
    import torch
    from dsgan_hip import _lib as L
    from dsgan_hip import functional as HF
    HF.set_precision(case.prec)        # the library's half type follows it (fwd_bf16 / bwd_h)
    lib = L.load()
    P = PC.INProblem(case, bundle, DEV, lib)
    plans = PC.in_expect_plan(lib, P)
    try:
        PC.in_launch_fwd(L, P)
        torch.cuda.synchronize()
        PC.in_check(P, fwd_only=True)      # (sets the relu / lrelu mask the backward's reference takes)
        PC.in_launch_bwd(L, P)
        torch.cuda.synchronize()
        ratios = PC.in_check(P)
    except RuntimeError as e:
        if _faulted(e):
            # a faulted device answers every later call with the same error: end the run here
            pytest.exit("GPU fault in %s: %s" % (P.tag(), e), returncode=3)
        raise
    finally:
        HF.set_precision("fp32")
    for what, r in ratios.items():
        bwd = what in ("dx", "dxh", "dres", "dscale", "dxsum")
        p = plans[int(bwd)]
        # an output whose last operation is one rounding judged against that rounding's own half ulp
        # (the 16-bit conversions; dres = dy * slope) is recorded apart from the accumulated ones
        cls = "r16" if what in ("yh", "dxh") else "mul" if what == "dres" and bundle["act"] in ("relu", "lrelu") else "acc"
        key = (case.entry, "bwd" if bwd else "fwd", p.form, p.rung or "S", case.prec, cls)
        if r >= IN_RATIOS.get(key, (-1.0, "", ""))[0]:
            IN_RATIOS[key] = (r, what, bundle["name"])


@pytest.mark.parametrize("case,bundle,judge", [p[1:] for p in DW_PROBLEMS], ids=[p[0] for p in DW_PROBLEMS])
def test_dwconv_form(case, bundle, judge):
    from dsgan_hip import functional as HF
    P = PC.DWProblem(case, bundle, judge, DEV)
    p = PC.dw_expect_plan(HF._lib.load(), P)
    try:
        PC.dw_launch(HF, P)
        r = PC.dw_check(P)
    except RuntimeError as e:
        if _faulted(e):
            pytest.exit("GPU fault in %s: %s" % (P.tag(), e), returncode=3)
        raise
    if judge == "rnd":
        key = (case.op, p.cfg, p.prefetch)
        if r >= DW_RATIOS.get(key, (-1.0, ""))[0]:
            DW_RATIOS[key] = (r, bundle["name"])


def test_report_largest_ratios():
    """The largest observed ratio to the bound per entry point, pass, form, rung and precision,
    printed for the record (each one was asserted <= 1 where it was measured)."""
    for key in sorted(IN_RATIOS, key=str):
        r, what, where = IN_RATIOS[key]
        print("ratio in  %-4s %-3s %-6s %-6s %-4s %-3s %.4f  (%s, %s)" % (key + (r, what, where)))
    for key in sorted(DW_RATIOS, key=str):
        r, where = DW_RATIOS[key]
        print("ratio dw  %-6s cfg %d pf %d  %.4f  (%s)" % (key + (r, where)))
    assert all(v[0] <= 1.0 for v in IN_RATIOS.values()) and all(v[0] <= 1.0 for v in DW_RATIOS.values())
