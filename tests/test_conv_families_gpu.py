"""Every conv kernel family against the fp64 reference, elementwise and on exact integers, inside
guard bands (tests/conv_cases.py: the case table, the option bundles, the two judges).

Each test is one case x bundle x judge: it asserts the family the chooser names (the case's own,
or under shifted views whatever the chooser falls back to), launches conv_{fwd,dgrad,wgrad}_raw on
views whose surroundings hold NaN (inputs) or a fixed bit pattern (outputs), asserts the family the
launch recorded, and then checks the moats bit for bit and the result with its judge.

Recorded on an MI355X (1344 tests, 6.2 s for the module; slowest 0.69 s, the first test, which
loads the library): the largest ratio to the judge-2 bound per (op, family.form) and precision,
counted under the family the launch took (so igemm / small_in / small_out include the fallbacks of
the shifted-view bundles).  Every ratio above 0.1 belongs to a reduction of n <= 30 terms, where a
single rounding is a visible share of an n-ulp bound, except two: pwgemm.gemm's bf16 data-grad
(0.106, the gact=gelu bundle: the fp32 evaluation of gelu' against the 2^-21 the bound grants it),
and pw_small's forward with xact=gelu in the 16-bit modes: that kernel keeps the activated operand
in fp32, the reference rounds it to the 16-bit type, and the difference uses up to half of the
2 u A the bound grants for that rounding.

    dgrad  igemm         fp32 0.1296  bf16 0.0956  fp16 0.1097
    dgrad  pconv                      bf16 0.0420  fp16 0.0877
    dgrad  pconvt                     bf16 0.0496  fp16 0.0783
    dgrad  pglast        fp32 0.0848  bf16 0.0379  fp16 0.0983
    dgrad  pw_small      fp32 0.1583  bf16 0.0866  fp16 0.1252
    dgrad  pwf32         fp32 0.0876
    dgrad  pwgemm.gemm                bf16 0.1063  fp16 0.0949
    dgrad  pwgemm.io_ws               bf16 0.0094  fp16 0.0141
    dgrad  small_in      fp32 0.0994  bf16 0.0568  fp16 0.1124
    dgrad  small_out     fp32 0.0549  bf16 0.0270  fp16 0.0609
    dgrad  tconv                      bf16 0.0719  fp16 0.0319
    dgrad  thin3         fp32 0.1575  bf16 0.0798  fp16 0.1667
    fwd    igemm         fp32 0.0571  bf16 0.0196  fp16 0.0231
    fwd    pconv                      bf16 0.0023  fp16 0.0026
    fwd    pglast        fp32 0.0014  bf16 0.0008  fp16 0.0011
    fwd    pw_small      fp32 0.1468  bf16 0.4276  fp16 0.3927
    fwd    pwf32         fp32 0.0457
    fwd    pwgemm.gemm                bf16 0.0221  fp16 0.0305
    fwd    pwgemm.io_ws               bf16 0.0231  fp16 0.0208
    fwd    small_in      fp32 0.1215  bf16 0.0723  fp16 0.1192
    fwd    small_out     fp32 0.0291  bf16 0.0116  fp16 0.0254
    fwd    tconv                      bf16 0.0023  fp16 0.0025
    fwd    thin3         fp32 0.0160  bf16 0.0137  fp16 0.0219
    wgrad  igemm         fp32 0.0428  bf16 0.0162  fp16 0.0189
    wgrad  pglast        fp32 0.0054  bf16 0.0039  fp16 0.0052
    wgrad  pwf32         fp32 0.0060
    wgrad  pwgemm.gemm                bf16 0.0015  fp16 0.0019
    wgrad  thin3         fp32 0.0002  bf16 0.0001  fp16 0.0001
    wgrad  wconv.db                   bf16 0.0141  fp16 0.0177
    wgrad  wconv.plain                bf16 0.0163  fp16 0.0156
    wgrad  wgrad_small   fp32 0.0181  bf16 0.0169  fp16 0.0174
"""
import pytest

import conv_cases as CC

pytestmark = pytest.mark.gpu

DEV = "cuda"
PROBLEMS = CC.problems()
RATIOS = {}


@pytest.fixture(scope="module", autouse=True)
def _lib():
    import dsgan_hip
    dsgan_hip.require_gpu()
    yield
    dsgan_hip.set_precision("fp32")


@pytest.mark.parametrize("case,bundle,judge", [p[1:] for p in PROBLEMS], ids=[p[0] for p in PROBLEMS])
def test_conv_family(case, bundle, judge):
    from dsgan_hip import functional as HF
    with CC.state(HF, case, True):
        P = CC.Problem(case, bundle, judge, DEV)
        CC.expect_family(HF, P)
        try:
            CC.launch(HF, P)
            r = CC.check(P)
        except RuntimeError as e:
            if any(s in str(e) for s in ("illegal memory access", "HIP error", "hipError")):
                # a faulted device answers every later call with the same error: end the run here
                pytest.exit("GPU fault in %s: %s" % (CC.case_id(case), e), returncode=3)
            raise
    if judge == "rnd":
        key = (case.op,) + P.fam + (case.prec,)
        if r > RATIOS.get(key, (0.0, ""))[0] or key not in RATIOS:
            RATIOS[key] = (r, CC.bundle_id(bundle))


def test_report_largest_ratios():
    """The largest observed ratio to the judge-2 bound per (op, family, form, precision), printed for
    the record (each one was asserted <= 1 where it was measured)."""
    for key in sorted(RATIOS, key=str):
        r, where = RATIOS[key]
        print("ratio %-6s %-20s %-6s %-5s %.4f  (%s)" % (key[0], key[1], key[2] or "-", key[3], r, where))
    assert all(r <= 1.0 for r, _ in RATIOS.values())
