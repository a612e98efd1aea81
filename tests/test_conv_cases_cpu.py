"""The tests of tests/conv_cases.py, without a GPU: the case table reaches what training calls, the
judges pass a correct result and reject each of five injected defects.

torch's CPU fp32 conv / conv-grad / einsum of the same operands stands in for the kernel
(conv_cases.standin): it writes into the same guarded views, and the same check() judges it.
"""
import inspect
import itertools
import os
import re

import pytest
import torch

import conv_cases as CC
from test_dispatch_cpu import FAMILIES

CASE_IDS = [CC.case_id(c) for c in CC.CASES]
RATIOS = {}


@pytest.fixture(scope="module")
def HF():
    from dsgan_hip import _lib
    if not os.path.exists(_lib.LIB_PATH):
        pytest.skip("libdsgan_hip.so not built (run __graft_entry__.build())")
    from dsgan_hip import functional
    return functional


def _problem(HF, case, b, judge):
    P = CC.Problem(case, b, judge)
    CC.expect_family(HF, P)
    return P


def _plain(case):
    return CC.bundles(case)[0]


def _linear(case):
    return CC.bundles(case)[1]


def _rejected(P):
    """check() must raise on P as it stands; returns the message."""
    with pytest.raises(AssertionError) as e:
        CC.check(P)
    return str(e.value)


# ------------------------------------------------------------------------------------------
# the table
# ------------------------------------------------------------------------------------------
def test_case_ids_are_unique_and_shapes_small():
    assert len(set(CASE_IDS)) == len(CASE_IDS)
    ids = [p[0] for p in CC.problems()]
    assert len(set(ids)) == len(ids)
    for c in CC.CASES:
        N, Cin, H, W, Cout, K, s, p = c.shape
        Ho, Wo = (H + 2 * p - K) // s + 1, (W + 2 * p - K) // s + 1
        assert max(N * Cout * Ho * Wo, N * Cin * H * W, Cout * Cin * K * K) <= 10 ** 6, c
        P = CC.Problem(c, _plain(c), "int")
        assert (P.n_terms() <= 600) != c.deep or c.op == "wgrad", (CC.case_id(c), P.n_terms())


@pytest.fixture(scope="module")
def exercised(HF):
    """{(prec, op, family, form, *flags)} the case table exercises, asked of the choosers; every
    bundle that keeps its views aligned must take the case's own family (expect_family asserts it)."""
    seen = set()
    for c in CC.CASES:
        with CC.state(HF, c, False):
            for b in CC.bundles(c):
                P = _problem(HF, c, b, "rnd" if not c.deep else "int")
                if not b["misalign"]:      # a fallback family counts for nothing here
                    seen.add((c.prec, c.op) + P.fam + CC.bundle_flags(b))
    return seen


def test_table_covers_every_recorded_combination(exercised):
    missing = sorted(CC.table_combos() - exercised, key=str)
    assert not missing, "%d combinations of the dispatch table in no case, first: %r" % (len(missing), missing[:5])


def test_table_covers_every_family_where_it_can_occur(HF, exercised):
    choosers = {"fwd": HF.conv_fwd_family, "dgrad": HF.conv_dgrad_family, "wgrad": HF.conv_wgrad_family}
    assert len(CC.LEFT_OUT) <= 5
    in_table = {(r["op"], r["fam"], r["form"]) for r in CC.ROWS}
    assert not {k[:3] for k in CC.LEFT_OUT} & in_table
    for op, fn in choosers.items():
        # the families this op's chooser can return, read from its return statements
        named = set(re.findall(r'return "(\w+_kernel)"', inspect.getsource(fn)))
        can = {(f, form) for f, form in FAMILIES if f in named}
        if op == "wgrad":
            can.discard(("pwgemm_kernel", "io_ws"))    # the weight-grad has the dsgan_pw_gemm form only
        else:
            can -= {("wconv_kernel", "db"), ("wconv_kernel", "plain")}
        assert {k[1:] for k in CC.ADMITS if k[0] == op} | {k[1:3] for k in CC.LEFT_OUT if k[0] == op} == can
        for fam, form in can - {k[1:3] for k in CC.LEFT_OUT if k[0] == op}:
            precs = {e[0] for e in exercised if e[1:4] == (op, fam, form)}
            want = {"fp32"} if fam == "pwf32_kernel" else (
                {"bf16", "fp16"} if fam in ("pwgemm_kernel", "pconv_kernel", "pconvt_kernel", "tconv_kernel",
                                            "wconv_kernel") else {"fp32", "bf16", "fp16"})
            assert precs == want, (op, fam, form, precs)


def test_deep_cases_reach_their_split_paths(HF):
    """The deep-K cases of the families with a workspace-backed split are deep enough to split."""
    lib = HF._lib.load()
    for c in CC.CASES:
        if not c.deep:
            continue
        N, Cin, H, W, Cout, K, s, p = c.shape
        Ho, Wo = (H + 2 * p - K) // s + 1, (W + 2 * p - K) // s + 1
        if c.fam == "pwgemm_kernel" and c.op == "fwd":
            assert lib.dsgan_pw_fd_workspace(0, Cout, Cin, H * W, N) > 0, c
        elif c.fam == "pwgemm_kernel" and c.op == "dgrad":
            assert lib.dsgan_pw_fd_workspace(1, Cin, Cout, H * W, N) > 0, c
        elif c.fam == "pwgemm_kernel" and c.op == "wgrad":
            assert lib.dsgan_pw_wgrad_workspace(Cout, Cin, H * W, N) > 0, c
        elif c.fam == "pwf32_kernel" and c.op == "wgrad":
            assert lib.dsgan_pw_f32_wgrad_workspace(Cout, Cin, H * W, N) > 0, c
        elif c.fam == "wconv_kernel":
            assert lib.dsgan_wconv_workspace(N, Cin, Cout, Ho, Wo, K, K) > K * K * Cout * Cin + Cout, c
        elif c.fam == "igemm_kernel" and c.op == "wgrad":
            assert lib.dsgan_conv_wgrad_workspace(N, Cin, Cout, K, K, Ho, Wo, 0 if c.prec == "fp32" else 1) > 0, c


# ------------------------------------------------------------------------------------------
# the judges judge
# ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", CC.CASES, ids=CASE_IDS)
def test_standin_passes_both_judges(HF, case):
    """torch's fp32 result stays within judge 2 (its ratio recorded) and is exact on integer data,
    in every bundle, with the guards intact."""
    with CC.state(HF, case, False):
        for b in CC.bundles(case):
            for judge in CC.judges(case, b):
                P = _problem(HF, case, b, judge)
                CC.standin(P)
                r = CC.check(P)
                key = (case.op, case.fam, case.form, case.prec)
                RATIOS[key] = max(RATIOS.get(key, 0.0), r)
    if not case.deep:
        print("largest ratio to the judge-2 bound: %.4f" % RATIOS[(case.op, case.fam, case.form, case.prec)])


# ------------------------------------------------------------------------------------------
# injected defects fail
# ------------------------------------------------------------------------------------------
SHALLOW = [c for c in CC.CASES if not c.deep]


@pytest.mark.parametrize("case", [c for c in SHALLOW if c.op != "wgrad" and c.shape[5] > 1],
                         ids=lambda c: CC.case_id(c))
def test_defect_border_column_without_its_outermost_tap(HF, case):
    with CC.state(HF, case, False):
        P = _problem(HF, case, _plain(case), "rnd")
        CC.standin(P)
        short = CC.compute(P, torch.float32, drop_tap_col=True)["out"]
        P.v("out")[..., 0] = short[..., 0]
        msg = _rejected(P)
    assert "outside n*2^-23*A" in msg and "index" in msg


def _twice(P):
    """The constant addend once more on the last row of the last three channels."""
    c, d, out = P.case, P.cpu, P.v("out")
    if c.op == "wgrad":
        out[-3:, :, -1, :] += d["y0"][-3:, :, -1, :].float()
    elif P.b["bias"]:
        out[:, -3:, -1, :] += d["bias"][-3:].float().view(1, -1, 1)
    else:
        out[:, -3:, -1, :] += d["y0"][:, -3:, -1, :].float()


@pytest.mark.parametrize("case", SHALLOW, ids=lambda c: CC.case_id(c))
def test_defect_addend_twice_on_a_ragged_tile_row(HF, case):
    with CC.state(HF, case, False):
        P = _problem(HF, case, _linear(case), "rnd")
        assert P.b["bias"] or P.b["acc"] or case.op == "wgrad"
        CC.standin(P)
        _twice(P)
        msg = _rejected(P)
    assert "outside n*2^-23*A" in msg


def _drop_one_term(P):
    """One product of the reduction taken out of one output element (a non-zero one)."""
    c, d, out = P.case, P.cpu, P.v("out")
    N, Cin, H, W, Cout, K, s, p = c.shape
    # tap (pad, pad) pairs output pixel (oh, ow) with input pixel (oh * s, ow * s)
    for co, ci, oh, ow in itertools.product(range(Cout), range(Cin), range(P.Ho), range(P.Wo)):
        if c.op == "fwd":
            t = d["x"][0, ci, oh * s, ow * s] * d["w"][co, ci, p, p]
            at = (0, co, oh, ow)
        elif c.op == "dgrad":
            t = d["dy"][0, co, oh, ow] * d["w"][co, ci, p, p]
            at = (0, ci, oh * s, ow * s)
        else:
            t = d["dy"][0, co, oh, ow] * d["x"][0, ci, oh * s, ow * s]
            at = (co, ci, p, p)
        if t != 0:
            out[at] -= float(t)
            return
    raise AssertionError("no non-zero term")


@pytest.mark.parametrize("case", CC.CASES, ids=CASE_IDS)
def test_defect_one_k_term_dropped(HF, case):
    with CC.state(HF, case, False):
        for b in (_plain(case), _linear(case)):
            P = _problem(HF, case, b, "int")
            CC.standin(P)
            _drop_one_term(P)
            msg = _rejected(P)
            assert "1 of " in msg and "differ on integer data" in msg


@pytest.mark.parametrize("case", CC.CASES, ids=CASE_IDS)
def test_defect_one_moat_element_overwritten(HF, case):
    with CC.state(HF, case, False):
        for b in (_plain(case), _linear(case)):
            for name in ("out", "db") if b["db"] else ("out",):
                P = _problem(HF, case, b, "int")
                CC.standin(P)
                sl = P.slots[name]
                inside = (~sl.moat_mask).nonzero().reshape(-1)
                # right behind the first contiguous run of the view: between two samples of a slice,
                # behind the tensor otherwise
                gaps = (inside[1:] - inside[:-1] > 1).nonzero().reshape(-1)
                at = int(inside[gaps[0]] if len(gaps) else inside[-1]) + 1
                assert sl.moat_mask[at]
                sl.buf[at] = 1.0
                assert "of the moat written" in _rejected(P)
        # and a launch that writes an input is caught as well
        P = _problem(HF, case, _plain(case), "int")
        CC.standin(P)
        src = P.slots["x" if case.op == "fwd" else "dy"]
        src.buf[0] = 0.0
        assert "of an input written" in _rejected(P)


@pytest.mark.parametrize("case", CC.CASES, ids=CASE_IDS)
def test_defect_nan_moat_element_leaks_into_the_output(HF, case):
    with CC.state(HF, case, False):
        for judge in CC.judges(case, _plain(case)):
            P = _problem(HF, case, _plain(case), judge)
            CC.standin(P)
            src = P.slots["x" if case.op == "fwd" else "dy"]
            leak = src.buf[0]                      # a moat element of an input: NaN
            assert torch.isnan(leak)
            P.v("out").view(-1)[-1] += leak * 0.0  # "times a zero-padded weight"
            assert "non-finite output" in _rejected(P)
