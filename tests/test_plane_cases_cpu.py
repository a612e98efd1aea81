"""The tests of tests/plane_cases.py, without a GPU: the tables reach every launch form the two plan
queries can name, the judges pass a correct result and reject each injected defect.

torch's CPU fp32 ops stand in for the kernels (plane_cases.in_standin / dw_standin): they write into
the same guarded views, and the same in_check() / dw_check() judge them.
"""
import itertools
import os

import pytest
import torch

import plane_cases as PC

IN_IDS = [PC.in_case_id(c) for c in PC.IN_CASES]
RATIOS = {}


@pytest.fixture(scope="module")
def lib():
    from dsgan_hip import _lib
    if not os.path.exists(_lib.LIB_PATH):
        pytest.skip("libdsgan_hip.so not built (run __graft_entry__.build())")
    return _lib.load()


def _in_problem(lib, c, b):
    P = PC.INProblem(c, b, "cpu", lib)
    PC.in_expect_plan(lib, P)
    return P


def _bundle(c, name):
    return next(b for b in PC.in_bundles(c) if b["name"] == name)


def _case(entry, HW, prec="fp32", planes=None):
    return next(c for c in PC.IN_CASES if (c.entry, c.HW, c.prec) == (entry, HW, prec)
                and (planes is None or c.N * c.C == planes))


def _rejected(fn, *a):
    with pytest.raises(AssertionError) as e:
        fn(*a)
    return str(e.value)


# ------------------------------------------------------------------------------------------
# the tables
# ------------------------------------------------------------------------------------------
def test_ids_are_unique_and_tensors_small():
    for ids in ([p[0] for p in PC.in_problems()], [p[0] for p in PC.dw_problems()]):
        assert len(set(ids)) == len(ids)
    assert all(c.N * c.C * c.HW <= 2 ** 21 for c in PC.IN_CASES)
    assert all(c.N * c.C * (4 if c.op[0] == "m" else 1) * c.H * c.W <= 2 ** 23 for c in PC.DW_CASES)
    assert all((c.N * c.C) % 4 for c in PC.IN_CASES if c.entry != "ws")    # the wave form's early exit is taken


def test_in_table_covers_every_plan_code(lib):
    """Every (form, rung, full, backward) dsgan_instnorm_plan returns over plane sizes on and beside
    every ladder edge, aligned or not, with and without scratch, is the expected plan of a case."""
    assert len(PC.LEFT_OUT) <= 3
    sizes = set(range(1, 4200)) | set(range(16300, 16500)) | set(range(65400, 66700)) | {98308}
    can = set()
    for HW, al, bwd, ws, (N, C) in itertools.product(sorted(sizes), (0, 1), (0, 1), (0, 1), ((2, 3), (1, 127), (2, 64))):
        p = PC.in_plan(lib, N, C, HW, al, bwd, ws)
        can.add((p.form, p.rung, p.full, bwd))
    seen = set()
    for c in PC.IN_CASES:
        for bwd in (0, 1):
            seen.add((c.form, c.rung, bool(c.full and not bwd), bwd))
            if any(b["misalign"] for b in PC.in_bundles(c)):
                seen.add(("scalar", PC.in_plan(lib, c.N, c.C, c.HW, 0, bwd, 0).rung, False, bwd))
    assert can - seen - set(PC.LEFT_OUT) == set(), sorted(can - seen, key=str)
    assert seen <= can
    # the split forms' S: 4 chunks, a last chunk of one float4, and many
    assert {c.S for c in PC.IN_CASES if c.form == "split"} == {4, 5, 17}
    assert PC.in_plan(lib, 2, 3, 16388, 1, 0, 1).S == 5 and (16388 // 4) % 1024 == 1


def test_dw_table_covers_every_plan_code(lib):
    can = set()
    for op, multi, al, K, H, W, (N, C) in itertools.product(
            (0, 1), (0, 1), (0, 1), PC.KS, (4, 8, 40, 70), (4, 32, 36, 64, 65, 128, 256),
            ((2, 3), (16, 512), (17, 512), (5, 512), (16, 128), (2, 1024))):
        p = PC.dw_plan(lib, N, C, H, W, K, al, op, multi)
        if not (multi and p.cfg == 0):          # the four-quarter entry points refuse these
            can.add((op, multi, p.cfg, p.prefetch))
    seen = set()
    for c in PC.DW_CASES:
        wg, multi = int(c.op in ("wgrad", "mwgrad")), int(c.op[0] == "m")
        seen.add((wg, multi, c.cfg, int(c.pf)))
        if any(b["misalign"] for b in PC.dw_bundles(c)):
            seen.add((wg, multi, 0, 0))
    assert can - seen == set(), sorted(can - seen)
    assert seen <= can


# ------------------------------------------------------------------------------------------
# InstanceNorm: the judge judges
# ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", PC.IN_CASES, ids=IN_IDS)
def test_in_standin_passes(lib, case):
    """torch's fp32 two-pass InstanceNorm stays within the derived bound in every bundle, guards
    intact; for relu / lrelu its own mask stays inside the cap (the seeds' condition)."""
    for b in PC.in_bundles(case):
        P = _in_problem(lib, case, b)
        PC.in_standin(P)
        for k, r in PC.in_check(P).items():
            key = (case.entry, case.rung or "split", k)
            RATIOS[key] = max(RATIOS.get(key, 0.0), r)
            print("%-8s %-8s %.4f" % (b["name"], k, r))


FWD_MUTANTS = [
    # (mutant, case, bundle, the output that must fail)
    ("onepass", ("one", 4096), "offset", "rstd"),
    ("onepass", ("one", 65540), "offset", "rstd"),
    ("drop4", ("one", 1020), "plain", "mean"),
    ("drop4", ("one", 65540), "plain", "mean"),
    ("drop4", ("one", 65540), "spike", "mean"),
    ("noscale", ("one", 4092), "allon", "mean"),
    ("sample0", ("one", 4092), "plain", "mean"),
    ("res_first", ("one", 4092), "fast", "mean"),
]


@pytest.mark.parametrize("mut,key,bundle,what", FWD_MUTANTS, ids=lambda v: str(v))
def test_in_forward_defect_is_rejected(lib, mut, key, bundle, what):
    c = _case(*key)
    P = _in_problem(lib, c, _bundle(c, bundle))
    PC.in_standin(P, mut_fwd=mut)
    msg = _rejected(PC.in_check, P, True)
    assert "[%s]" % what in msg and "outside the bound" in msg


def test_in_sym_mean_must_be_zero_bit_for_bit(lib):
    c = _case("one", 4092)
    P = _in_problem(lib, c, _bundle(c, "sym"))
    PC.in_standin(P)
    assert bool((P.v("mean") == 0).all())
    P.v("mean")[2] = 2.0 ** -40      # inside the bound, but not the exact sum
    assert "sums to exactly 0" in _rejected(PC.in_check, P, True)


BWD_MUTANTS = [
    ("drop4", ("one", 1020), "spike", "dx"),
    ("drop4", ("one", 65540), "spike", "dx"),
    ("drop4", ("one", 65540), "allon", "dx"),
    ("noscale", ("one", 4092), "allon", "dx"),
    ("sample0", ("one", 4092), "plain", "dx"),
]


@pytest.mark.parametrize("mut,key,bundle,what", BWD_MUTANTS, ids=lambda v: str(v))
def test_in_backward_defect_is_rejected(lib, mut, key, bundle, what):
    """The forward is right (and passes), the backward alone carries the defect."""
    c = _case(*key)
    P = _in_problem(lib, c, _bundle(c, bundle))
    PC.in_standin(P, mut_bwd=mut)
    PC.in_check(P, True)
    msg = _rejected(PC.in_check, P)
    assert "[%s]" % what in msg and "outside the bound" in msg


def test_in_16bit_and_small_outputs_are_judged(lib):
    c = _case("h16", 4092, "bf16")
    for name, what in (("yh", "yh"), ("dxh", "dxh"), ("dxsum", "dxsum"), ("dres", "dres")):
        P = _in_problem(lib, c, _bundle(c, "allon"))
        PC.in_standin(P)
        v = P.v(name)
        at = (0,) * (v.dim() - 1) + (5,)
        v[at] = 3.0 if v.dtype != torch.float32 else v[at] + 1.0
        assert "[%s]" % what in _rejected(PC.in_check, P)
    c = _case("one", 4092)
    P = _in_problem(lib, c, _bundle(c, "lrelu"))
    PC.in_standin(P)
    P.v("dscale")[4] *= 1.01
    assert "[dscale]" in _rejected(PC.in_check, P)
    P = _in_problem(lib, c, _bundle(c, "sym"))      # act none: dres is dy bit for bit
    PC.in_standin(P)
    P.v("dres")[0, 0, 0, 7] *= 1.0 + 2.0 ** -23
    assert "dres differs from dy" in _rejected(PC.in_check, P)


def test_in_closed_form_dscale_is_the_definition():
    """dscale's reference is the kernels' closed form evaluated in fp64; it equals the sum by the
    definition (sum over the plane of dL/d(scale x) * x) up to that sum's own cancellation error."""
    for key, bname in ((("one", 4092), "allon"), (("one", 1023), "lrelu"), (("one", 16388), "offset")):
        c = _case(*key)
        b = _bundle(c, bname)
        d = PC.in_data(c, b)
        R = PC.in_fwd(d, b["act"], torch.float64)
        closed = PC.in_bwd(d, b["act"], torch.float64, R["mu"], R["r"])
        direct = PC.in_bwd(d, b["act"], torch.float64, R["mu"], R["r"], direct_dscale=True)
        terms = (R["r"] * closed["t"] * d["x"]).abs().sum(-1)
        assert bool(((closed["dscale"] - direct["dscale"]).abs() <= 2.0 ** -50 * c.HW * terms).all())
        assert bool((closed["dscale"].abs() > 0).all())


def test_in_moat_and_input_writes_are_caught(lib):
    for c, bname in ((_case("one", 4092), "allon"), (_case("h16", 1020, "fp16"), "allon"), (_case("ws", 16388), "plain")):
        b = _bundle(c, bname)
        names = list(_in_problem(lib, c, b).slots)
        for name in names:
            P = _in_problem(lib, c, b)
            PC.in_standin(P)
            sl = P.slots[name]
            inside = (~sl.moat_mask).nonzero().reshape(-1)
            gaps = (inside[1:] - inside[:-1] > 1).nonzero().reshape(-1)
            at = int(inside[gaps[0]] if len(gaps) else inside[-1]) + 1
            assert sl.moat_mask[at]
            sl.buf[at] = 1.0
            msg = _rejected(PC.in_check, P)
            assert ("of an input written" if sl.kind == "in" else "of the moat written") in msg and "'%s'" % name in msg


def test_in_nan_from_a_moat_is_caught(lib):
    c = _case("one", 16388)
    P = _in_problem(lib, c, _bundle(c, "plain"))
    PC.in_standin(P)
    assert torch.isnan(P.slots["x"].buf[0])
    P.v("dx").view(-1)[-1] += P.slots["x"].buf[0] * 0.0
    assert "non-finite output" in _rejected(PC.in_check, P)


# ------------------------------------------------------------------------------------------
# depthwise: the judges judge
# ------------------------------------------------------------------------------------------
def _dw_problem(lib, c, b, judge):
    P = PC.DWProblem(c, b, judge)
    PC.dw_expect_plan(lib, P)
    return P


SMALL_DW = [c for c in PC.DW_CASES if not c.big]


@pytest.mark.parametrize("case", PC.DW_CASES, ids=PC.dw_case_id)
def test_dw_standin_passes_both_judges(lib, case):
    if case.big and case.N * case.C * case.H * case.W > 2 ** 21:
        # (the long references run once, on the GPU; the plan is still asserted here)
        _dw_problem(lib, case, PC.dw_bundles(case)[0], "int")
        return
    for b in PC.dw_bundles(case):
        for j in PC.dw_judges(case, b):
            P = _dw_problem(lib, case, b, j)
            PC.dw_standin(P)
            r = PC.dw_check(P)
            RATIOS[(case.op, case.cfg)] = max(RATIOS.get((case.op, case.cfg), 0.0), r)
    print("largest ratio to n*2^-23*A: %.4f" % RATIOS[(case.op, case.cfg)])


def _dw_bundle(c, name):
    return next(b for b in PC.dw_bundles(c) if b["name"] == name)


@pytest.mark.parametrize("case", [c for c in SMALL_DW if c.op in ("fwd", "mfwd")], ids=PC.dw_case_id)
def test_dw_forward_defects_are_rejected(lib, case):
    for mut, bname in (("noflip", "flip"), ("clamp", "bias"), ("bias_twice", "bias+acc")):
        for j in ("int", "rnd"):
            P = _dw_problem(lib, case, _dw_bundle(case, bname), j)
            PC.dw_standin(P, mut=mut)
            msg = _rejected(PC.dw_check, P)
            assert ("differ on integer data" if j == "int" else "outside n*2^-23*A") in msg, (mut, j)


@pytest.mark.parametrize("case", [c for c in SMALL_DW if c.K in (0, 7)], ids=PC.dw_case_id)
def test_dw_moat_and_input_writes_are_caught(lib, case):
    b = PC.dw_bundles(case)[1]
    for name in list(_dw_problem(lib, case, b, "int").slots):
        P = _dw_problem(lib, case, b, "int")
        PC.dw_standin(P)
        sl = P.slots[name]
        inside = (~sl.moat_mask).nonzero().reshape(-1)
        gaps = (inside[1:] - inside[:-1] > 1).nonzero().reshape(-1)
        at = int(inside[gaps[0]] if len(gaps) else inside[-1]) + 1
        assert sl.moat_mask[at]
        sl.buf[at] = 1.0
        assert ("of an input written" if sl.kind == "in" else "of the moat written") in _rejected(PC.dw_check, P)


@pytest.mark.parametrize("case", [c for c in SMALL_DW if c.op in ("wgrad", "mwgrad") and c.K in (0, 7)],
                         ids=PC.dw_case_id)
def test_dw_weight_grad_one_image_short_is_rejected(lib, case):
    """A weight-grad that leaves the last image's last row out of one tap."""
    # (n * 2^-23 * A grows with the n = N H W summed terms: past ~1000 it no longer sees one row, which
    # is what the integer judge is for)
    for j in ("int", "rnd") if case.N * case.H * case.W <= 1024 else ("int",):
        P = _dw_problem(lib, case, PC.dw_bundles(case)[0], j)
        PC.dw_standin(P)
        d = P.cpu
        o, q, K = P.quarters[-1]
        p = K // 2
        # tap (p, p) pairs dy[h, w] with x[h, w]
        t = (d["dy"][-1, o:o + q, -1, :] * d["x"][-1, o:o + q, -1, :]).sum(-1)
        assert bool((t != 0).any())
        P.v("dw%d" % (len(P.quarters) - 1))[:, 0, p, p] -= t.float()
        msg = _rejected(PC.dw_check, P)
        assert ("differ on integer data" if j == "int" else "outside n*2^-23*A") in msg
