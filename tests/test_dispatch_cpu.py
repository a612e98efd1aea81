"""Which kernel family each conv of the train step takes, asked without a GPU.

functional.conv_{fwd,dgrad,wgrad}_family choose the family (and, for pwgemm_kernel and
wconv_kernel, the launch form) of a conv_*_raw call from plain numbers.  A layer that falls through
to igemm_kernel because a stride or an alignment changed still passes every correctness test; this
one pins the choice.

tests/golden/conv_dispatch_v1.json holds the plain inputs of every distinct conv_*_raw call of two
eager train steps at the benchmark's config (256^2, B=16, bf16) and at 64^2, B=2, fp32, plus
hand-made calls at the smallest shapes that reach the families those steps do not (tconv at stride
1 and 2, the dsgan_pw_gemm form of pwgemm in fwd / dgrad, wconv without a bias grad), each with
the family its launch recorded on IGEMM_TIMER and the entry point it called.  The table was
recorded by tools/call_trace.py on the tree *before* the choosers existed (the launchers' own
if/elif ladders), so the expectations do not come from the code under test.
"""
import inspect
import json
import os

import pytest

TABLE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "conv_dispatch_v1.json")
BASE = 1 << 32   # a 256-byte aligned stand-in address: the choosers read pointers' alignment only

FAMILIES = {("thin3_kernel", None), ("pw_small_kernel", None), ("pglast_kernel", None), ("small_out_kernel", None),
            ("small_in_kernel", None), ("pwgemm_kernel", "io_ws"), ("pwgemm_kernel", "gemm"), ("pwf32_kernel", None),
            ("pconv_kernel", None), ("pconvt_kernel", None), ("tconv_kernel", None), ("wconv_kernel", "db"),
            ("wconv_kernel", "plain"), ("wgrad_small_kernel", None), ("igemm_kernel", None)}


@pytest.fixture(scope="module")
def HF():
    from dsgan_hip import _lib
    if not os.path.exists(_lib.LIB_PATH):
        pytest.skip("libdsgan_hip.so not built (run __graft_entry__.build())")
    from dsgan_hip import functional
    return functional


with open(TABLE) as _f:
    ROWS = json.load(_f)


@pytest.fixture
def state(HF):
    """set(prec, pglast, db_fold): the module state the choice reads, put back afterwards.  The
    precision is set without set_precision(), which also switches the library's half type."""
    old = HF._state["prec"], HF.PGLAST[0], HF.WCONV_DB_FOLD

    def set_(prec, pglast=True, db_fold=True):
        HF._state["prec"], HF.PGLAST[0], HF.WCONV_DB_FOLD = prec, pglast, db_fold
    yield set_
    set_(*old)


def _args(fn, r):
    return {k: (BASE + r[k] if k.endswith("_ptr") and r[k] is not None else r[k])
            for k in inspect.signature(fn).parameters}


def test_table_reaches_every_family_and_form():
    seen = {(r["fam"], r["form"]) for r in ROWS}
    assert seen == FAMILIES
    # tconv's data-grad has a one-launch (stride 1) and a per-parity (stride 2) form
    assert {r["stride"] for r in ROWS if r["fam"] == "tconv_kernel" and r["op"] == "dgrad"} == {1, 2}
    assert len(ROWS) <= 500


def test_every_recorded_call_takes_its_recorded_family(HF, state):
    choosers = {"fwd": HF.conv_fwd_family, "dgrad": HF.conv_dgrad_family, "wgrad": HF.conv_wgrad_family}
    bad = []
    for r in ROWS:
        state(r["prec"], r["pglast"], r["db_fold"])
        fn = choosers[r["op"]]
        got = fn(**_args(fn, r))
        if got != (r["fam"], r["form"]):
            bad.append((got, r))
    assert not bad, "%d of %d rows differ, first: %r" % (len(bad), len(ROWS), bad[0])


def test_toggles_move_the_choice(HF, state):
    """PGLAST[0] and WCONV_DB_FOLD are inputs of the choice: off, the PatchGAN head leaves pglast.hip
    and the 4x4 weight-grad takes the form without the bias grad."""
    head = next(r for r in ROWS if r["fam"] == "pglast_kernel" and r["op"] == "fwd")
    state(head["prec"], pglast=False)
    assert HF.conv_fwd_family(**_args(HF.conv_fwd_family, head))[0] == "small_out_kernel"
    wc = next(r for r in ROWS if r["form"] == "db")
    state(wc["prec"], db_fold=False)
    assert HF.conv_wgrad_family(**_args(HF.conv_wgrad_family, wc)) == ("wconv_kernel", "plain")
