"""Case table and judges for the conv kernel families (conv_{fwd,dgrad,wgrad}_raw).

A plain helper module: tests/test_conv_cases_cpu.py checks the table and the judges without a GPU,
tests/test_conv_families_gpu.py runs the table through the kernels.

A *case* is one (op, precision, family, form) at a small shape with a ragged edge in every tiled
dimension.  A *bundle* is a set of options on top of it.  A *problem* (Problem) is a case x bundle
x judge with its operands built: every tensor the launch reads or writes is a view into a larger
1-D buffer with a moat before and after it (and, for channel slices, the unused channels of the
wide buffer between the samples).  Moats around inputs hold NaN, moats around outputs a fixed bit
pattern that is compared as int32 after the launch.

Judge "int": integer-valued operands, every partial sum exact in any order, the output bitwise
equal to the fp64 reference.  Judge "rnd": normal data (pre-rounded to the 16-bit type in the
16-bit modes), every element within the a-priori bound n * 2^-23 * A of the fp64 reference, A the
same op on absolute values and n the number of summed terms.

The same Problem runs on the CPU (device="cpu"): standin() computes it with torch's fp32 ops in
place of the kernel, which is how the judges themselves are tested.
"""
import collections
import json
import os
import zlib

import torch
import torch.nn.functional as F

TABLE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "conv_dispatch_v1.json")
with open(TABLE) as _f:
    ROWS = json.load(_f)

HALVES = ("bf16", "fp16")
U16 = {"bf16": 2.0 ** -8, "fp16": 2.0 ** -11}     # one RNE conversion to the 16-bit type
SLOPE32 = float(torch.tensor(0.2, dtype=torch.float32))   # LRELU_SLOPE as the kernels receive it
MOAT_BITS = 0x4B3C2D1E                                    # output moats (an ordinary finite float)
EPS = 2.0 ** -23


def _hdt(prec):
    return torch.float16 if prec == "fp16" else torch.bfloat16


def _q(t, prec):
    """16-bit modes round MFMA operands to bf16 / fp16: pre-rounded operands leave the kernel's
    fp32 accumulation as its only error."""
    return t.to(_hdt(prec)).to(t.dtype) if prec in HALVES else t


# ------------------------------------------------------------------------------------------
# what each (op, family, form) admits.  lin: the linear options (bias, acc, db, slice); act /
# xact / gact: output activation, activation on load, act'(gpre) epilogue; align: the chooser has
# an alignment rule for it (bundle (d) breaks it); ws: the launch takes a workspace (the
# allocator's free blocks and the workspace itself are poisoned with NaN first).
# ------------------------------------------------------------------------------------------
def _adm(lin, act=False, xact=False, gact=False, align=False, ws=False):
    return dict(lin=tuple(lin), act=act, xact=xact, gact=gact, align=align, ws=ws)


BAS = ("bias", "acc", "slice")
ADMITS = {
    ("fwd", "thin3_kernel", None): _adm(BAS, align=True),
    ("fwd", "pw_small_kernel", None): _adm(BAS, act=True, xact=True, align=True),
    ("fwd", "pglast_kernel", None): _adm(BAS, ws=True),
    ("fwd", "small_out_kernel", None): _adm(BAS),
    ("fwd", "small_in_kernel", None): _adm(BAS, act=True),
    ("fwd", "pwgemm_kernel", "io_ws"): _adm(BAS, act=True, align=True, ws=True),
    ("fwd", "pwgemm_kernel", "gemm"): _adm(BAS, act=True, xact=True, align=True, ws=True),
    ("fwd", "pwf32_kernel", None): _adm(BAS, act=True, align=True),
    ("fwd", "pconv_kernel", None): _adm(BAS, act=True, ws=True),
    ("fwd", "tconv_kernel", None): _adm(("bias", "slice"), act=True),
    ("fwd", "igemm_kernel", None): _adm(BAS, act=True, xact=True),
    ("dgrad", "thin3_kernel", None): _adm(("acc", "slice"), align=True),
    ("dgrad", "pw_small_kernel", None): _adm(("acc", "slice"), gact=True, align=True),
    ("dgrad", "pglast_kernel", None): _adm(("acc", "slice")),
    ("dgrad", "small_out_kernel", None): _adm(BAS),
    ("dgrad", "small_in_kernel", None): _adm(("acc", "slice")),
    ("dgrad", "pwgemm_kernel", "io_ws"): _adm(("acc", "slice"), align=True, ws=True),
    ("dgrad", "pwgemm_kernel", "gemm"): _adm(("acc", "slice"), gact=True, align=True, ws=True),
    ("dgrad", "pwf32_kernel", None): _adm(("acc", "slice"), gact=True, align=True),
    ("dgrad", "pconv_kernel", None): _adm(("acc", "slice"), gact=True, ws=True),
    ("dgrad", "pconvt_kernel", None): _adm(BAS, gact=True),
    ("dgrad", "tconv_kernel", None): _adm(("bias", "slice"), gact=True),
    ("dgrad", "igemm_kernel", None): _adm(BAS, gact=True),
    ("wgrad", "thin3_kernel", None): _adm(("db", "slice"), align=True, ws=True),
    ("wgrad", "pglast_kernel", None): _adm(("db", "slice"), ws=True),
    ("wgrad", "wgrad_small_kernel", None): _adm(("db", "slice"), ws=True),
    ("wgrad", "pwgemm_kernel", "gemm"): _adm(("db", "slice"), xact=True, align=True, ws=True),
    ("wgrad", "pwf32_kernel", None): _adm(("db", "slice"), align=True, ws=True),
    ("wgrad", "wconv_kernel", "db"): _adm(("slice",), align=True, ws=True),      # db is the form itself
    ("wgrad", "wconv_kernel", "plain"): _adm(("slice",), align=True, ws=True),   # with db the form changes
    ("wgrad", "igemm_kernel", None): _adm(("db", "slice"), xact=True, ws=True),
}
# the weight-grad families whose kernel also sums the bias grad into db (the others leave db alone)
DB_FOLDS = {("pglast_kernel", None), ("pwgemm_kernel", "gemm"), ("pwf32_kernel", None), ("wconv_kernel", "db")}
# (op, family, form, reason) the choosers can return but no case exercises: at most 5, none of them
# in the dispatch table (tests/test_conv_cases_cpu.py).  Nothing is left out.
LEFT_OUT = ()

ALL3 = ("fp32", "bf16", "fp16")
Case = collections.namedtuple("Case", "op prec fam form shape deep base toggles")


def _c(op, precs, fam, form, shape, deep=False, base=(), toggles=()):
    return [Case(op, pr, fam, form, shape, deep, tuple(base), tuple(toggles)) for pr in precs]


# shape = (N, Cin, H, W, Cout, K, stride, pad) of the forward conv, for all three ops.  deep: a
# long reduction that reaches a split / wide-tile path; the integer judge only (n > 600).
# (pwgemm's 256-row and 256 x 256 tiles need >= 512 / 256 such tiles, 1.6e7 outputs: they stay with
# test_ops_gpu.py's 1024 -> 1024 at 96 x 96 case.)
CASES = sum([
    # ---- forward
    _c("fwd", ALL3, "thin3_kernel", None, (2, 9, 4, 256, 1, 3, 1, 1)),
    _c("fwd", ALL3, "thin3_kernel", None, (3, 6, 4, 256, 3, 3, 1, 1)),
    _c("fwd", ALL3, "pw_small_kernel", None, (2, 12, 24, 22, 70, 1, 1, 0)),      # K small, two blocks of pixels
    _c("fwd", ALL3, "pw_small_kernel", None, (3, 70, 6, 10, 12, 1, 1, 0)),       # M small
    _c("fwd", ALL3, "pglast_kernel", None, (2, 24, 7, 9, 1, 4, 1, 1)),
    _c("fwd", ALL3, "pglast_kernel", None, (2, 256, 7, 7, 1, 4, 1, 1), deep=True),   # ordered partials
    _c("fwd", ALL3, "small_out_kernel", None, (2, 20, 9, 7, 3, 3, 1, 1)),
    _c("fwd", ALL3, "small_out_kernel", None, (2, 6, 10, 9, 5, 4, 2, 1)),
    _c("fwd", ALL3, "small_in_kernel", None, (2, 3, 9, 7, 20, 3, 1, 1)),
    _c("fwd", HALVES, "pwgemm_kernel", "io_ws", (2, 40, 12, 32, 72, 1, 1, 0)),
    _c("fwd", HALVES, "pwgemm_kernel", "io_ws", (2, 1024, 8, 16, 256, 1, 1, 0), deep=True),   # split-K forward
    _c("fwd", HALVES, "pwgemm_kernel", "gemm", (2, 44, 12, 32, 72, 1, 1, 0)),    # K % 8 != 0
    _c("fwd", ("fp32",), "pwf32_kernel", None, (2, 44, 12, 32, 72, 1, 1, 0)),
    _c("fwd", ("fp32",), "pwf32_kernel", None, (1, 1024, 8, 16, 64, 1, 1, 0), deep=True),
    _c("fwd", HALVES, "pconv_kernel", None, (2, 32, 10, 9, 72, 4, 2, 1)),
    _c("fwd", HALVES, "pconv_kernel", None, (2, 32, 7, 9, 72, 3, 1, 1)),
    _c("fwd", HALVES, "pconv_kernel", None, (2, 32, 6, 7, 40, 4, 1, 1)),
    _c("fwd", HALVES, "tconv_kernel", None, (2, 32, 9, 7, 40, 3, 2, 1)),
    _c("fwd", ALL3, "igemm_kernel", None, (2, 20, 9, 7, 24, 3, 2, 1)),
    _c("fwd", ALL3, "igemm_kernel", None, (3, 44, 6, 7, 70, 1, 1, 0)),           # a 1x1 the pointwise GEMMs refuse
    # ---- data-grad
    _c("dgrad", ALL3, "thin3_kernel", None, (2, 9, 4, 256, 1, 3, 1, 1)),
    _c("dgrad", ALL3, "thin3_kernel", None, (3, 6, 4, 256, 3, 3, 1, 1)),
    _c("dgrad", ALL3, "pw_small_kernel", None, (2, 12, 24, 22, 70, 1, 1, 0)),
    _c("dgrad", ALL3, "pw_small_kernel", None, (3, 70, 6, 10, 12, 1, 1, 0)),
    _c("dgrad", ALL3, "pglast_kernel", None, (2, 24, 7, 9, 1, 4, 1, 1)),
    _c("dgrad", ALL3, "small_out_kernel", None, (2, 6, 10, 9, 20, 4, 2, 1)),
    _c("dgrad", ALL3, "small_out_kernel", None, (2, 3, 9, 7, 20, 3, 1, 1)),
    _c("dgrad", ALL3, "small_in_kernel", None, (2, 20, 9, 7, 3, 3, 1, 1)),
    _c("dgrad", HALVES, "pwgemm_kernel", "io_ws", (2, 40, 12, 32, 72, 1, 1, 0)),
    _c("dgrad", HALVES, "pwgemm_kernel", "io_ws", (1, 64, 4, 32, 1024, 1, 1, 0), deep=True),   # split-K
    _c("dgrad", HALVES, "pwgemm_kernel", "gemm", (2, 36, 12, 32, 72, 1, 1, 0)),  # Cin % 8 != 0
    _c("dgrad", ("fp32",), "pwf32_kernel", None, (2, 36, 12, 32, 72, 1, 1, 0)),
    _c("dgrad", ("fp32",), "pwf32_kernel", None, (1, 64, 4, 32, 1024, 1, 1, 0), deep=True),
    _c("dgrad", HALVES, "pconv_kernel", None, (2, 40, 7, 9, 32, 3, 1, 1)),
    _c("dgrad", HALVES, "pconv_kernel", None, (2, 40, 8, 9, 32, 4, 1, 1)),
    _c("dgrad", HALVES, "pconvt_kernel", None, (2, 72, 10, 14, 32, 4, 2, 1)),
    _c("dgrad", HALVES, "pconvt_kernel", None, (2, 24, 9, 14, 32, 3, 2, 1)),     # odd H: the last row dropped
    _c("dgrad", HALVES, "tconv_kernel", None, (2, 20, 7, 7, 32, 3, 2, 1)),       # odd W: per-parity launches
    _c("dgrad", HALVES, "tconv_kernel", None, (2, 20, 8, 9, 32, 3, 1, 1), base=("bias",)),   # one launch
    _c("dgrad", ALL3, "igemm_kernel", None, (2, 20, 9, 7, 24, 3, 2, 1)),
    _c("dgrad", ALL3, "igemm_kernel", None, (3, 70, 6, 7, 44, 1, 1, 0)),
    # ---- weight-grad (n = N * Ho * Wo)
    _c("wgrad", ALL3, "thin3_kernel", None, (2, 9, 4, 256, 1, 3, 1, 1)),
    _c("wgrad", ALL3, "thin3_kernel", None, (1, 6, 4, 256, 3, 3, 1, 1)),
    _c("wgrad", ALL3, "pglast_kernel", None, (2, 24, 7, 9, 1, 4, 1, 1)),
    _c("wgrad", ALL3, "pglast_kernel", None, (3, 256, 7, 7, 1, 4, 1, 1)),
    _c("wgrad", ALL3, "wgrad_small_kernel", None, (2, 20, 9, 7, 3, 3, 1, 1)),
    _c("wgrad", ALL3, "wgrad_small_kernel", None, (2, 6, 10, 9, 5, 4, 2, 1)),
    _c("wgrad", ALL3, "wgrad_small_kernel", None, (2, 6, 8, 10, 20, 1, 1, 0)),   # Cin <= 8, 1x1
    _c("wgrad", HALVES, "pwgemm_kernel", "gemm", (3, 40, 8, 12, 72, 1, 1, 0)),
    _c("wgrad", HALVES, "pwgemm_kernel", "gemm", (2, 40, 64, 64, 72, 1, 1, 0), deep=True),    # split-K
    _c("wgrad", ("fp32",), "pwf32_kernel", None, (3, 36, 4, 12, 72, 1, 1, 0)),
    _c("wgrad", ("fp32",), "pwf32_kernel", None, (2, 36, 64, 64, 72, 1, 1, 0), deep=True),
    _c("wgrad", HALVES, "wconv_kernel", "db", (3, 32, 8, 8, 72, 3, 2, 1), base=("db",)),
    _c("wgrad", HALVES, "wconv_kernel", "db", (2, 32, 10, 12, 72, 4, 1, 1), base=("db",)),
    _c("wgrad", HALVES, "wconv_kernel", "db", (2, 32, 40, 44, 72, 4, 2, 1), deep=True, base=("db",)),
    _c("wgrad", HALVES, "wconv_kernel", "plain", (3, 32, 8, 8, 72, 3, 2, 1)),
    _c("wgrad", HALVES, "wconv_kernel", "plain", (2, 32, 10, 12, 72, 4, 1, 1)),
    _c("wgrad", HALVES, "wconv_kernel", "plain", (2, 64, 6, 8, 40, 3, 1, 1), base=("db",), toggles=("db_fold_off",)),
    _c("wgrad", ALL3, "igemm_kernel", None, (2, 20, 9, 7, 24, 3, 2, 1)),
    _c("wgrad", ALL3, "igemm_kernel", None, (2, 20, 40, 40, 24, 3, 1, 1), deep=True),
], [])


def case_id(c):
    return "%s-%s-%s%s-%s%s" % (c.op, c.prec, c.fam.replace("_kernel", ""), "." + c.form if c.form else "",
                                "x".join(map(str, c.shape)), "-deep" if c.deep else "")


# ------------------------------------------------------------------------------------------
# bundles
# ------------------------------------------------------------------------------------------
def _bundle(**kw):
    b = dict(bias=False, acc=False, db=False, slice=False, act=None, xact=None, gact=None, misalign=False)
    b.update(kw)
    return b


def bundle_id(b):
    parts = [k for k in ("bias", "acc", "db", "slice", "misalign") if b[k]]
    parts += ["%s=%s" % (k, b[k]) for k in ("act", "xact", "gact") if b[k]]
    return "+".join(parts) or "plain"


def row_flags(r):
    """The option flags of a dispatch-table row (non-dense: a batch stride that is not C*H*W)."""
    Ho = r["Ho"] if "Ho" in r else (r["H"] + 2 * r["pad"] - r["KH"]) // r["stride"] + 1
    Wo = r["Wo"] if "Wo" in r else (r["W"] + 2 * r["pad"] - r["KW"]) // r["stride"] + 1
    px, py = r["Cin"] * r["H"] * r["W"], r["Cout"] * Ho * Wo
    if r["op"] == "fwd":
        nd = r["xbs"] != px or r["ybs"] != py
    elif r["op"] == "dgrad":
        nd = r["dybs"] != py or r["dxbs"] != px or (r["gpre_ptr"] is not None and r["gbs"] != px)
    else:
        nd = r["dybs"] != py or r["xbs"] != px
    return (r.get("act"), r.get("xact"), bool(r.get("accumulate")), bool(r.get("has_bias")), bool(r.get("has_db")),
            r.get("gpre_ptr") is not None, bool(nd))


def bundle_flags(b):
    return (b["act"], b["xact"], b["acc"], b["bias"], b["db"], b["gact"] is not None, b["slice"] or b["misalign"])


def table_combos():
    """{(prec, op, family, form, *row_flags)} of the dispatch table."""
    return {(r["prec"], r["op"], r["fam"], r["form"]) + row_flags(r) for r in ROWS}


def bundles(case):
    """The option bundles of a case: (a) plain, (b) every linear option the family admits (and that
    set without the slices), (c) each activation option, (d) bundle (b) with the views shifted off
    the family's alignment rule, and one bundle for each combination of options with which the
    dispatch table records this (op, family, form)."""
    adm = ADMITS[(case.op, case.fam, case.form)]
    base = {k: True for k in case.base}
    lin = {k: True for k in adm["lin"]}
    dense = {k: True for k in adm["lin"] if k != "slice"}
    out = [_bundle(**base), _bundle(**dict(base, **lin))]
    if not case.deep:
        out.append(_bundle(**dict(base, **dense)))
        if adm["act"]:
            ab = {"bias": True} if "bias" in adm["lin"] else {}
            out += [_bundle(**dict(base, act=a, **ab)) for a in ("relu", "lrelu")]
        if adm["gact"]:
            out += [_bundle(**dict(base, gact=a)) for a in ("relu", "lrelu", "gelu")]
            out.append(_bundle(**dict(base, gact="lrelu", slice=True)))
        if adm["xact"]:
            out += [_bundle(**dict(base, xact="gelu")), _bundle(**dict(base, xact="gelu", **lin))]
        if adm["align"]:
            out.append(_bundle(**dict(base, misalign=True, **lin)))
        for r in ROWS:
            if (r["op"], r["fam"], r["form"]) != (case.op, case.fam, case.form):
                continue
            if (r["prec"] == "fp32") != (case.prec == "fp32"):
                continue
            act, xact, acc, bias, db, gpre, nd = row_flags(r)
            out.append(_bundle(**dict(dict(act=act, xact=xact, acc=acc, bias=bias, db=db,
                                           gact=(r.get("gact") or "relu") if gpre else None, slice=nd), **base)))
    seen, uniq = set(), []
    for b in out:
        if bundle_id(b) not in seen:
            seen.add(bundle_id(b))
            uniq.append(b)
    return uniq


def judges(case, b):
    """The integer judge wherever there is no GELU; the random-data judge wherever n stays short."""
    js = []
    if b["xact"] != "gelu" and b["gact"] != "gelu":
        js.append("int")
    if not case.deep:
        js.append("rnd")
    return js


def problems():
    """[(id, case, bundle, judge)] -- the GPU module's parameters."""
    out = []
    for c in CASES:
        for b in bundles(c):
            for j in judges(c, b):
                out.append(("%s-%s-%s" % (case_id(c), bundle_id(b), j), c, b, j))
    return out


# ------------------------------------------------------------------------------------------
# guarded tensors
# ------------------------------------------------------------------------------------------
class Slot:
    """A tensor as a view into a 1-D buffer: ``view`` is what the launch gets, everything else in
    ``buf`` is moat (NaN around an input, MOAT_BITS around an output)."""

    def __init__(self, data, kind, device, wide=None, lead=0, moat=1 << 14):
        data = data.to(torch.float32)
        self.kind = kind
        moat = (moat + 63) // 64 * 64
        if wide is None:
            n = data.numel()
            self.buf = torch.empty(2 * moat + lead + n, dtype=torch.float32)
            self._fill()
            self.view = self.buf[moat + lead:moat + lead + n].view(data.shape)
        else:   # channels [c_off, c_off + C) of an (N, c_tot, H, W) buffer
            c_off, c_tot = wide
            N, C, H, W = data.shape
            n = N * c_tot * H * W
            self.buf = torch.empty(2 * moat + lead + n, dtype=torch.float32)
            self._fill()
            self.view = self.buf[moat + lead:moat + lead + n].view(N, c_tot, H, W)[:, c_off:c_off + C]
        self.view.copy_(data)
        idx = torch.arange(self.buf.numel()).as_strided(self.view.size(), self.view.stride(),
                                                        self.view.storage_offset())
        self.moat_mask = torch.ones(self.buf.numel(), dtype=torch.bool)
        self.moat_mask[idx.reshape(-1)] = False
        if device != "cpu":
            off, size, stride = self.view.storage_offset(), self.view.size(), self.view.stride()
            self.buf = self.buf.to(device)
            self.view = self.buf.as_strided(size, stride, off)
        self.before = self.bits().clone()

    def _fill(self):
        if self.kind == "in":
            self.buf.fill_(float("nan"))
        else:
            self.buf.view(torch.int32).fill_(MOAT_BITS)

    def bits(self):
        return self.buf.view(torch.int32).cpu()

    def check(self, name):
        """An input: the whole buffer unchanged.  An output: every moat element unchanged."""
        now = self.bits()
        bad = (now != self.before)
        if self.kind == "out":
            bad &= self.moat_mask
        if bad.any():
            i = int(bad.nonzero()[0])
            inside = (~self.moat_mask).nonzero().reshape(-1)
            raise AssertionError("%s: %d element(s) %s written; first at buffer offset %d (the view spans %d..%d)"
                                 % (name, int(bad.sum()), "of the moat" if self.kind == "out" else "of an input",
                                    i, int(inside[0]), int(inside[-1])))


class Problem:
    """A case x bundle x judge with its operands.  ``cpu`` holds the fp64 operands, ``slots`` the
    guarded tensors on ``device``."""

    def __init__(self, case, b, judge, device="cpu"):
        if b["acc"] and (b["act"] or b["gact"]) and judge == "int":
            raise ValueError("the integer judge does not take an activation together with accumulate")
        self.case, self.b, self.judge, self.device = case, b, judge, device
        self.fam = (case.fam, case.form)                      # expect_family() sets both from the chooser
        self.db_summed = b["db"] and self.fam in DB_FOLDS
        N, Cin, H, W, Cout, K, s, p = case.shape
        Ho, Wo = (H + 2 * p - K) // s + 1, (W + 2 * p - K) // s + 1
        self.Ho, self.Wo = Ho, Wo
        g = torch.Generator().manual_seed(zlib.crc32(("%s|%s|%s" % (case_id(case), bundle_id(b), judge)).encode()))
        prec, op = case.prec, case.op

        def act_t(*shape):      # activations / gradients
            if judge == "int":
                return torch.randint(-3, 4, shape, generator=g).double()
            return _q(torch.randn(shape, generator=g), prec).double()

        def wt_t(*shape):
            if judge == "int":
                return torch.randint(-2, 3, shape, generator=g).double()
            return _q(torch.randn(shape, generator=g) * 0.5, prec).double()

        def add_t(*shape):      # bias, y0: fp32 addends
            if judge == "int":
                return torch.randint(-8, 9, shape, generator=g).double()
            return torch.randn(shape, generator=g).double()

        d = {}
        d["x"] = act_t(N, Cin, H, W) if op != "dgrad" else None
        d["dy"] = act_t(N, Cout, Ho, Wo) if op != "fwd" else None
        d["w"] = wt_t(Cout, Cin, K, K) if op != "wgrad" else None
        d["bias"] = add_t(Cout if op == "fwd" else Cin) if b["bias"] else None
        d["gpre"] = torch.randn((N, Cin, H, W), generator=g).double() if b["gact"] else None
        out_shape = {"fwd": (N, Cout, Ho, Wo), "dgrad": (N, Cin, H, W), "wgrad": (Cout, Cin, K, K)}[op]
        d["y0"] = add_t(*out_shape) if (b["acc"] or op == "wgrad") else None
        d["db0"] = add_t(Cout) if b["db"] else None
        self.cpu = d
        self.out_shape = out_shape

        lead = 1 if b["misalign"] else 0
        sliced = b["slice"] or b["misalign"]

        def plane(t, kind, fill=None):
            if t is None and fill is None:
                return None
            data = t if t is not None else fill
            n_, c_, h_, w_ = data.shape
            wide = (4, (4 + c_ + 1 + 3) // 4 * 4) if sliced else None
            return Slot(data, kind, device, wide=wide, lead=lead, moat=max(1 << 14, 32 * h_ * w_))

        nan_out = torch.full(out_shape, float("nan"))   # an output that is not accumulated into starts as NaN
        s_ = {}
        if op == "wgrad":
            s_["x"], s_["dy"] = plane(d["x"], "in"), plane(d["dy"], "in")
            s_["out"] = Slot(d["y0"], "out", device)
            s_["db"] = Slot(d["db0"], "out", device) if b["db"] else None
        else:
            src = "x" if op == "fwd" else "dy"
            s_[src] = plane(d[src], "in")
            s_["w"] = Slot(d["w"], "in", device)
            s_["bias"] = Slot(d["bias"], "in", device) if b["bias"] else None
            s_["gpre"] = plane(d["gpre"], "in")
            s_["out"] = plane(d["y0"], "out", fill=nan_out)
        self.slots = {k: v for k, v in s_.items() if v is not None}

    def v(self, name):
        sl = self.slots.get(name)
        return None if sl is None else sl.view

    # -- the number of summed terms of one output element (an upper bound at the borders)
    def n_terms(self):
        N, Cin, H, W, Cout, K, s, p = self.case.shape
        b = self.b
        n = {"fwd": Cin * K * K, "dgrad": Cout * K * K, "wgrad": N * self.Ho * self.Wo}[self.case.op]
        n += int(b["bias"]) + int(b["acc"] or self.case.op == "wgrad")
        n += int(b["act"] == "lrelu") + int(b["gact"] in ("lrelu", "gelu"))    # the activation's own product
        return n


# ------------------------------------------------------------------------------------------
# the op itself, in any dtype (fp64: the reference; fp32: the CPU stand-in for a kernel)
# ------------------------------------------------------------------------------------------
def gelu_exact(x):
    """common.h gelu_f: nn.GELU()'s erf form, the one ACT_GELU selects in every raw conv launcher."""
    return 0.5 * x * (1.0 + torch.erf(x * 0.7071067811865476))


def gelu_grad_exact(x):
    """common.h gelu_g: Phi(x) + x phi(x)."""
    return 0.5 * (1.0 + torch.erf(x * 0.7071067811865476)) + x * torch.exp(-0.5 * x * x) * 0.3989422804014327


def act_fwd(z, act):
    if act == "relu":
        return torch.clamp_min(z, 0.0)
    if act == "lrelu":
        return torch.where(z > 0, z, z * torch.tensor(SLOPE32, dtype=torch.float32).to(z.dtype))
    if act == "gelu":
        return gelu_exact(z)
    return z


def act_grad(x, act):
    if act == "relu":
        return (x > 0).to(x.dtype)
    if act == "lrelu":
        one = torch.ones((), dtype=x.dtype)
        return torch.where(x > 0, one, torch.tensor(SLOPE32, dtype=torch.float32).to(x.dtype))
    if act == "gelu":
        return gelu_grad_exact(x)
    raise ValueError(act)


def _conv_weight(x, wshape, dy, s, p):
    """Weight-grad of conv2d by the definition (one einsum per tap): exact in the operands' dtype."""
    Cout, Cin, K, _ = wshape
    N, _, Ho, Wo = dy.shape
    xp = F.pad(x, (p, p, p, p))
    dw = torch.empty(wshape, dtype=x.dtype)
    for kh in range(K):
        for kw in range(K):
            xs = xp[:, :, kh:kh + (Ho - 1) * s + 1:s, kw:kw + (Wo - 1) * s + 1:s]
            dw[:, :, kh, kw] = torch.einsum("nohw,nchw->oc", dy, xs)
    return dw


def compute(P, dt, mode="ref", drop_tap_col=False, conv_only=False, xact=True):
    """{'out': ..., 'db': ...} of problem P computed in dtype ``dt``.  mode "abs": the same op on
    absolute values without the activations' sign logic (the bound's A); mode "pre": the value the
    act'(gpre) factor multiplies / the output activation is applied to.  drop_tap_col: the forward
    or data-grad with the weight's tap column kw = pad left out (an injected defect's material).
    conv_only: the reduction alone, without bias, act'(gpre), activation and y0; xact=False: without
    the activation on load (both for the margins of bound_rnd)."""
    c, b, d = P.case, P.b, P.cpu
    if conv_only:
        b = dict(b, bias=False, gact=None, act=None)
        d = dict(d, bias=None, y0=None)
    if not xact:
        b = dict(b, xact=None)
    N, Cin, H, W, Cout, K, s, p = c.shape
    ab = (lambda t: t.abs()) if mode == "abs" else (lambda t: t)
    cast = lambda t: None if t is None else ab(t.to(dt))
    res = {}
    if c.op in ("fwd", "wgrad"):
        x = d["x"].to(dt)
        if b["xact"]:
            x = act_fwd(x, b["xact"])
            if c.prec in HALVES:
                x = x.to(torch.float32).to(_hdt(c.prec)).to(dt)   # the kernel rounds the activated operand
        x = ab(x)
    if c.op == "fwd":
        w = cast(d["w"])
        if drop_tap_col:
            w = w.clone()
            w[:, :, :, p] = 0
        z = F.conv2d(x, w, cast(d["bias"]), stride=s, padding=p)
    elif c.op == "dgrad":
        w = cast(d["w"])
        if drop_tap_col:
            w = w.clone()
            w[:, :, :, p] = 0
        z = torch.nn.grad.conv2d_input((N, Cin, H, W), w, cast(d["dy"]), stride=s, padding=p)
        if b["bias"]:
            z = z + cast(d["bias"]).view(1, -1, 1, 1)
    else:
        z = _conv_weight(x, (Cout, Cin, K, K), cast(d["dy"]), s, p)
    if mode == "pre":
        return {"out": z}
    if b["gact"]:
        z = z * ab(act_grad(d["gpre"].to(dt), b["gact"]))
    if mode != "abs":
        z = act_fwd(z, b["act"])
    if d["y0"] is not None:
        z = z + cast(d["y0"])
    res["out"] = z
    if b["db"]:
        res["db"] = cast(d["db0"])
        if P.db_summed:
            res["db"] = res["db"] + cast(d["dy"]).sum(dim=(0, 2, 3))
    return res


def standin(P):
    """torch's CPU fp32 ops in place of the kernel: writes the outputs of P (device "cpu")."""
    got = compute(P, torch.float32)
    P.v("out").copy_(got["out"])
    if P.b["db"]:
        P.v("db").copy_(got["db"])


# ------------------------------------------------------------------------------------------
# which family a problem takes, and the launch
# ------------------------------------------------------------------------------------------
class state:
    """with state(HF, case, gpu): the module state a case needs (precision, PGLAST, WCONV_DB_FOLD),
    restored afterwards.  Without a GPU the precision is set as test_dispatch_cpu.py does, without
    the library's half-type switch."""

    def __init__(self, HF, case, gpu):
        self.HF, self.case, self.gpu = HF, case, gpu

    def __enter__(self):
        HF = self.HF
        self.old = HF._state["prec"], HF.PGLAST[0], HF.WCONV_DB_FOLD
        if self.gpu:
            HF.set_precision(self.case.prec)
        else:
            HF._state["prec"] = self.case.prec
        HF.PGLAST[0] = True
        HF.WCONV_DB_FOLD = "db_fold_off" not in self.case.toggles
        return self

    def __exit__(self, *exc):
        HF = self.HF
        _, HF.PGLAST[0], HF.WCONV_DB_FOLD = self.old
        if self.gpu:
            HF.set_precision("fp32")
        else:
            HF._state["prec"] = self.old[0]


def _bs(t):
    N, C, H, W = t.shape
    return t.stride(0) if N > 1 else C * H * W


def chosen(HF, P):
    """(family, form) the choosers name for P's tensors, asked as conv_*_raw asks."""
    c, b = P.case, P.b
    N, Cin, H, W, Cout, K, s, p = c.shape
    if c.op == "fwd":
        x, y, w = P.v("x"), P.v("out"), P.v("w")
        return HF.conv_fwd_family(Cin, H, W, Cout, K, K, s, p, _bs(x), _bs(y), 0, x.data_ptr(), y.data_ptr(),
                                  w.data_ptr(), None, 4, True, b["act"], b["xact"], b["acc"])
    if c.op == "dgrad":
        dy, dx, w, gp = P.v("dy"), P.v("out"), P.v("w"), P.v("gpre")
        return HF.conv_dgrad_family(Cin, H, W, Cout, K, K, s, p, P.Ho, P.Wo, _bs(dy), _bs(dx),
                                    0 if gp is None else _bs(gp), dy.data_ptr(), dx.data_ptr(), w.data_ptr(),
                                    None if gp is None else gp.data_ptr(), 4, True, None, b["bias"], b["acc"])
    dy, x = P.v("dy"), P.v("x")
    return HF.conv_wgrad_family(N, Cin, H, W, Cout, K, K, s, p, _bs(dy), _bs(x), dy.data_ptr(), x.data_ptr(), 4, True,
                                b["xact"], b["db"])


def expect_family(HF, P):
    """The family P must take: the case's own, or under misalignment whatever the chooser names.
    Sets P.fam and P.db_summed."""
    fam = chosen(HF, P)
    if not P.b["misalign"]:
        assert fam == (P.case.fam, P.case.form), "%s with %s takes %r, not its own family" % (
            case_id(P.case), bundle_id(P.b), fam)
    else:
        assert fam != (P.case.fam, P.case.form) or not ADMITS[(P.case.op,) + fam]["align"], \
            "%s: the shifted views still take %r" % (case_id(P.case), fam)
    P.fam = fam
    P.db_summed = P.b["db"] and fam in DB_FOLDS
    return fam


def launch(HF, P):
    """The kernel launch of P on the GPU: poisons scratch first where the family takes any, asserts
    the family on the timer afterwards."""
    c, b = P.case, P.b
    N, Cin, H, W, Cout, K, s, p = c.shape
    fam = P.fam
    real_ws = HF._ws
    if ADMITS[(c.op,) + fam]["ws"]:
        # the allocator's free blocks start as NaN (test_wconv_db_fold_vs_channel_sum), and so does
        # the workspace the launcher hands over, whichever block it came from
        for n in (1 << 14, 1 << 18, (1 << 20) + (1 << 18)):
            poison = torch.full((n,), float("nan"), device=P.device)
            del poison

        def nan_ws(query, *dims, like):
            t = real_ws(query, *dims, like=like)
            if t is not None:
                t.fill_(float("nan"))
            return t
        HF._ws = nan_ws
    HF.IGEMM_TIMER.rec, HF.IGEMM_TIMER.on = [], True
    try:
        if c.op == "fwd":
            HF.conv_fwd_raw(P.v("x"), P.v("w"), P.v("bias"), s, p, act=b["act"], out=P.v("out"),
                            accumulate=b["acc"], xact=b["xact"])
        elif c.op == "dgrad":
            HF.conv_dgrad_raw(P.v("dy"), P.v("w"), (N, Cin, H, W), s, p, bias=P.v("bias"), gpre=P.v("gpre"),
                              gact=b["gact"], out=P.v("out"), accumulate=b["acc"])
        else:
            did = HF.conv_wgrad_raw(P.v("dy"), P.v("x"), P.v("out"), s, p, xact=b["xact"], db=P.v("db"))
            assert bool(did) == bool(P.db_summed), "conv_wgrad_raw returned %r for %r" % (did, fam)
    finally:
        HF.IGEMM_TIMER.on = False
        HF._ws = real_ws
    torch.cuda.synchronize()
    assert HF.IGEMM_TIMER.rec[-1][4] == fam[0], (HF.IGEMM_TIMER.rec[-1][4], fam)


# ------------------------------------------------------------------------------------------
# the judges
# ------------------------------------------------------------------------------------------
def _where(idx, shape):
    """An element's index and its distance from the far edge of every dimension (tile-edge view)."""
    return "index %s of %s (from the far edges: %s)" % (tuple(idx), tuple(shape),
                                                        tuple(n - 1 - i for i, n in zip(idx, shape)))


def check_guards(P):
    for name, sl in P.slots.items():
        sl.check("%s %s: tensor '%s'" % (case_id(P.case), bundle_id(P.b), name))


def judge_int(P, got, ref, pre=None, what="out"):
    """Bitwise equal to the fp64 reference; the elements an lrelu scaled may be one fp32 ulp off
    torch's fp32 product."""
    n = P.n_terms()
    assert n * 6 + 16 < 2 ** 24, "integer data no longer exact at n = %d" % n
    tag = "%s %s [%s, int]" % (case_id(P.case), bundle_id(P.b), what)
    assert torch.isfinite(got).all(), "%s: non-finite output at %s" % (
        tag, _where((~torch.isfinite(got)).nonzero()[0].tolist(), got.shape))
    want = ref.to(torch.float32)
    scaled = None
    if what == "out" and P.b["act"] == "lrelu":
        scaled = pre < 0
        want = F.leaky_relu(pre.to(torch.float32), 0.2)
    elif what == "out" and P.b["gact"] == "lrelu":
        scaled = P.cpu["gpre"] <= 0
        want = pre.to(torch.float32) * act_grad(P.cpu["gpre"].to(torch.float32), "lrelu")
    if scaled is None:
        bad = got != want
    else:
        bad = torch.where(scaled, (got - want).abs() > EPS * want.abs(), got != want)
    if bad.any():
        i = bad.nonzero()[0].tolist()
        t = tuple(i)
        raise AssertionError("%s: %d of %d elements differ on integer data; first at %s: got %r, exact %r"
                             % (tag, int(bad.sum()), bad.numel(), _where(i, got.shape), got[t].item(), want[t].item()))
    return 0.0


def bound_rnd(P, what="out"):
    """n * 2^-23 * A per element (and the margins of an in-kernel GELU), in fp64."""
    c, b = P.case, P.b
    A = compute(P, torch.float64, mode="abs")[what]
    if what == "db":
        return (c.shape[0] * P.Ho * P.Wo + 1) * EPS * A
    bound = P.n_terms() * EPS * A
    if b["xact"] == "gelu":
        # gelu_f in fp32: |gelu_f(x) - gelu(x)| <= 2^-22 |x| from the rounding of x/sqrt2, of 1 + erf
        # (<= 2, so absolute 2^-23 per rounding and for the few-ulp erf polynomial) and of the two
        # products; doubled.  In the 16-bit modes the activated operand is then rounded: 2 u A.
        bound = bound + 2.0 ** -21 * compute(P, torch.float64, mode="abs", conv_only=True, xact=False)["out"]
        if c.prec in HALVES:
            bound = bound + 2 * U16[c.prec] * compute(P, torch.float64, mode="abs", conv_only=True)["out"]
    if b["gact"] == "gelu":
        # gelu_g in fp32: Phi to 2^-23 absolute (as above), x phi(x) <= 0.25 through __expf whose
        # argument scaling costs |x^2/2| 2^-24 relative (|gpre| < 6: < 18 ulp) -> < 2^-21 absolute
        bound = bound + 2.0 ** -21 * compute(P, torch.float64, mode="pre")["out"].abs()
    return bound


def judge_rnd(P, got, ref, what="out"):
    """Every element within the a-priori bound; returns the largest ratio to it."""
    tag = "%s %s [%s, rnd]" % (case_id(P.case), bundle_id(P.b), what)
    assert torch.isfinite(got).all(), "%s: non-finite output at %s" % (
        tag, _where((~torch.isfinite(got)).nonzero()[0].tolist(), got.shape))
    bound = bound_rnd(P, what)
    err = (got.double() - ref).abs()
    ratio = err / bound.clamp_min(1e-300)
    ratio = torch.where((err == 0), torch.zeros_like(ratio), ratio)
    worst = int(ratio.argmax())
    i = list(torch.unravel_index(torch.tensor(worst), got.shape))
    i = [int(k) for k in i]
    r = float(ratio.reshape(-1)[worst])
    if not r <= 1.0:
        t = tuple(i)
        raise AssertionError("%s: %d of %d elements outside n*2^-23*A (n = %d); worst at %s: got %.9g, ref %.9g, "
                             "%.3g x the bound %.3g" % (tag, int((ratio > 1).sum()), ratio.numel(), P.n_terms(),
                                                        _where(i, got.shape), got[t].item(), ref[t].item(), r,
                                                        bound[t].item()))
    return r


def check(P):
    """Guards, then the problem's judge on every output; returns the largest judge-2 ratio (0 for
    the integer judge)."""
    check_guards(P)
    ref = compute(P, torch.float64)
    pre = compute(P, torch.float64, mode="pre")["out"] if P.judge == "int" else None
    worst = 0.0
    for what in ("out", "db") if P.b["db"] else ("out",):
        got = P.v(what).detach().cpu().contiguous()
        if P.judge == "int":
            judge_int(P, got, ref[what], pre, what)
        else:
            worst = max(worst, judge_rnd(P, got, ref[what], what))
    return worst
