"""Autograd Functions over libdsgan_hip.so -- the fused ops the DS-GAN networks are built from.

Every forward and backward here is one or more HIP kernels launched on torch's current stream.
PyTorch provides allocation (caching allocator), stream handles and the autograd tape only.

Weight/bias gradients are *accumulated* by the kernels straight into ``param.grad``, which
``dsgan_hip.flat.FlatParams`` binds to a view of one flat fp32 buffer (zeroed once per step);
the Functions therefore return ``None`` for parameters.  A parameter whose ``requires_grad`` is
False (the frozen VGG16, or D during the G step, DSGAN/models/base_model.py:171-177) gets no
weight-grad launch at all.
"""
import contextlib
import ctypes
import os
import math

import torch

from . import _lib
from ._lib import call, ptr, stream


def wsa(t):
    """(pointer, element count) of a scratch tensor (None -> NULL, 0): every scratch-taking entry
    point takes the buffer's size right after it and refuses an undersized one (include/dsgan_hip.h).
    Inside deferred_splits() the tensor is a keep-alive candidate of the call it is passed to: held
    until split_flush() when that call queued a split reduction (which reads it after the call has
    returned), dropped otherwise (InstanceNorm workspaces, forward scratch and the like
    are not held for the whole backward pass)."""
    if t is not None and _DEFER_KEEP[0] is not None:
        _DEFER_CAND.append(t)
    return (ptr(t), t.numel() if t is not None else 0)


# Deferred split reductions (split_reduce.hip): inside deferred_splits() every weight-grad launcher
# queues its fixed-order split reduction (dw += sum_s partials[s]) instead of launching it, and the
# block's end issues the queue as a few batched launches -- ~160 small reduction launches per
# training step become a handful.  Only parameter gradients go through these reductions, and they
# are read only after the backward pass (the optimizer, the non-finite guard) or by the DDP bucket
# all-reduce, which flushes first (dist.GradBuckets._launch).  The scratch of a call that queued a
# reduction (wsa, _keep) is held until the flush.
DEFER_SPLITS = [os.environ.get("DSGAN_DEFER_SPLITS", "1") != "0"]   # (=0: immediate, for A/B runs)
_DEFER_KEEP = [None]
_DEFER_CAND = []


def _defer_hook(queued):
    """_lib.call's report after each entry point: keep that call's candidates if it queued a reduction."""
    if queued and _DEFER_KEEP[0] is not None:
        _DEFER_KEEP[0].extend(_DEFER_CAND)
    _DEFER_CAND.clear()


def _keep(t):
    if _DEFER_KEEP[0] is not None:
        _DEFER_CAND.append(t)
    return t


def split_flush():
    """Launch the queued split reductions (no-op when none are queued)."""
    lib = _lib.load()
    if lib.dsgan_split_pending() > 0:
        call("dsgan_split_flush", stream())
    if _DEFER_KEEP[0] is not None:
        _DEFER_KEEP[0] = []
    _DEFER_CAND.clear()


@contextlib.contextmanager
def deferred_splits():
    """Run a backward pass with its weight-grads' split reductions queued and flushed at the end
    (nested use is a no-op; DEFER_SPLITS[0] = False turns the batching off)."""
    if not DEFER_SPLITS[0] or _DEFER_KEEP[0] is not None:
        yield
        return
    lib = _lib.load()
    _DEFER_KEEP[0] = []
    _DEFER_CAND.clear()
    _lib.DEFER_HOOK[0] = _defer_hook
    lib.dsgan_split_defer(1)
    try:
        yield
    finally:
        lib.dsgan_split_defer(0)
        _lib.DEFER_HOOK[0] = None
        try:
            split_flush()
        finally:
            _DEFER_KEEP[0] = None
            _DEFER_CAND.clear()


# PatchGAN 4x4 weight-grads also sum the conv's bias grad from their staged dy tiles
# (dsgan_wconv_db) instead of a separate channel-sum pass (78 launches per step fewer); the
# round-3 non-finite replay with it does not reproduce on the round-4 tree (tools/nan_diag.py,
# profiles/r04/nan_diag.txt); see DESIGN.md section 6.
WCONV_DB_FOLD = True

ACT = {None: 0, "none": 0, "gelu": 1, "relu": 2, "lrelu": 3, "sigmoid": 4}
ACT_GELU_FAST = 5   # common.h: GELU by A&S 7.1.26 (|err| <= 1.5e-7), the 16-bit modes' InstanceNorm epilogues
PREC = {"fp32": 0, "bf16": 1, "fp16": 1}   # the C ABI's prec: 0 exact f32, 1 16-bit MFMA operands
_state = {"prec": "fp32"}
IN_EPS = 1e-5
LRELU_SLOPE = 0.2


def set_precision(p):
    """'fp32' (exact f32 MFMA, parity mode), 'bf16' (bf16 MFMA operands, fp32 accumulate) or
    'fp16' (IEEE fp16 MFMA operands and 16-bit storage, fp32 accumulate; BASELINE configs[4]).
    bf16 and fp16 run the same kernels: the library's half type (dsgan_set_half_type) selects
    the 16-bit instantiation, so it follows the precision here."""
    if p not in PREC:
        raise ValueError(p)
    _state["prec"] = p
    want = 1 if p == "fp16" else 0
    lib = _lib.load()
    if lib.dsgan_get_half_type() != want:
        call("dsgan_set_half_type", want)


def get_precision():
    return _state["prec"]


@contextlib.contextmanager
def precision(p):
    """Scoped precision: ops created inside run (forward AND backward -- the contraction
    Functions record it in ctx) at precision ``p``.  ``None`` keeps the current one."""
    old = _state["prec"]
    if p is not None:
        set_precision(p)
    try:
        yield
    finally:
        set_precision(old)


def _prec():
    return PREC[_state["prec"]]


def _is16():
    """16-bit MFMA operands (bf16 or fp16 mode)."""
    return _state["prec"] != "fp32"


def half_dtype():
    """torch dtype of the 16-bit operand / storage tensors of the current precision."""
    return torch.float16 if _state["prec"] == "fp16" else torch.bfloat16


class KernelTimer:
    """Brackets every implicit-GEMM launch with HIP events on the launch stream (bench.py's
    roofline leg).  Off by default; when on, records (start, end, algorithmic_flops).

    ``kernel_only=True`` (IGEMM_TIMER) also switches the library's kernel-only timer
    (``dsgan_ktimer``) with it: the pointwise GEMM launchers then record an event pair around the
    GEMM kernel itself, without the split-K finishing pass the same C-ABI call may issue --
    ``pw_kernel_ms()`` reads those, the figure rocprofv3 reports for ``pwgemm_kernel``."""

    def __init__(self, kernel_only=False):
        self._on = False
        self.rec = []
        self.kernel_only = kernel_only

    @property
    def on(self):
        return self._on

    @on.setter
    def on(self, v):
        self._on = bool(v)
        if self.kernel_only:
            _lib.load().dsgan_ktimer(1 if v else 0)

    def reset(self):
        """Drop the records (and the library's kernel-only pairs)."""
        self.rec = []
        if self.kernel_only:
            _lib.load().dsgan_ktimer(-1)

    def pw_kernel_ms(self):
        """Per-launch ms of the pointwise GEMM kernels recorded since reset() (kernel-only timer),
        or None when the library could not read them (events recorded by graph nodes)."""
        lib = _lib.load()
        torch.cuda.synchronize()
        n = lib.dsgan_ktimer(1 if self._on else 0)
        if n <= 0:
            return []
        buf = (ctypes.c_float * n)()
        got = lib.dsgan_ktimer_read(buf, n)
        if got != n:
            return None
        return list(buf)

    def begin(self):
        if not self.on:
            return None
        e0 = torch.cuda.Event(enable_timing=True)
        e0.record()
        return e0

    def end(self, e0, flops, tag=None, fam="other", nbytes=0):
        if e0 is None:
            return
        e1 = torch.cuda.Event(enable_timing=True)
        e1.record()
        self.rec.append((e0, e1, flops, tag, fam, nbytes))

    def summary(self):
        torch.cuda.synchronize()
        ms = sum(r[0].elapsed_time(r[1]) for r in self.rec)
        fl = sum(r[2] for r in self.rec)
        return dict(launches=len(self.rec), total_ms=ms, flops=fl)

    def families(self):
        """{kernel family: [launches, ms, algorithmic flops, algorithmic bytes]} over the recorded
        launches (bytes: every operand the launch must read or write once, in its stored dtype)."""
        torch.cuda.synchronize()
        out = {}
        for r in self.rec:
            a = out.setdefault(r[4], [0, 0.0, 0.0, 0.0])
            a[0] += 1
            a[1] += r[0].elapsed_time(r[1])
            a[2] += r[2]
            a[3] += r[5]
        return out

    def table(self):
        torch.cuda.synchronize()
        return [(r[0].elapsed_time(r[1]), r[2], r[3] + (r[4],)) for r in self.rec]


IGEMM_TIMER = KernelTimer(kernel_only=True)
AUX_TIMER = KernelTimer()   # the HBM-bound depthwise / InstanceNorm launches (tools/launch_table.py)


class _timed:
    """``with _timed(timer, flops, tag, fam, nbytes): call(...)`` -- the one place a launch is
    bracketed with a KernelTimer's event pair; the record is (e0, e1, flops, tag, fam, nbytes).
    With the timer off it creates no event and records nothing."""
    __slots__ = ("timer", "rec", "e0")

    def __init__(self, timer, flops, tag=None, fam="other", nbytes=0):
        self.timer, self.rec = timer, (flops, tag, fam, nbytes)

    def __enter__(self):
        self.e0 = self.timer.begin()

    def __exit__(self, etype, exc, tb):
        if etype is None:
            self.timer.end(self.e0, *self.rec)


def _ws(query, *dims, like):
    """fp32 scratch of a launch, on ``like``'s device: as many elements as the library's ``query``
    (a ``*_workspace`` function) returns for ``dims``, None when that is 0.  Hand it to the entry
    point through wsa(), which also makes it that call's keep-alive candidate."""
    n = getattr(_lib.load(), query)(*dims)
    return torch.empty(n, device=like.device, dtype=torch.float32) if n > 0 else None


def _nb(*ts):
    """HBM bytes of the given operands (None skipped): the algorithmic traffic of a launch."""
    return float(sum(t.numel() * t.element_size() for t in ts if t is not None))


def _conv_flops(N, Cin, Cout, KH, KW, Ho, Wo):
    # algorithmic MACs of the conv (also for its dgrad/wgrad): every output pixel x every tap
    return 2.0 * N * Cout * Cin * KH * KW * Ho * Wo


def _in_act(act):
    """Activation code of an InstanceNorm launch: the 16-bit modes take the A&S GELU (the MLP
    kernels' form); fp32 mode keeps the exact erf."""
    return ACT_GELU_FAST if act == "gelu" and _state["prec"] != "fp32" else ACT[act]


def nchw(t):
    """Return (tensor, batch_stride) with the per-sample [C,H,W] block dense (channel slices of
    a concat buffer qualify); otherwise make it contiguous."""
    if t.dim() != 4:
        raise ValueError("expected NCHW tensor, got %s" % (tuple(t.shape),))
    N, C, H, W = t.shape
    s = t.stride()
    if (s[3] == 1 and s[2] == W and s[1] == H * W) or t.numel() == 0:
        return t, (s[0] if N > 1 else C * H * W)
    t = t.contiguous()
    return t, C * H * W


def _empty(N, C, H, W, like):
    return torch.empty((N, C, H, W), device=like.device, dtype=torch.float32)


# Gradient-readiness hook (dsgan_hip.dist.GradBuckets): every Function calls _params_done() at
# the end of its backward with the parameters whose weight-grads it has just launched, so a
# bucket of the flat gradient can start its all-reduce while the rest of backward runs.
GRAD_READY = [None]


def _params_done(*ps):
    h = GRAD_READY[0]
    if h is not None:
        h([p for p in ps if p is not None])


def _grad_buf(p):
    """Accumulation target for a parameter's gradient, or None when it is frozen."""
    if p is None or not p.requires_grad:
        return None
    if p.grad is None:
        # FlatParams binds .grad up front; a free-standing parameter gets a zeroed buffer here.
        p.grad = torch.zeros_like(p)
    return p.grad


# ------------------------------------------------------------------------------------------
# raw launchers (no autograd)
# ------------------------------------------------------------------------------------------

def _pw_ok(mode, M, K, P, a_bs, b_bs, a, b):
    if not _is16():
        return False
    return bool(_lib.load().dsgan_pw_supported(mode, M, K, P, a_bs, b_bs, a, b))


def _tconv(X, xbs, Wt, bias, Y, ybs, gpre, gbs, nb, K, M, Hin, Win, Hout, Wout, stride, taps,
           Hdst, Wdst, os_, ph, pw, act, gact, xh=False):
    """Wt: fp32 tap-major weights (_wtrans) or their bf16 copy (_wtrans_bf16, mode 0); xh: X holds
    the 16-bit half type (dsgan_tconv_ws_xh, bf16 weights only)."""
    dh = (ctypes.c_int * len(taps))(*[t[0] for t in taps])
    dw = (ctypes.c_int * len(taps))(*[t[1] for t in taps])
    call("dsgan_tconv_ws_xh" if xh else "dsgan_tconv_ws", ptr(X), xbs, ptr(Wt), ptr(bias), ptr(Y), ybs, ptr(gpre),
         gbs, nb, K, M, Hin, Win, Hout, Wout, stride, len(taps), ctypes.cast(dh, ctypes.c_void_p),
         ctypes.cast(dw, ctypes.c_void_p), Hdst, Wdst, os_, ph, pw, ACT[act], ACT[gact], LRELU_SLOPE,
         *(() if xh else (int(Wt.dtype != torch.float32),)),
         *wsa(_ws("dsgan_tconv_workspace", nb, K, M, Hout, Wout, len(taps), like=X)), stream())


# Cached weight copies (tap-major transforms, 16-bit casts): an entry is valid while the
# parameter's storage pointer and the global weight generation are unchanged.  FlatAdam.step()
# bumps the generation (weights are updated in place by the fused Adam kernel, invisible to
# torch's version counters).
WEIGHT_GEN = [0]
_PARAM_GEN = {}
_WT_CACHE = {}     # conv weights in a kernel's layout (_wtrans, _wtrans_bf16, _vgg_wt)
_BF16_CACHE = {}   # plain 16-bit casts (bf16_weight)


class _Copy:
    """A cache entry: the copy of parameter ``w`` (at storage pointer ``ptr``), built at generation
    ``gen`` / ``w._version``.  ``mode``: the dsgan_wtrans_multi mode that rebuilds a 16-bit copy in
    place (0-2 tap-major, -1 plain cast), None for a copy that is rebuilt at its next use."""
    __slots__ = ("gen", "version", "w", "ptr", "copy", "mode")


def _wgen(w):
    return (WEIGHT_GEN[0], _PARAM_GEN.get(id(w), 0))


def _cached(cache, w, what, build, mode=None):
    """The copy of ``w`` that the tuple ``what`` names in ``cache``, from ``build()`` when there is
    none or the weight has changed since (generation, ``_version``, identity)."""
    key = (id(w), w.data_ptr(), tuple(w.shape)) + what
    ent = cache.get(key)
    gen = _wgen(w)
    if ent is not None and ent.gen == gen and ent.version == w._version and ent.w is w:
        return ent.copy
    ent = _Copy()
    ent.gen, ent.version, ent.w, ent.ptr, ent.copy, ent.mode = gen, w._version, w, w.data_ptr(), build(), mode
    if cache is _BF16_CACHE and len(cache) > 8192:
        cache.clear()
    cache[key] = ent
    return ent.copy


def bump_weight_generation(params=None):
    """Invalidate cached weight transforms: of ``params`` (the ones an optimizer just updated),
    or of every weight.  Frozen weights (VGG16) keep their bf16 / tap-major copies across steps.
    With ``params``, the 16-bit copies cached for them (bf16_weight, _wtrans_bf16) are rebuilt
    right away, in place, by one batched launch (dsgan_wtrans_multi) instead of one launch per
    copy at its next use."""
    if params is None:
        WEIGHT_GEN[0] += 1
    else:
        for p in params:
            _PARAM_GEN[id(p)] = _PARAM_GEN.get(id(p), 0) + 1
        _refresh_half_copies(params)
    if len(_WT_CACHE) > 8192:
        _WT_CACHE.clear()


def _refresh_half_copies(params):
    ids = {id(p) for p in params}
    todo = [e for cache in (_WT_CACHE, _BF16_CACHE) for e in cache.values()
            if id(e.w) in ids and e.mode is not None and e.ptr == e.w.data_ptr() and e.copy.dtype == half_dtype()]
    if not todo:
        return
    n = len(todo)
    src = (ctypes.c_void_p * n)(*[e.w.data_ptr() for e in todo])
    dst = (ctypes.c_void_p * n)(*[e.copy.data_ptr() for e in todo])
    desc = []
    for e in todo:
        w = e.w
        Co, Ci, KH, KW = (tuple(w.shape) + (1, 1, 1))[:4] if w.dim() < 4 else tuple(w.shape)
        if e.mode < 0:   # plain cast: any shape, as a flat run of numel elements
            Co, Ci, KH, KW = w.numel(), 1, 1, 1
        desc += [Co, Ci, KH, KW, e.mode]
    dsc = (ctypes.c_int * len(desc))(*desc)
    call("dsgan_wtrans_multi", ctypes.cast(src, ctypes.c_void_p), ctypes.cast(dst, ctypes.c_void_p),
         ctypes.cast(dsc, ctypes.c_void_p), n, stream())
    for e in todo:
        e.gen, e.version = _wgen(e.w), e.w._version


def _wtrans(w, mode, kh0=0, kw0=0, nth=0, ntw=0):
    """fp32 tap-major weights for tconv.hip, cached (rebuilt at the next use after an update).  The
    rebuild writes the entry's own buffer: a launch captured into a HIP graph while the entry was
    current (the D step's data-grads, whose copies the preceding G step rebuilt) keeps reading the
    buffer that later rebuilds refresh, instead of a copy no replay writes again."""
    what = (mode, kh0, kw0, nth, ntw)
    old = _WT_CACHE.get((id(w), w.data_ptr(), tuple(w.shape)) + what)
    out = old.copy if old is not None and old.w is w else None
    return _cached(_WT_CACHE, w, what, lambda: _wtrans_build(w, mode, kh0, kw0, nth, ntw, out))


def _wtrans_build(w, mode, kh0=0, kw0=0, nth=0, ntw=0, out=None):
    Co, Ci, KH, KW = w.shape
    taps = nth * ntw if mode == 2 else KH * KW
    wt = out if out is not None else torch.empty(taps * Co * Ci, device=w.device, dtype=torch.float32)
    call("dsgan_conv_wtrans", ptr(w), ptr(wt), Co, Ci, KH, KW, mode, kh0, kw0, nth, ntw, stream())
    return wt


def _wtrans_bf16(w, mode):
    """bf16 tap-major weights for pconv.hip / pconvt.hip (mode 0 forward, 1 stride-1 data-grad,
    2 stride-2 data-grad / ConvTranspose), cached."""
    def build():
        Co, Ci, KH, KW = w.shape
        wb = torch.empty(KH * KW * Co * Ci, device=w.device, dtype=half_dtype())
        call("dsgan_conv_wtrans_bf16", ptr(w), ptr(wb), Co, Ci, KH, KW, mode, stream())
        return wb
    return _cached(_WT_CACHE, w, (half_dtype(), mode), build, mode)


def bf16_weight(w):
    """bf16 copy of a parameter for the fused kernels, cached like _wtrans (same invalidation)."""
    def build():
        out = torch.empty(w.shape, device=w.device, dtype=half_dtype())
        call("dsgan_f32_to_bf16", ptr(w), ptr(out), w.numel(), stream())
        return out
    return _cached(_BF16_CACHE, w, (half_dtype(),), build, -1)


def _pw_ws(M, N, P, nb, like):
    """Split-K scratch of a pointwise weight-grad (dsgan_pw_wgrad_workspace), or None."""
    return _ws("dsgan_pw_wgrad_workspace", M, N, P, nb, like=like)


# Eligibility rules of the kernel families.  They take plain numbers -- pointers as integers, of
# which only the alignment is read -- so that the choice can be asked without a tensor.

def _pw_io_ok(K, P, xbs, ybs, x, y, pre=None, pbs=0):
    """dsgan_pw_fwd_io / dgrad_io alignment rules with fp32 activations (16-bit weight rows: K % 8)."""
    return (K % 8 == 0 and P % 128 == 0 and xbs % 8 == 0 and ybs % 8 == 0 and x % 16 == 0
            and y % 16 == 0 and (pre is None or (pbs % 4 == 0 and pre % 16 == 0)))


def _pwf_ok(mode, M, K, P, a_bs, b_bs, a, b):
    """fp32 operands (the MidMLKA 1x1 conv, or every 1x1 in the fp32 parity mode): pwf32.hip."""
    return _state["prec"] == "fp32" and bool(_lib.load().dsgan_pw_f32_supported(mode, M, K, P, a_bs, b_bs, a, b))


def _pws_ok(K, M, P, xbs, ybs, x, y):
    """1x1 contraction with <= 16 channels on one side for pwsmall.hip (16-byte rows)."""
    return ((K <= 16 or M <= 16) and x % 16 == 0 and y % 16 == 0
            and bool(_lib.load().dsgan_pw_small_supported(K, M, P, xbs, ybs)))


PGLAST = [True]   # the PatchGAN head on pglast.hip (off: the generic small-channel kernels; tests / A-B)


def _pglast_ok(Cout, Cin, KH, KW, stride, pad, H, W, w_dim, w_contig):
    """Conv(Cin -> 1, 4x4, stride 1, pad 1): the PatchGAN head (networks.py:567-568), pglast.hip."""
    return (PGLAST[0] and Cout == 1 and KH == 4 and KW == 4 and stride == 1 and pad == 1 and w_dim == 4
            and w_contig and bool(_lib.load().dsgan_pglast_supported(Cin, H, W)))


def _thin3_ok(M, H, W, bs_small, bs_big, p_small, p_big):
    """3x3 / s1 / p1 conv with <= 4 channels on one side at W % 256 == 0 (thin3.hip)."""
    return (p_small % 16 == 0 and p_big % 16 == 0
            and bool(_lib.load().dsgan_thin3_supported(M, H, W, bs_small, bs_big)))


def _pconv_ok(K, KH, KW, stride):
    return _is16() and bool(_lib.load().dsgan_pconv_supported(K, KH, KW, stride))


def _pconv(x, xbs, wb, b, y, ybs, N, K, M, H, W, Ho, Wo, KH, KW, stride, pad, act, gpre, gbs, gact, accumulate):
    call("dsgan_pconv_ws", ptr(x), xbs, ptr(wb), ptr(b), ptr(y), ybs, ptr(gpre), gbs, N, K, M, H, W, Ho, Wo, KH, KW,
         stride, pad, ACT[act], ACT[gact], LRELU_SLOPE, int(accumulate),
         *wsa(_ws("dsgan_pconv_workspace", N, K, M, Ho, Wo, like=x)), stream())


# Which kernel family a conv takes -- the main performance fact of a layer -- as functions of plain
# numbers and flags: shapes, batch strides, pointer values (alignment only), the weight's dim() and
# contiguity, the epilogue options present, and the module's state (the precision, PGLAST[0],
# WCONV_DB_FOLD).  They touch no tensor and launch nothing, so they answer on a machine without a
# GPU (tests/test_dispatch_cpu.py).  Each returns (family, form): the family is the name the
# timer records, the form tells the two launch forms of pwgemm_kernel ("io_ws": the cached 16-bit
# weight through dsgan_pw_{fwd,dgrad}_io_ws, "gemm": dsgan_pw_gemm) and of wconv_kernel ("db": with
# the bias grad folded in, "plain") apart and is None elsewhere.  The first rule that holds wins.

def conv_fwd_family(Cin, H, W, Cout, KH, KW, stride, pad, xbs, ybs, pbs, x_ptr, y_ptr, w_ptr, pre_ptr,
                    w_dim, w_contig, act, xact, accumulate):
    pw = KH == 1 and KW == 1 and stride == 1 and pad == 0
    if (KH == 3 and KW == 3 and stride == 1 and pad == 1 and act is None and pre_ptr is None and xact is None
            and w_contig and _thin3_ok(Cout, H, W, ybs, xbs, y_ptr, x_ptr)):
        return "thin3_kernel", None      # 3x3 into <= 4 channels at full resolution (the G head)
    if pw and pre_ptr is None and _pws_ok(Cin, Cout, H * W, xbs, ybs, x_ptr, y_ptr):
        return "pw_small_kernel", None   # 1x1 with <= 16 channels on one side (the 3/12-channel layers at 256^2)
    if (_pglast_ok(Cout, Cin, KH, KW, stride, pad, H, W, w_dim, w_contig) and act is None and pre_ptr is None
            and xact is None):
        return "pglast_kernel", None     # PatchGAN head 256 -> 1, 4x4 s1
    if Cout <= 8 and act is None and pre_ptr is None and xact is None:
        return "small_out_kernel", None  # few output channels (G head, PatchGAN last layer): direct conv
    if Cin * KH * KW <= 36 and Cout >= 16 and pre_ptr is None and xact is None and act in (None, "relu", "lrelu"):
        return "small_in_kernel", None   # few input taps into many channels (VGG conv1_1)
    if pw and _pw_ok(0, Cout, Cin, H * W, 0, xbs, w_ptr, x_ptr):
        io = xact is None and _pw_io_ok(Cin, H * W, xbs, ybs, x_ptr, y_ptr, pre_ptr, pbs)
        return "pwgemm_kernel", "io_ws" if io else "gemm"
    if pw and pre_ptr is None and xact is None and _pwf_ok(0, Cout, Cin, H * W, 0, xbs, w_ptr, x_ptr):
        return "pwf32_kernel", None
    if w_dim == 4 and pre_ptr is None and xact is None and _pconv_ok(Cin, KH, KW, stride):
        return "pconv_kernel", None
    if (_is16() and w_dim == 4 and (KH > 1 or KW > 1) and Cin % 32 == 0
            and pre_ptr is None and not accumulate and xact is None and KH * KW <= 16):
        return "tconv_kernel", None
    return "igemm_kernel", None


def conv_dgrad_family(Cin, H, W, Cout, KH, KW, stride, pad, Ho, Wo, dybs, dxbs, gbs, dy_ptr, dx_ptr, w_ptr,
                      gpre_ptr, w_dim, w_contig, act, has_bias, accumulate):
    pw = KH == 1 and KW == 1 and stride == 1 and pad == 0
    if (KH == 3 and KW == 3 and stride == 1 and pad == 1 and act is None and not has_bias and gpre_ptr is None
            and w_contig and _thin3_ok(Cout, H, W, dybs, dxbs, dy_ptr, dx_ptr)):
        return "thin3_kernel", None
    if (pw and act is None and not has_bias and _pws_ok(Cout, Cin, H * W, dybs, dxbs, dy_ptr, dx_ptr)
            and (gpre_ptr is None or (gbs % 4 == 0 and gpre_ptr % 16 == 0))):
        return "pw_small_kernel", None
    if (_pglast_ok(Cout, Cin, KH, KW, stride, pad, H, W, w_dim, w_contig) and act is None and not has_bias
            and gpre_ptr is None):
        return "pglast_kernel", None
    if Cin <= 8 and act is None and gpre_ptr is None and stride in (1, 2):
        return "small_out_kernel", None  # data-grad into a 3/6-channel tensor: direct transposed gather
    if (Cout * KH * KW <= 27 and KH * KW <= 9 and Cin >= 16 and act is None and gpre_ptr is None and stride == 1
            and not has_bias):
        return "small_in_kernel", None   # data-grad out of a 3-channel conv (G head)
    if pw and not has_bias and act is None and _pw_ok(1, Cin, Cout, H * W, 0, dybs, w_ptr, dy_ptr):
        io = gpre_ptr is None and Cin % 8 == 0 and _pw_io_ok(Cout, H * W, dybs, dxbs, dy_ptr, dx_ptr)
        return "pwgemm_kernel", "io_ws" if io else "gemm"
    if pw and not has_bias and act is None and _pwf_ok(1, Cin, Cout, H * W, 0, dybs, w_ptr, dy_ptr):
        return "pwf32_kernel", None
    if w_dim == 4 and stride == 1 and act is None and not has_bias and KH == KW and _pconv_ok(Cout, KH, KW, 1):
        return "pconv_kernel", None      # stride-1 data-grad = forward conv of dy with the flipped, transposed kernel
    if (_is16() and w_dim == 4 and stride == 2 and pad == 1 and KH == KW and act is None
            and H <= 2 * Ho and H > 2 * Ho - 2 and W <= 2 * Wo and W > 2 * Wo - 2 and W % 2 == 0 and dxbs % 2 == 0
            and (gpre_ptr is None or gbs % 2 == 0) and _lib.load().dsgan_pconvt_supported(Cout, KH, stride, pad)):
        return "pconvt_kernel", None     # stride-2 data-grad / ConvTranspose: all four output parities in one launch
    if (_is16() and w_dim == 4 and (KH > 1 or KW > 1) and Cout % 32 == 0
            and act is None and not accumulate and stride in (1, 2) and KH * KW <= 16):
        return "tconv_kernel", None
    return "igemm_kernel", None


def conv_wgrad_family(N, Cin, H, W, Cout, KH, KW, stride, pad, dybs, xbs, dy_ptr, x_ptr, w_dim, w_contig,
                      xact, has_db):
    pw = KH == 1 and KW == 1 and stride == 1 and pad == 0
    if (xact is None and KH == 3 and KW == 3 and stride == 1 and pad == 1 and w_contig
            and _thin3_ok(Cout, H, W, dybs, xbs, dy_ptr, x_ptr)):
        return "thin3_kernel", None
    if xact is None and w_contig and _pglast_ok(Cout, Cin, KH, KW, stride, pad, H, W, w_dim, w_contig):
        return "pglast_kernel", None
    if xact is None and KH * KW in (1, 9, 16) and (Cout <= 8 or (Cin <= 8 and KH * KW == 1)):
        return "wgrad_small_kernel", None
    if pw and _pw_ok(2, Cout, N * H * W, H * W, dybs, xbs, dy_ptr, x_ptr):
        return "pwgemm_kernel", "gemm"
    if pw and xact is None and _pwf_ok(2, Cout, N * H * W, H * W, dybs, xbs, dy_ptr, x_ptr):
        return "pwf32_kernel", None
    if (xact is None and _is16() and w_contig and pad == 1 and W % 4 == 0
            and xbs % 4 == 0 and x_ptr % 16 == 0 and _lib.load().dsgan_wconv_supported(Cin, KH, KW, stride)):
        # "db": the bias grad from the staged dy tiles (no channel-sum pass)
        return "wconv_kernel", "db" if has_db and WCONV_DB_FOLD else "plain"
    return "igemm_kernel", None


def conv_fwd_raw(x, w, b, stride, pad, act=None, out=None, pre=None, accumulate=False, xact=None):
    x, xbs = nchw(x)
    N, Cin, H, W = x.shape
    Cout, Cin_w, KH, KW = w.shape if w.dim() == 4 else (w.shape[0], w.shape[1], 1, 1)
    if Cin_w != Cin:
        raise ValueError("conv: input has %d channels, weight expects %d" % (Cin, Cin_w))
    Ho = (H + 2 * pad - KH) // stride + 1
    Wo = (W + 2 * pad - KW) // stride + 1
    y = out if out is not None else _empty(N, Cout, Ho, Wo, x)
    y, ybs = nchw(y)
    pbs = 0
    if pre is not None:
        pre, pbs = nchw(pre)
    fam, form = conv_fwd_family(Cin, H, W, Cout, KH, KW, stride, pad, xbs, ybs, pbs, x.data_ptr(), y.data_ptr(),
                                w.data_ptr(), None if pre is None else pre.data_ptr(), w.dim(), w.is_contiguous(),
                                act, xact, accumulate)
    with _timed(IGEMM_TIMER, _conv_flops(N, Cin, Cout, KH, KW, Ho, Wo), ("fwd", N, Cin, H, W, Cout, KH, stride), fam,
                _nb(x, w, b, y, pre) + (_nb(y) if accumulate else 0.0)):
        if fam == "thin3_kernel":     # row-strip fp32 stream
            call("dsgan_thin3_fwd", ptr(x), xbs, ptr(w), ptr(b), ptr(y), ybs, N, Cin, Cout, H, W, int(accumulate),
                 stream())
        elif fam == "pw_small_kernel":   # VALU stream
            call("dsgan_pw_small", ptr(x), xbs, ptr(w), Cin, 1, ptr(b), ptr(y), ybs, None, 0, N, Cin, Cout, H * W,
                 ACT[act], ACT[xact], 0, int(accumulate), LRELU_SLOPE, stream())
        elif fam == "pglast_kernel":     # channel chunks in LDS, partials summed in order
            call("dsgan_pglast_fwd", ptr(x), xbs, ptr(w), ptr(b), ptr(y), ybs, N, Cin, H, W, int(accumulate),
                 *wsa(_ws("dsgan_pglast_workspace", N, Cin, H, W, like=x)), stream())
        elif fam == "small_out_kernel":
            call("dsgan_conv_small_out", ptr(x), xbs, ptr(w), Cin * KH * KW, KH * KW, KW, 1, ptr(b), ptr(y), ybs,
                 N, Cin, Cout, H, W, Ho, Wo, KH, KW, stride, pad, 0, int(accumulate), stream())
        elif fam == "small_in_kernel":   # thread-per-pixel exact fp32 dot products
            call("dsgan_conv_small_in", ptr(x), xbs, ptr(w), Cin * KH * KW, KH * KW, KW, 1, ptr(b), ptr(y), ybs,
                 N, Cin, Cout, H, W, Ho, Wo, KH, KW, stride, pad, 0, ACT[act], LRELU_SLOPE, int(accumulate), stream())
        elif form == "io_ws":
            # the cached 16-bit weight copy instead of converting the fp32 weight tile in every
            # workgroup (the same RNE rounding: the same bits)
            call("dsgan_pw_fwd_io_ws", ptr(bf16_weight(w)), 1, ptr(x), xbs, 0, ptr(y), ybs, 0, ptr(pre), pbs, 0,
                 ptr(b), Cout, Cin, H * W, N, ACT[act], int(accumulate), LRELU_SLOPE,
                 *wsa(_ws("dsgan_pw_fd_workspace", 0, Cout, Cin, H * W, N, like=x)), stream())
        elif fam == "pwgemm_kernel":
            call("dsgan_pw_gemm", 0, ptr(w), 0, ptr(x), xbs, ptr(y), ybs, ptr(b), ptr(pre), pbs, None, 0,
                 Cout, N * H * W, Cin, H * W, N, ACT[act], 0, ACT[xact], int(accumulate), LRELU_SLOPE,
                 *wsa(_ws("dsgan_pw_fd_workspace", 0, Cout, Cin, H * W, N, like=x)), stream())
        elif fam == "pwf32_kernel":
            call("dsgan_pw_gemm_f32", 0, ptr(w), 0, ptr(x), xbs, ptr(y), ybs, ptr(b), None, 0, Cout, N * H * W, Cin,
                 H * W, N, ACT[act], 0, int(accumulate), LRELU_SLOPE, None, 0, stream())
        elif fam == "pconv_kernel":
            _pconv(x, xbs, _wtrans_bf16(w, 0), b, y, ybs, N, Cin, Cout, H, W, Ho, Wo, KH, KW, stride, pad, act,
                   None, 0, None, accumulate)
        elif fam == "tconv_kernel":
            wt = _wtrans_bf16(w, 0) if Cin % 8 == 0 else _wtrans(w, 0)
            taps = [(kh - pad, kw - pad) for kh in range(KH) for kw in range(KW)]
            _tconv(x, xbs, wt, b, y, ybs, None, 0, N, Cin, Cout, H, W, Ho, Wo, stride, taps, Ho, Wo, 1, 0, 0,
                   act, None)
        else:
            call("dsgan_conv_fwd", ptr(x), xbs, ptr(w), ptr(b), ptr(y), ybs, ptr(pre), pbs, N, Cin, H, W,
                 Cout, KH, KW, stride, pad, Ho, Wo, ACT[act], LRELU_SLOPE, int(accumulate), ACT[xact], _prec(),
                 stream())
    return y


def _tconv_dgrad(dy, dybs, w, bias, dx, dxbs, gpre, gbs, N, Cin, H, W, Cout, KH, KW, Ho, Wo, stride, pad, gact):
    """Tap-major data-grad: one launch at stride 1 (flipped kernel), one per output parity at stride 2."""
    if stride == 1:
        pp, qq = KH - 1 - pad, KW - 1 - pad
        taps = [(kh - pp, kw - qq) for kh in range(KH) for kw in range(KW)]
        _tconv(dy, dybs, _wtrans(w, 1), bias, dx, dxbs, gpre, gbs, N, Cout, Cin, Ho, Wo, H, W, 1, taps, H, W, 1,
               0, 0, None, gact)
        return
    for ph in range(2):
        for pw_ in range(2):
            kh0, kw0 = (ph + pad) & 1, (pw_ + pad) & 1
            nth, ntw = (KH - kh0 + 1) // 2, (KW - kw0 + 1) // 2
            Hc, Wc = (H - ph + 1) // 2, (W - pw_ + 1) // 2
            if Hc <= 0 or Wc <= 0:
                continue
            ch, cw = (ph + pad - kh0) // 2, (pw_ + pad - kw0) // 2
            wt = _wtrans(w, 2, kh0, kw0, nth, ntw)
            taps = [(ch - (nth - 1) + a, cw - (ntw - 1) + c) for a in range(nth) for c in range(ntw)]
            _tconv(dy, dybs, wt, bias, dx, dxbs, gpre, gbs, N, Cout, Cin, Ho, Wo, Hc, Wc, 1, taps,
                   H, W, 2, ph, pw_, None, gact)


def conv_dgrad_raw(dy, w, x_shape, stride, pad, bias=None, act=None, gpre=None, gact=None,
                   out=None, accumulate=False):
    """dx (N,Cin,H,W) of a conv with weight w [Cout,Cin,KH,KW]; also a ConvTranspose forward."""
    dy, dybs = nchw(dy)
    N, Cin, H, W = x_shape
    Cout, _, KH, KW = w.shape if w.dim() == 4 else (w.shape[0], w.shape[1], 1, 1)
    Ho, Wo = dy.shape[2], dy.shape[3]
    dx = out if out is not None else torch.empty((N, Cin, H, W), device=dy.device, dtype=torch.float32)
    dx, dxbs = nchw(dx)
    gbs = 0
    if gpre is not None:
        gpre, gbs = nchw(gpre)
    fam, form = conv_dgrad_family(Cin, H, W, Cout, KH, KW, stride, pad, Ho, Wo, dybs, dxbs, gbs, dy.data_ptr(),
                                  dx.data_ptr(), w.data_ptr(), None if gpre is None else gpre.data_ptr(), w.dim(),
                                  w.is_contiguous(), act, bias is not None, accumulate)
    with _timed(IGEMM_TIMER, _conv_flops(N, Cin, Cout, KH, KW, Ho, Wo), ("dgrad", N, Cin, H, W, Cout, KH, stride), fam,
                _nb(dy, w, bias, dx, gpre) + (_nb(dx) if accumulate else 0.0)):
        if fam == "thin3_kernel":
            call("dsgan_thin3_dgrad", ptr(dy), dybs, ptr(w), ptr(dx), dxbs, N, Cin, Cout, H, W, int(accumulate),
                 stream())
        elif fam == "pw_small_kernel":
            call("dsgan_pw_small", ptr(dy), dybs, ptr(w), 1, Cin, None, ptr(dx), dxbs, ptr(gpre), gbs, N, Cout, Cin,
                 H * W, 0, 0, ACT[gact], int(accumulate), LRELU_SLOPE, stream())
        elif fam == "pglast_kernel":
            call("dsgan_pglast_dgrad", ptr(dy), dybs, ptr(w), ptr(dx), dxbs, N, Cin, H, W, int(accumulate), stream())
        elif fam == "small_out_kernel":   # w(m=ci, k=co, kh, kw)
            call("dsgan_conv_small_out", ptr(dy), dybs, ptr(w), KH * KW, Cin * KH * KW, KW, 1, ptr(bias),
                 ptr(dx), dxbs, N, Cout, Cin, Ho, Wo, H, W, KH, KW, stride, pad, 1, int(accumulate), stream())
        elif fam == "small_in_kernel":    # stride-1 transposed gather, w(m=ci, k=co, kh, kw)
            call("dsgan_conv_small_in", ptr(dy), dybs, ptr(w), KH * KW, Cin * KH * KW, KW, 1, None, ptr(dx), dxbs,
                 N, Cout, Cin, Ho, Wo, H, W, KH, KW, 1, pad, 1, 0, LRELU_SLOPE, int(accumulate), stream())
        elif form == "io_ws":
            call("dsgan_pw_dgrad_io_ws", ptr(bf16_weight(w)), 1, ptr(dy), dybs, 0, ptr(dx), dxbs, 0, None, 0, Cin,
                 Cout, H * W, N, int(accumulate),
                 *wsa(_ws("dsgan_pw_fd_workspace", 1, Cin, Cout, H * W, N, like=dy)), stream())
        elif fam == "pwgemm_kernel":
            call("dsgan_pw_gemm", 1, ptr(w), 0, ptr(dy), dybs, ptr(dx), dxbs, None, None, 0, ptr(gpre), gbs,
                 Cin, N * H * W, Cout, H * W, N, 0, ACT[gact], 0, int(accumulate), LRELU_SLOPE,
                 *wsa(_ws("dsgan_pw_fd_workspace", 1, Cin, Cout, H * W, N, like=dy)), stream())
        elif fam == "pwf32_kernel":
            call("dsgan_pw_gemm_f32", 1, ptr(w), 0, ptr(dy), dybs, ptr(dx), dxbs, None, ptr(gpre), gbs, Cin,
                 N * H * W, Cout, H * W, N, 0, ACT[gact], int(accumulate), LRELU_SLOPE, None, 0, stream())
        elif fam == "pconv_kernel":
            _pconv(dy, dybs, _wtrans_bf16(w, 1), None, dx, dxbs, N, Cout, Cin, Ho, Wo, H, W, KH, KW, 1,
                   KH - 1 - pad, None, gpre, gbs, gact, accumulate)
        elif fam == "pconvt_kernel":
            call("dsgan_pconvt", ptr(dy), dybs, ptr(_wtrans_bf16(w, 2)), ptr(bias), ptr(dx), dxbs, ptr(gpre), gbs, N,
                 Cout, Cin, Ho, Wo, H, W, KH, stride, pad, ACT[gact], LRELU_SLOPE, int(accumulate), stream())
        elif fam == "tconv_kernel":
            _tconv_dgrad(dy, dybs, w, bias, dx, dxbs, gpre, gbs, N, Cin, H, W, Cout, KH, KW, Ho, Wo, stride, pad, gact)
        else:
            call("dsgan_conv_dgrad", ptr(dy), dybs, ptr(w), ptr(bias), ptr(dx), dxbs, None, 0, ptr(gpre), gbs,
                 ACT[gact], N, Cin, H, W, Cout, KH, KW, stride, pad, Ho, Wo, ACT[act], LRELU_SLOPE,
                 int(accumulate), _prec(), stream())
    return dx


def conv_wgrad_raw(dy, x, dw, stride, pad, xact=None, db=None):
    """dw += conv weight-grad; db (optional) += the bias grad sum(dy) when the kernel taken can fold
    it into the weight-grad (the bf16 pointwise path).  Returns True when db was accumulated."""
    dy, dybs = nchw(dy)
    x, xbs = nchw(x)
    N, Cin, H, W = x.shape
    Cout, Ho, Wo = dy.shape[1], dy.shape[2], dy.shape[3]
    KH, KW = (dw.shape[2], dw.shape[3]) if dw.dim() == 4 else (1, 1)
    fam, form = conv_wgrad_family(N, Cin, H, W, Cout, KH, KW, stride, pad, dybs, xbs, dy.data_ptr(), x.data_ptr(),
                                  dw.dim(), dw.is_contiguous(), xact, db is not None)
    # the families whose kernel also sums the bias grad
    did_db = db is not None and (fam in ("pglast_kernel", "pwgemm_kernel", "pwf32_kernel") or form == "db")
    with _timed(IGEMM_TIMER, _conv_flops(N, Cin, Cout, KH, KW, Ho, Wo), ("wgrad", N, Cin, H, W, Cout, KH, stride), fam,
                _nb(dy, x, dw)):
        if fam == "thin3_kernel":
            call("dsgan_thin3_wgrad", ptr(dy), dybs, ptr(x), xbs, ptr(dw),
                 *wsa(_ws("dsgan_thin3_wgrad_workspace", N, Cin, Cout, H, W, like=dy)), N, Cin, Cout, H, W, stream())
        elif fam == "pglast_kernel":
            call("dsgan_pglast_wgrad", ptr(dy), dybs, ptr(x), xbs, ptr(dw), ptr(db), N, Cin, H, W,
                 *wsa(_ws("dsgan_pglast_workspace", N, Cin, H, W, like=dy)), stream())
        elif fam == "wgrad_small_kernel":
            call("dsgan_conv_wgrad_small", ptr(dy), dybs, ptr(x), xbs, ptr(dw), N, Cin, H, W, Cout, KH, KW,
                 stride, pad, Ho, Wo,
                 *wsa(_ws("dsgan_conv_wgrad_small_workspace", N, Cin, Cout, KH, KW, Ho, Wo, like=dy)), stream())
        elif fam == "pwgemm_kernel":
            call("dsgan_pw_gemm", 2, ptr(dy), dybs, ptr(x), xbs, ptr(dw), 0, ptr(db), None, 0, None, 0,
                 Cout, Cin, N * H * W, H * W, N, 0, 0, ACT[xact], 0, LRELU_SLOPE, *wsa(_pw_ws(Cout, Cin, H * W, N, dy)),
                 stream())
        elif fam == "pwf32_kernel":
            call("dsgan_pw_gemm_f32", 2, ptr(dy), dybs, ptr(x), xbs, ptr(dw), 0, ptr(db), None, 0, Cout, Cin, N * H * W,
                 H * W, N, 0, 0, 0, LRELU_SLOPE,
                 *wsa(_ws("dsgan_pw_f32_wgrad_workspace", Cout, Cin, H * W, N, like=dy)), stream())
        elif fam == "wconv_kernel":
            ws = _ws("dsgan_wconv_workspace", N, Cin, Cout, Ho, Wo, KH, KW, like=dy)
            if form == "db":
                call("dsgan_wconv_db", ptr(dy), dybs, ptr(x), xbs, ptr(dw), ptr(db), *wsa(ws), N, Cin, Cout, H, W, Ho,
                     Wo, KH, KW, stride, pad, stream())
            else:
                call("dsgan_wconv", ptr(dy), dybs, ptr(x), xbs, ptr(dw), *wsa(ws), N, Cin, Cout, H, W, Ho, Wo, KH, KW,
                     stride, pad, stream())
        else:
            call("dsgan_conv_wgrad", ptr(dy), dybs, ptr(x), xbs, ptr(dw), N, Cin, H, W, Cout, KH, KW,
                 stride, pad, Ho, Wo, ACT[xact], _prec(),
                 *wsa(_ws("dsgan_conv_wgrad_workspace", N, Cin, Cout, KH, KW, Ho, Wo, _prec(), like=dy)), stream())
    return did_db


def channel_sum_raw(dy, out):
    dy, dybs = nchw(dy)
    N, C, H, W = dy.shape
    ws = torch.empty(N * C, device=dy.device, dtype=torch.float32)
    call("dsgan_channel_sum", ptr(dy), dybs, ptr(out), N, C, H * W, *wsa(ws), stream())


def act_bwd_raw(dy, pre, act, out=None):
    dy = dy.contiguous()
    pre = pre.contiguous()
    out = out if out is not None else torch.empty_like(dy)
    call("dsgan_act_bwd", ptr(dy), ptr(pre), ptr(out), dy.numel(), ACT[act], LRELU_SLOPE, 0, stream())
    return out


def fill_(t, v):
    if not t.is_contiguous():
        raise ValueError("fill_: contiguous tensor required")
    call("dsgan_fill", ptr(t), float(v), t.numel(), stream())
    return t


def zeros(shape, like):
    return fill_(torch.empty(shape, device=like.device, dtype=torch.float32), 0.0)


def fingerprint(t):
    """The 64-bit fingerprint (a python int in [0, 2^64)) of a contiguous device tensor of a 4-byte
    element type, over its bit patterns (dsgan_fingerprint: -0.0 differs from 0.0, NaN payloads
    count).  Synchronises; meant for checkpoint save / load time, not for the step."""
    if not t.is_contiguous() or t.element_size() != 4:
        raise ValueError("fingerprint: a contiguous tensor of a 4-byte element type required, got %s %s"
                         % (t.dtype, "contiguous" if t.is_contiguous() else "strided"))
    part = torch.empty(int(_lib.load().dsgan_fingerprint_parts()) + 1, device=t.device, dtype=torch.int64)
    call("dsgan_fingerprint", ptr(t), t.numel(), ptr(part), part.numel() - 1, ptr(part[-1:]), stream())
    return int(part[-1].item()) & (2 ** 64 - 1)


def copy_multi(pairs):
    """dst <- src for a list of (dst, src) dense fp32 tensors of equal size, one launch per 32 pairs."""
    if not pairs:
        return
    n = pairs[0][0].numel()
    for d, s in pairs:
        if d.numel() != n or s.numel() != n or not d.is_contiguous() or not s.is_contiguous() \
                or d.dtype != torch.float32 or s.dtype != torch.float32:
            raise ValueError("copy_multi: dense fp32 tensors of one size required")
    srcs = (ctypes.c_void_p * len(pairs))(*[ptr(s) for _, s in pairs])
    dsts = (ctypes.c_void_p * len(pairs))(*[ptr(d) for d, _ in pairs])
    call("dsgan_copy_multi", ctypes.cast(srcs, ctypes.c_void_p), ctypes.cast(dsts, ctypes.c_void_p), len(pairs), n,
         stream())


class CatSlot:
    """The buffer of a channel concatenation cat(head, tail) [N, Ch+Ct, H, W], allocated before
    either half exists.  The tail's producer writes straight into ``tail()`` (a Block output that
    is a decoder skip, MixConvNeXtML.py:229-236), and the node that forms the concatenation
    (ConvTNormFn / InstanceNormCatFn, upSample :61-66) finds the tail already in place and writes
    only the head: the skip is never copied.  ``tail()`` / ``whole()`` alias the buffer's storage
    without being autograd views of it (no kernel writes through torch in-place ops)."""

    def __init__(self, N, Ch, Ct, H, W, like):
        self.buf = _empty(N, Ch + Ct, H, W, like)
        self.Ch, self.Ct = Ch, Ct

    def _alias(self, c0, C):
        b = self.buf
        N, _, H, W = b.shape
        return torch.empty(0, device=b.device, dtype=b.dtype).set_(
            b.untyped_storage(), b.storage_offset() + c0 * H * W, (N, C, H, W), b.stride())

    def tail(self):
        return self._alias(self.Ch, self.Ct)

    def whole(self):
        return self._alias(0, self.Ch + self.Ct)

    def holds(self, t, Ch):
        """t is this slot's tail (behind a head of Ch channels)."""
        b = self.buf
        N, _, H, W = b.shape
        return (t is not None and Ch == self.Ch and t.dim() == 4 and t.dtype == b.dtype and t.device == b.device
                and tuple(t.shape) == (N, self.Ct, H, W) and tuple(t.stride()) == tuple(b.stride())
                and t.data_ptr() == b.data_ptr() + self.Ch * H * W * b.element_size())


def copy_into(dst, src):
    """dst[n] <- src[n] for per-sample dense blocks (used for channel concatenation)."""
    src, sbs = nchw(src)
    dst4, dbs = nchw(dst)
    if dst4.data_ptr() != dst.data_ptr():
        raise ValueError("copy_into: destination must be per-sample dense")
    N = src.shape[0]
    E = src.shape[1] * src.shape[2] * src.shape[3]
    call("dsgan_copy_strided", ptr(src), sbs, ptr(dst), dbs, N, E, stream())


# ------------------------------------------------------------------------------------------
# Shared activations: one gradient buffer per tensor with several consumers.
#
# autograd sums the input-grads of a tensor's consumers with one torch add per extra consumer
# (2 reads + 1 write of the whole tensor each).  ``share(x)`` returns an alias of x carrying a
# _GradBox; consumer Functions see the box on their input and, in backward, either hand their
# freshly computed grad to the box (the first one is adopted as the buffer, no copy) or let the
# kernel accumulate straight into the buffer (maxpool / depthwise / GEMM data-grads have an
# accumulate epilogue).  ShareFn's backward -- run by autograd after every consumer -- returns
# the buffer.  A tensor that may also be referenced elsewhere (a grad autograd handed us) is
# only borrowed, never accumulated into in place.
# ------------------------------------------------------------------------------------------

class _GradBox:
    # outer: the box of the tensor this one aliases (share of a shared tensor, e.g. a Block's input
    # P_i = share(maxpool(R_i))); merged: this box accumulates straight into outer's buffer
    __slots__ = ("buf", "owned", "outer", "merged")

    def __init__(self):
        self.buf, self.owned, self.outer, self.merged = None, False, None, False


def _box(t):
    return getattr(t, "_dsg_box", None)


def _add_n_raw(out, ts):
    ts4 = [nchw(t) for t in ts]
    o4, obs = nchw(out)
    N, C, H, W = o4.shape
    arr = (ctypes.c_void_p * len(ts4))(*[t.data_ptr() for t, _ in ts4])
    bss = (ctypes.c_long * len(ts4))(*[bs for _, bs in ts4])
    call("dsgan_add_n", ctypes.cast(arr, ctypes.c_void_p), ctypes.cast(bss, ctypes.c_void_p), len(ts4), ptr(o4),
         obs, N, C * H * W, stream())


def _acc_target(box):
    """(buffer, True) when a kernel may accumulate its grad straight into the box.  An empty box
    whose outer box already owns a buffer merges into it: its consumers accumulate into the outer
    buffer in-kernel, instead of filling a buffer of their own that ShareFn then adds to the outer
    one (one add of the whole tensor per nested share)."""
    if box is None:
        return None, False
    if box.buf is None and box.outer is not None:
        ob, _ = _acc_target(box.outer)
        if ob is not None:
            box.buf, box.owned, box.merged = ob, True, True
    if box.buf is not None and box.owned:
        return box.buf, True
    return None, False


def _give(box, t, adopt=True):
    """Route a consumer's input-grad t: returns t itself when the input is not shared."""
    if box is None or t is None:
        return t
    if box.buf is None:
        box.buf, box.owned = t, adopt
    elif box.owned:
        _add_n_raw(box.buf, [box.buf, t])
    else:
        nb = _empty(*t.shape, t)
        _add_n_raw(nb, [box.buf, t])
        box.buf, box.owned = nb, True
    return None


class ShareFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, box):
        ctx.set_materialize_grads(False)
        ctx.box, ctx.outer = box, _box(x)
        box.outer = ctx.outer
        return x.view_as(x)

    @staticmethod
    def backward(ctx, g):
        box = ctx.box
        buf, own, merged = box.buf, box.owned, box.merged
        box.buf, box.merged = None, False
        if g is not None:
            if buf is None:
                buf, own = g, False
            elif own:
                _add_n_raw(buf, [buf, g])
            else:
                nb = _empty(*g.shape, g)
                _add_n_raw(nb, [buf, g])
                buf, own = nb, True
        if merged:
            return None, None   # every grad already sits in the outer box's buffer
        if ctx.outer is not None:
            _give(ctx.outer, buf, adopt=own)
            return None, None
        return buf, None


def share(x):
    """Alias of x whose consumers accumulate into one gradient buffer (see above)."""
    box = _GradBox()
    y = ShareFn.apply(x, box)
    y._dsg_box = box
    return y


# ------------------------------------------------------------------------------------------
# Conv2d (+bias, +relu/lrelu):  VGG 3x3, PatchGAN 4x4, G head 3x3, 1x1 convs
# ------------------------------------------------------------------------------------------

class Conv2dFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, w, b, stride, pad, act):
        y = conv_fwd_raw(x, w, b, stride, pad, act)
        ctx.prec = _state["prec"]
        ctx.stride, ctx.pad, ctx.act = stride, pad, act
        ctx.x_shape = tuple(x.shape)
        ctx.save_for_backward(x, w, b, y if act in ("relu", "lrelu") else None)
        ctx.w_ref, ctx.b_ref = w, b
        ctx.box = _box(x)
        return y

    @staticmethod
    def backward(ctx, dy):
        with precision(ctx.prec):
            return Conv2dFn._backward(ctx, dy)

    @staticmethod
    def _backward(ctx, dy):
        x, w, b, y = ctx.saved_tensors
        if ctx.act in ("relu", "lrelu"):
            dy = act_bwd_raw(dy, y, ctx.act)  # sign(y) == sign(pre) for relu/lrelu
        dx = None
        if ctx.needs_input_grad[0]:
            out, acc = _acc_target(ctx.box)
            dx = conv_dgrad_raw(dy, w, ctx.x_shape, ctx.stride, ctx.pad, out=out, accumulate=acc)
            dx = None if acc else _give(ctx.box, dx)
        gw = _grad_buf(ctx.w_ref) if ctx.needs_input_grad[1] else None
        gb = _grad_buf(ctx.b_ref) if (b is not None and ctx.needs_input_grad[2]) else None
        if gw is not None and conv_wgrad_raw(dy, x, gw, ctx.stride, ctx.pad, db=gb):
            gb = None
        if gb is not None:
            channel_sum_raw(dy, gb)
        _params_done(ctx.w_ref, ctx.b_ref)
        return dx, None, None, None, None, None


# NLayerDiscriminator layer 0 (networks.py:543-545) on the stem kernels (pgstem.hip); off routes it
# through the generic conv + LeakyReLU backward + bias channel sum (tests, A/B)
PGSTEM = [True]


def _pgstem_ok(x, w, stride, pad, act):
    if not PGSTEM[0] or act != "lrelu" or stride != 2 or pad != 1 or w.dim() != 4 or tuple(w.shape[2:]) != (4, 4):
        return False
    if x.dim() != 4 or not x.is_cuda or not w.is_contiguous() or w.shape[1] != x.shape[1]:
        return False
    N, Cin, H, W = x.shape
    return bool(_lib.load().dsgan_pgstem_supported(Cin, w.shape[0], H, W))


class PatchStemFn(torch.autograd.Function):
    """Conv2d(Cin, ndf, 4, 2, 1) + bias + LeakyReLU(0.2, True), the PatchGAN stem: one kernel per
    direction (dsgan_pgstem_*), exact fp32 in every precision mode.  The backward differentiates
    the LeakyReLU through its saved output, as the reference's in-place activation does."""

    @staticmethod
    def forward(ctx, x, w, b):
        ctx.box = _box(x)
        x, xbs = nchw(x)
        if xbs % 4 or x.data_ptr() % 16:
            x, xbs = x.contiguous(), x[0].numel()
        N, Cin, H, W = x.shape
        Cout = w.shape[0]
        y = _empty(N, Cout, H // 2, W // 2, x)
        with _timed(IGEMM_TIMER, _conv_flops(N, Cin, Cout, 4, 4, H // 2, W // 2), ("fwd", N, Cin, H, W, Cout, 4, 2),
                    "pgstem_kernel", _nb(x, w, b, y)):
            call("dsgan_pgstem_fwd", ptr(x), xbs, ptr(w), ptr(b), ptr(y), y[0].numel(), N, Cin, Cout, H, W,
                 LRELU_SLOPE, stream())
        ctx.save_for_backward(x, w, b, y)
        ctx.xbs = xbs
        ctx.w_ref, ctx.b_ref = w, b
        return y

    @staticmethod
    def backward(ctx, dy):
        x, w, b, y = ctx.saved_tensors
        dy, dybs = nchw(dy)
        if dybs % 4 or dy.data_ptr() % 16:
            dy, dybs = dy.contiguous(), dy[0].numel()
        N, Cin, H, W = x.shape
        Cout = w.shape[0]
        flops = _conv_flops(N, Cin, Cout, 4, 4, H // 2, W // 2)
        dx = None
        if ctx.needs_input_grad[0]:
            out, acc = _acc_target(ctx.box)
            dx = out if out is not None else _empty(N, Cin, H, W, dy)
            dx4, dxbs = nchw(dx)
            if dx4.data_ptr() != dx.data_ptr():
                raise RuntimeError("PatchStemFn: accumulation target is not NCHW-dense")
            with _timed(IGEMM_TIMER, flops, ("dgrad", N, Cin, H, W, Cout, 4, 2), "pgstem_kernel",
                        _nb(dy, y, w, dx) + (_nb(dx) if acc else 0.0)):
                call("dsgan_pgstem_dgrad", ptr(dy), dybs, ptr(y), y[0].numel(), ptr(w), ptr(dx), dxbs, N, Cin, Cout,
                     H, W, LRELU_SLOPE, int(acc), stream())
            dx = None if acc else _give(ctx.box, dx)
        gw = _grad_buf(ctx.w_ref) if ctx.needs_input_grad[1] else None
        gb = _grad_buf(ctx.b_ref) if (b is not None and ctx.needs_input_grad[2]) else None
        if gw is not None or gb is not None:
            # a frozen weight with a live bias still runs the weight-grad kernel (into scratch)
            dwt = gw if gw is not None else _keep(torch.zeros_like(w))
            with _timed(IGEMM_TIMER, flops, ("wgrad", N, Cin, H, W, Cout, 4, 2), "pgstem_kernel", _nb(dy, y, x, dwt)):
                call("dsgan_pgstem_wgrad", ptr(dy), dybs, ptr(y), y[0].numel(), ptr(x), ctx.xbs, ptr(dwt), ptr(gb), N,
                     Cin, Cout, H, W, LRELU_SLOPE,
                     *wsa(_ws("dsgan_pgstem_wgrad_workspace", N, Cin, Cout, H, W, like=dy)), stream())
        _params_done(ctx.w_ref, ctx.b_ref)
        return dx, None, None


def conv2d(x, w, b=None, stride=1, pad=0, act=None):
    """w may be OIHW or a Linear [out, in] weight (== 1x1 conv); pass the Parameter itself so its
    gradient lands in param.grad."""
    if _pgstem_ok(x, w, stride, pad, act):
        return PatchStemFn.apply(x, w, b)
    return Conv2dFn.apply(x, w, b, stride, pad, act)


# ------------------------------------------------------------------------------------------
# ConvTranspose2d(k3, s2, p1, op1) (+bias): forward = conv data-grad, backward = conv forward
# ------------------------------------------------------------------------------------------

class ConvT3s2Fn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, w, b):
        N, Ci, Hi, Wi = x.shape
        Co = w.shape[1]
        y = conv_dgrad_raw(x, w, (N, Co, 2 * Hi, 2 * Wi), 2, 1, bias=b)
        ctx.prec = _state["prec"]
        ctx.save_for_backward(x, w, b)
        ctx.w_ref, ctx.b_ref = w, b
        ctx.box = _box(x)
        return y

    @staticmethod
    def backward(ctx, dy):
        with precision(ctx.prec):
            return ConvT3s2Fn._backward(ctx, dy)

    @staticmethod
    def _backward(ctx, dy):
        x, w, b = ctx.saved_tensors
        dx = conv_fwd_raw(dy, w, None, 2, 1) if ctx.needs_input_grad[0] else None
        gw = _grad_buf(ctx.w_ref) if ctx.needs_input_grad[1] else None
        if gw is not None:
            conv_wgrad_raw(x, dy, gw, 2, 1)
        gb = _grad_buf(ctx.b_ref) if (b is not None and ctx.needs_input_grad[2]) else None
        if gb is not None:
            channel_sum_raw(dy, gb)
        _params_done(ctx.w_ref, ctx.b_ref)
        return _give(ctx.box, dx), None, None


def conv_transpose3s2(x, w, b):
    return ConvT3s2Fn.apply(x, w, b)


# ------------------------------------------------------------------------------------------
# ConvNeXt pointwise MLP + shortcut (Block.forward tail, MixConvNeXtML.py:236-242):
#   out = Ws x + W2 gelu(W1 h + b1) + b2
# backward: the dgrad of W2 multiplies by gelu'(z) in its epilogue (no standalone GELU pass).
# ------------------------------------------------------------------------------------------

def _mlp_tile(C, P, HW, x):
    """Pixels per b1-grad partial row of the fused MLP kernels (mlp.hip), 0 if unsupported."""
    if not _is16() or x.data_ptr() % 16:
        return 0
    return int(_lib.load().dsgan_mlp_supported(C, P, HW))


# The fused block tail takes the block's 1x1 shortcut into its forward kernel (dsgan_mlp_fwd_sc): one
# launch, and out is written once instead of written, re-read and re-written.  (=0: shortcut GEMM,
# then dsgan_mlp_fwd accumulating on it, for A/B runs)
MLP_FOLD_SC = [os.environ.get("DSGAN_MLP_FOLD_SC", "1") != "0"]


def _mlp_flops(N, C, P, HW):
    # algorithmic MACs of the two Linear layers (fwd; each of dgrad/wgrad is the same count)
    return 2.0 * N * HW * (4 * C * C + 4 * C * P)


class PwMlpFn(torch.autograd.Function):
    """Block tail: out = Ws x + W2 gelu(W1 h + b1) + b2, h = IN(d) when ``norm`` (the block's
    InstanceNorm, MixConvNeXtML.py:221, folded into this node so that h never needs an fp32 copy).

    In bf16 mode h is stored bf16 (dsgan_instnorm_fwd_bf16): its only readers are bf16-operand
    MFMA GEMMs that round it to bf16 on load anyway, so this halves its bytes and changes no bit.
      * fused shapes (mlp.hip): forward out = Ws x + W2 gelu(W1 h + b1) + b2 in one kernel
        (dsgan_mlp_fwd_sc; MLP_FOLD_SC off or a misaligned x: out = Ws x by pwgemm, then
        dsgan_mlp_fwd accumulating on it) -- z is never stored; backward recomputes z and writes
        only bf16 gelu(z) and dz for the two weight-grads.
      * other bf16 shapes with HW % 128 == 0: pwconv1 evaluates GELU once and writes g = gelu(z) and
        gp = gelu'(z), both bf16; backward writes dz = (W2^T dy) * gp in bf16 (again exactly what
        its two GEMM readers would round to) with the b1 grad summed from the fp32 values in the
        same epilogue.
      * otherwise (fp32 parity mode, tiny shapes) only the pre-GELU hidden z [N,4C,H,W] (fp32) is
        materialised: pwconv2 and its weight-grad read gelu(z) through the GEMM's
        activation-on-load, and the data-grad of pwconv2 multiplies by gelu'(z) in its epilogue."""

    @staticmethod
    def forward(ctx, h, x, w1, b1, w2, b2, ws, norm=False, slot=None, acc=None):
        N, C, H, W = h.shape
        P, HW, C4 = w2.shape[0], H * W, 4 * C
        # out: the slot's tail when the block output is a decoder skip (written in place), or acc
        # itself when the block output is summed into acc (out = acc + block; the first kernel
        # accumulates, acc is returned dirty)
        if acc is not None:
            if (slot is not None or tuple(acc.shape) != (N, P, H, W) or acc.dtype != torch.float32
                    or not acc.is_contiguous()):
                raise ValueError("pw_mlp: acc must be a dense fp32 [%d,%d,%d,%d] tensor (no slot)" % (N, P, H, W))
            ctx.mark_dirty(acc)
        ctx.box_acc = _box(acc) if acc is not None else None
        out0 = slot.tail() if slot is not None else acc
        acc1 = acc is not None
        obs = nchw(out0)[1] if out0 is not None else P * HW
        ctx.refs = (w1, b1, w2, b2, ws)
        ctx.prec = _state["prec"]
        ctx.box_h, ctx.box_x = _box(h), _box(x)
        h, hbs = nchw(h)
        tile = _mlp_tile(C, P, HW, x)
        bigg = (not tile and _is16() and HW % 128 == 0 and C % 8 == 0
                and (norm or h.data_ptr() % 16 == 0))
        ctx.nrm = None
        if norm:
            d, dbs = h, hbs
            if (tile or bigg) and d.data_ptr() % 16 == 0 and dbs % 4 == 0 and HW % 4 == 0:
                mean = torch.empty(N * C, device=d.device, dtype=torch.float32)
                rstd = torch.empty(N * C, device=d.device, dtype=torch.float32)
                h = torch.empty((N, C, H, W), device=d.device, dtype=half_dtype())
                with _timed(AUX_TIMER, 0.0, ("in_fwd_bf16", N, C, H, W), "instnorm", _nb(d, h)):
                    call("dsgan_instnorm_fwd_bf16", ptr(d), dbs, ptr(h), C * HW, ptr(mean), ptr(rstd), N, C, HW,
                         IN_EPS, stream())
            else:
                h, mean, rstd = instnorm_raw(d)
                tile = tile if h.data_ptr() % 16 == 0 else 0
            hbs = C * HW
            ctx.nrm = (d, mean, rstd)
        elif h.data_ptr() % 16:
            tile = 0
        hb = int(h.dtype != torch.float32)
        ctx.hb = hb
        ctx.tile = tile
        if tile:
            # the shortcut folded into the kernel, or the shortcut GEMM and the kernel accumulating on it
            fold = False
            if MLP_FOLD_SC[0]:
                x4, xbs = nchw(x)
                fold = x4.data_ptr() % 16 == 0 and xbs % 4 == 0 and ws.is_contiguous()
            if fold:
                out = out0 if out0 is not None else _empty(N, P, H, W, h)
                flops = _mlp_flops(N, C, P, HW) + 2.0 * N * HW * C * P
                nbytes = _nb(h, w1, b1, w2, b2, x4, ws) + (2 if acc1 else 1) * _nb(out)
            else:
                out = conv_fwd_raw(x, ws, None, 1, 0, out=out0, accumulate=acc1)
                flops, nbytes = _mlp_flops(N, C, P, HW), _nb(h, w1, b1, w2, b2) + 2 * _nb(out)
            with _timed(IGEMM_TIMER, flops, ("mlp_fwd", N, C, H, W, P, 1, 1), "mlp_fwd_kernel", nbytes):
                mlp = (ptr(h), hbs, hb, ptr(bf16_weight(w1)), ptr(b1), ptr(bf16_weight(w2)), ptr(b2))
                if fold:
                    call("dsgan_mlp_fwd_sc", *mlp, ptr(x4), xbs, ptr(bf16_weight(ws)), ptr(out), obs, N, C, P, HW,
                         int(acc1), stream())
                else:
                    call("dsgan_mlp_fwd", *mlp, ptr(out), obs, N, C, P, HW, 1, stream())
            ctx.save_for_backward(h, x, ws)
            return acc if acc1 else out
        w1v = w1.view(w1.shape[0], w1.shape[1], 1, 1)
        w2v = w2.view(w2.shape[0], w2.shape[1], 1, 1)
        ctx.g = None
        if bigg:
            # large blocks: pwconv1 evaluates GELU once and writes g = gelu(z) and gp = gelu'(z), both
            # bf16; pwconv2 and the W2 weight-grad stream g, the pwconv2 data-grad multiplies by gp
            gp = torch.empty((N, C4, H, W), device=h.device, dtype=half_dtype())   # gelu'(z), for dz
            g = torch.empty((N, C4, H, W), device=h.device, dtype=half_dtype())    # gelu(z)
            with _timed(IGEMM_TIMER, 2.0 * N * HW * C4 * C, ("fwd", N, C, H, W, C4, 1, 1), "pwgemm_kernel",
                        _nb(h, w1, b1, g, gp)):
                call("dsgan_pw_fwd_io_ws", ptr(bf16_weight(w1)), 1, ptr(h), hbs, hb, ptr(g), C4 * HW, 1, ptr(gp),
                     C4 * HW, 1, ptr(b1), C4, C, HW, N, ACT["gelu"], 0, LRELU_SLOPE,
                     *wsa(_ws("dsgan_pw_fd_workspace", 0, C4, C, HW, N, like=h)), stream())
            out = conv_fwd_raw(x, ws, None, 1, 0, out=out0, accumulate=acc1)
            with _timed(IGEMM_TIMER, 2.0 * N * HW * C4 * P, ("fwd", N, C4, H, W, P, 1, 1), "pwgemm_kernel",
                        _nb(g, w2, b2) + 2 * _nb(out)):
                call("dsgan_pw_fwd_io_ws", ptr(bf16_weight(w2)), 1, ptr(g), C4 * HW, 1, ptr(out), obs, 0, None, 0, 0,
                     ptr(b2), P, C4, HW, N, 0, 1, LRELU_SLOPE,
                     *wsa(_ws("dsgan_pw_fd_workspace", 0, P, C4, HW, N, like=g)), stream())
            ctx.g = g
            ctx.save_for_backward(h, x, gp, w1v, w2v, ws)
            return acc if acc1 else out
        z = conv_fwd_raw(h, w1v, b1, 1, 0)
        x4, xbs = nchw(x)
        out = out0 if out0 is not None else _empty(N, P, H, W, h)
        if 5 * C <= 16 and _pws_ok(5 * C, P, HW, xbs, obs, x4.data_ptr(), z.data_ptr()) \
                and out.data_ptr() % 16 == 0:
            # tiny blocks (c1: 3 -> 12 -> 64 at 256^2): shortcut + pwconv2 in one streaming pass
            with _timed(IGEMM_TIMER, 2.0 * N * HW * P * 5 * C, ("fwd", N, 5 * C, H, W, P, 1, 1), "pw_small_kernel",
                        _nb(x4, z, out, ws, w2, b2)):
                call("dsgan_pw_small2", ptr(x4), xbs, ptr(ws), C, 1, ptr(z), 4 * C * HW, ptr(w2), 4 * C, ptr(b2),
                     ptr(out), obs, None, 0, N, C, P, HW, 0, ACT["gelu"], 0, int(acc1), LRELU_SLOPE, stream())
        else:
            conv_fwd_raw(x, ws, None, 1, 0, out=out, accumulate=acc1)
            conv_fwd_raw(z, w2v, b2, 1, 0, out=out, accumulate=True, xact="gelu")
        ctx.save_for_backward(h, x, z, w1v, w2v, ws)
        return acc if acc1 else out

    @staticmethod
    def backward(ctx, dy):
        with precision(ctx.prec):
            if ctx.tile:
                dh, dx = PwMlpFn._backward_fused(ctx, dy)
            else:
                dh, dx = PwMlpFn._backward_unfused(ctx, dy)
            if dh is not None and ctx.nrm is not None:
                d, mean, rstd = ctx.nrm
                dh = instnorm_bwd_raw(dh, d, None, None, mean, rstd, None, False, False)[0]
            ctx.nrm = None
        # out = acc + block: acc's grad is dy itself (borrowed, never adopted as a buffer)
        dacc = _give(ctx.box_acc, dy, adopt=False) if ctx.needs_input_grad[9] else None
        return _give(ctx.box_h, dh), dx, None, None, None, None, None, None, None, dacc

    # Every backward arm issues, after its data-path kernels: the W2 (or bare b2) grad, the
    # shortcut's weight-grad, the W1 (or bare b1) grad, then -- _done -- the readiness hook and the
    # shortcut's data-grad.  The arms differ in which kernel forms the W2 / W1 grads.

    @staticmethod
    def _b2_sc(dy, x, gb2, gws):
        """The b2 grad where no weight-grad kernel summed it (gb2 still set), then the shortcut's weight-grad."""
        if gb2 is not None:
            channel_sum_raw(dy, gb2)
        if gws is not None:
            conv_wgrad_raw(dy, x, gws, 1, 0)

    @staticmethod
    def _gdz_wgrads(ctx, dy, dybs, g, dz, h, x, grads):
        """The parameter grads from the 16-bit g = gelu(z) and dz.  The bias grads ride on the
        weight-grads' staged A tiles (db += sum_k A): b2 from dy, b1 from the bf16 dz (as the fused
        kernels sum it); a frozen weight with a trainable bias (not on the train path) takes a
        channel sum instead."""
        gw2, gb2, gws, gw1, gb1 = grads
        N, C, H, W = h.shape
        HW, C4, P = H * W, 4 * C, dy.shape[1]
        if gw2 is not None:
            with _timed(IGEMM_TIMER, 2.0 * N * HW * C4 * P, ("wgrad", N, C4, H, W, P, 1, 1), "pwgemm_kernel",
                        _nb(dy, g, gw2)):
                call("dsgan_pw_wgrad_mixed", ptr(dy), dybs, 0, ptr(g), C4 * HW, 1, ptr(gw2), ptr(gb2), P, C4, HW, N,
                     *wsa(_pw_ws(P, C4, HW, N, dy)), stream())
            gb2 = None
        PwMlpFn._b2_sc(dy, x, gb2, gws)
        if gw1 is not None:
            with _timed(IGEMM_TIMER, 2.0 * N * HW * C4 * C, ("wgrad", N, C, H, W, C4, 1, 1), "pwgemm_kernel",
                        _nb(dz, h, gw1)):
                call("dsgan_pw_wgrad_mixed", ptr(dz), C4 * HW, 1, ptr(h), C * HW, ctx.hb, ptr(gw1), ptr(gb1), C4, C,
                     HW, N, *wsa(_pw_ws(C4, C, HW, N, dz)), stream())
        elif gb1 is not None:
            channel_sum_raw(dz.float(), gb1)

    @staticmethod
    def _done(ctx, dy, ws, x):
        """Report the parameters' grads launched; returns the shortcut data-grad, accumulated into
        the shared buffer of x when there is one."""
        _params_done(*ctx.refs)
        if not ctx.needs_input_grad[1]:
            return None
        out, acc = _acc_target(ctx.box_x)
        dx = conv_dgrad_raw(dy, ws, tuple(x.shape), 1, 0, out=out, accumulate=acc)
        return None if acc else _give(ctx.box_x, dx)

    @staticmethod
    def _backward_unfused(ctx, dy):
        h, x, z, w1v, w2v, ws = ctx.saved_tensors
        w1, b1, w2, b2, ws_ref = ctx.refs
        # dy may be a channel slice of a concat gradient (c1's output feeds the u4 concat): every
        # consumer below takes a batch stride, so only a misaligned slice is copied
        dy, dybs = nchw(dy)
        if dy.data_ptr() % 16 or dybs % 8:
            dy = dy.contiguous()
            dybs = dy.shape[1] * dy.shape[2] * dy.shape[3]
        grads = gw2, gb2, gws, gw1, gb1 = tuple(_grad_buf(t) for t in (w2, b2, ws_ref, w1, b1))
        want_dh = ctx.needs_input_grad[0]
        if ctx.g is not None:
            # bf16 g/gp path (z slot holds gp = gelu'(z)): dz = (W2^T dy) * gp stored bf16, the b1
            # grad as fp32 partial row sums of the same epilogue
            N, C4, H, W = z.shape
            HW, P, C = H * W, w2.shape[0], h.shape[1]
            dz = torch.empty((N, C4, H, W), device=dy.device, dtype=half_dtype())
            with _timed(IGEMM_TIMER, 2.0 * N * HW * C4 * P, ("dgrad", N, C4, H, W, P, 1, 1), "pwgemm_kernel",
                        _nb(dy, w2, dz, z)):
                call("dsgan_pw_dgrad_io_ws", ptr(bf16_weight(w2)), 1, ptr(dy), dybs, 0, ptr(dz), C4 * HW, 1, ptr(z),
                     C4 * HW, C4, P, HW, N, 0, *wsa(_ws("dsgan_pw_fd_workspace", 1, C4, P, HW, N, like=dy)), stream())
            PwMlpFn._gdz_wgrads(ctx, dy, dybs, ctx.g, dz, h, x, grads)
            dh = None
            if want_dh:
                dh = _empty(N, C, H, W, dy)
                with _timed(IGEMM_TIMER, 2.0 * N * HW * C4 * C, ("dgrad", N, C4, H, W, C, 1, 1), "pwgemm_kernel",
                            _nb(dz, w1, dh)):
                    call("dsgan_pw_dgrad_io_ws", ptr(bf16_weight(w1)), 1, ptr(dz), C4 * HW, 1, ptr(dh), C * HW, 0, None,
                         0, C, C4, HW, N, 0, *wsa(_ws("dsgan_pw_fd_workspace", 1, C, C4, HW, N, like=dz)), stream())
            return dh, PwMlpFn._done(ctx, dy, ws, x)
        # fp32 z path: dz = (W2^T dy) * gelu'(z)
        dz = conv_dgrad_raw(dy, w2v, tuple(z.shape), 1, 0, gpre=z, gact="gelu")
        if gw2 is not None and conv_wgrad_raw(dy, z, gw2.view(w2v.shape), 1, 0, xact="gelu", db=gb2):
            gb2 = None
        PwMlpFn._b2_sc(dy, x, gb2, gws)
        if gw1 is not None and conv_wgrad_raw(dz, h, gw1.view(w1v.shape), 1, 0, db=gb1):
            gb1 = None
        if gb1 is not None:
            channel_sum_raw(dz, gb1)
        dh = conv_dgrad_raw(dz, w1v, tuple(h.shape), 1, 0) if want_dh else None
        return dh, PwMlpFn._done(ctx, dy, ws, x)

    @staticmethod
    def _backward_fused(ctx, dy):
        h, x, ws = ctx.saved_tensors
        w1, b1, w2, b2, ws_ref = ctx.refs
        N, C, H, W = h.shape
        HW, C4, P = H * W, 4 * h.shape[1], w2.shape[0]
        dy, dybs = nchw(dy)
        if dy.data_ptr() % 16:
            dy, dybs = dy.contiguous(), P * HW
        grads = gw2, gb2, gws, gw1, gb1 = tuple(_grad_buf(t) for t in (w2, b2, ws_ref, w1, b1))
        dh = _empty(N, C, H, W, h)
        if gw1 is not None and gb1 is not None and gw2 is not None and C < 256:
            # dh from the data-path kernel; dW1 / db1 / dW2 from the weight-path kernel, which
            # recomputes z and dz per hidden chunk -- gelu(z) and dz never reach HBM.  (Both kernels
            # are GELU/VALU-bound, so the recompute pays only where the bf16 g/dz round trip is the
            # larger cost: measured at B=16, C=128 @256^2 1.98 -> 1.77 ms, C=256 @128^2 1.70 -> 1.94 ms.)
            w1b, w2b = bf16_weight(w1), bf16_weight(w2)
            with _timed(IGEMM_TIMER, 2.0 * N * HW * C4 * (2 * C + P), ("mlp_bwd", N, C, H, W, P, 1, 1),
                        "mlp_bwd_kernel", _nb(h, dy, w1, b1, w2, dh)):
                call("dsgan_mlp_bwd", ptr(h), C * HW, ctx.hb, ptr(dy), dybs, ptr(w1b), ptr(b1), ptr(w2b), ptr(dh),
                     C * HW, None, None, None, N, C, P, HW, stream())
            with _timed(IGEMM_TIMER, 2.0 * N * HW * C4 * (2 * C + 2 * P), ("mlp_wgrad", N, C, H, W, P, 1, 1),
                        "mlp_wgrad_kernel", _nb(h, dy, w1, b1, w2, gw1, gb1, gw2)):
                call("dsgan_mlp_wgrad", ptr(h), C * HW, ctx.hb, ptr(dy), dybs, ptr(w1b), ptr(b1), ptr(w2b), ptr(gw1),
                     ptr(gb1), ptr(gw2), *wsa(_ws("dsgan_mlp_wgrad_workspace", C, P, HW, N, like=h)), N, C, P, HW,
                     stream())
            PwMlpFn._b2_sc(dy, x, gb2, gws)
            return dh, PwMlpFn._done(ctx, dy, ws, x)
        g = torch.empty((N, C4, H, W), device=h.device, dtype=half_dtype())
        dz = torch.empty_like(g)
        with _timed(IGEMM_TIMER, _mlp_flops(N, C, P, HW), ("mlp_bwd", N, C, H, W, P, 1, 1), "mlp_bwd_kernel",
                    _nb(h, dy, w1, b1, w2, dh, g, dz)):
            call("dsgan_mlp_bwd", ptr(h), C * HW, ctx.hb, ptr(dy), dybs, ptr(bf16_weight(w1)), ptr(b1),
                 ptr(bf16_weight(w2)), ptr(dh), C * HW, ptr(g), ptr(dz), None, N, C, P, HW, stream())
        PwMlpFn._gdz_wgrads(ctx, dy, dybs, g, dz, h, x, grads)
        return dh, PwMlpFn._done(ctx, dy, ws, x)


def pw_mlp(h, x, w1, b1, w2, b2, ws, norm=False, slot=None, acc=None):
    """ConvNeXt block tail; with norm=True the first argument is the depthwise-conv output d and
    the block's InstanceNorm h = IN(d) is applied inside (MixConvNeXtML.py:219-224).  ``slot``
    (CatSlot): the output is written into the slot's tail and returned as that alias.  ``acc``: the
    output is summed into acc in place (acc + block: the epilogue of the block's first kernel adds
    acc) and acc is returned."""
    return PwMlpFn.apply(h, x, w1, b1, w2, b2, ws, norm, slot, acc)


# ------------------------------------------------------------------------------------------
# Depthwise conv
# ------------------------------------------------------------------------------------------

def dwconv_raw(x, w, b, flip=False, out=None, accumulate=False):
    x, xbs = nchw(x)
    N, C, H, W = x.shape
    K = w.shape[-1]
    y = out if out is not None else _empty(N, C, H, W, x)
    y4, ybs = nchw(y)
    with _timed(AUX_TIMER, 2.0 * N * C * H * W * K * K, ("dw_dgrad" if flip else "dw_fwd", N, C, H, W, K), "dwconv",
                (3 if accumulate else 2) * _nb(x)):
        call("dsgan_dwconv_fwd", ptr(x), xbs, ptr(w), ptr(b), ptr(y4), ybs, N, C, H, W, K, int(flip), int(accumulate),
             stream())
    return y4


def _dw_wgrad(dy, x, gw, gb, K):
    dy4, dybs = nchw(dy)
    x4, xbs = nchw(x)
    N, C, H, W = x4.shape
    al = int(x4.data_ptr() % 16 == 0 and dy4.data_ptr() % 16 == 0 and xbs % 4 == 0 and dybs % 4 == 0)
    with _timed(AUX_TIMER, 2.0 * N * C * H * W * K * K, ("dw_wgrad", N, C, H, W, K), "dwconv", 2 * _nb(x4)):
        call("dsgan_dwconv_wgrad", ptr(dy4), dybs, ptr(x4), xbs, ptr(gw), ptr(gb), N, C, H, W, K,
             *wsa(_ws("dsgan_dwconv_wgrad_workspace", N, C, H, W, K, al, like=x4)), stream())


class DwConvFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, w, b):
        y = dwconv_raw(x, w, b)
        ctx.save_for_backward(x, w)
        ctx.refs = (w, b)
        ctx.box = _box(x)
        return y

    @staticmethod
    def backward(ctx, dy):
        x, w = ctx.saved_tensors
        wr, br = ctx.refs
        dx = None
        if ctx.needs_input_grad[0]:
            out, acc = _acc_target(ctx.box)
            dx = dwconv_raw(dy, w, None, flip=True, out=out, accumulate=acc)
            dx = None if acc else _give(ctx.box, dx)
        gw, gb = _grad_buf(wr), _grad_buf(br)
        if gw is not None:
            _dw_wgrad(dy, x, gw, gb, w.shape[-1])
        _params_done(wr, br)
        return dx, None, None


def dwconv(x, w, b):
    return DwConvFn.apply(x, w, b)


class MultiDwConvFn(torch.autograd.Function):
    """MidMLKA's chunk(4) -> X3/X5/X7/X9 depthwise -> cat (MixConvNeXtML.py:110-111), written
    straight into one output buffer (no chunk/cat copies); one launch per pass over the four
    quarters where the plane shape takes a tiled configuration (dsgan_dwconv_multi_*)."""

    @staticmethod
    def _multi_ok(x4, xbs, y, ybs):
        N, C, H, W = x4.shape
        return C % 4 == 0 and bool(_lib.load().dsgan_dwconv_multi_supported(H, W, ptr(x4), xbs, ptr(y), ybs))

    @staticmethod
    def forward(ctx, x, *wb):
        x4, xbs = nchw(x)
        N, C, H, W = x4.shape
        q = C // 4
        y = _empty(N, C, H, W, x4)
        if MultiDwConvFn._multi_ok(x4, xbs, y, C * H * W):
            with _timed(AUX_TIMER, 2.0 * N * q * H * W * (9 + 25 + 49 + 81), ("dw_multi_fwd", N, C, H, W, 0), "dwconv",
                        2 * _nb(x4)):
                call("dsgan_dwconv_multi_fwd", ptr(x4), xbs, *[ptr(t) for t in wb], ptr(y), C * H * W, N, q, H, W, 0,
                     0, stream())
        else:
            for i in range(4):
                dwconv_raw(x4[:, i * q:(i + 1) * q], wb[2 * i], wb[2 * i + 1], out=y[:, i * q:(i + 1) * q])
        ctx.save_for_backward(x4, *wb)
        ctx.refs = wb
        ctx.box = _box(x)
        return y

    @staticmethod
    def backward(ctx, dy):
        x, *wb = ctx.saved_tensors
        N, C, H, W = x.shape
        q = C // 4
        dy4, dybs = nchw(dy)
        out, acc = _acc_target(ctx.box)
        dx = None
        if ctx.needs_input_grad[0]:
            dx = out if acc else _empty(N, C, H, W, x)
        grads = [_grad_buf(r) for r in ctx.refs]
        xbs = x.stride(0) if N > 1 else C * H * W
        multi = MultiDwConvFn._multi_ok(x, xbs, dy4, dybs) and (dx is None or dx.stride(0) == C * H * W or N == 1)
        if multi:
            if dx is not None:
                with _timed(AUX_TIMER, 2.0 * N * q * H * W * 164, ("dw_multi_dgrad", N, C, H, W, 0), "dwconv",
                            (3 if acc else 2) * _nb(x)):
                    call("dsgan_dwconv_multi_fwd", ptr(dy4), dybs,
                         *[ptr(t) if i % 2 == 0 else None for i, t in enumerate(wb)], ptr(dx), C * H * W, N, q, H, W,
                         1, int(acc), stream())
            if all(g_ is not None for g_ in grads):
                with _timed(AUX_TIMER, 2.0 * N * q * H * W * 164, ("dw_multi_wgrad", N, C, H, W, 0), "dwconv", 2 * _nb(x)):
                    call("dsgan_dwconv_multi_wgrad", ptr(dy4), dybs, ptr(x), xbs, *[ptr(g_) for g_ in grads], N, q, H,
                         W, *wsa(_ws("dsgan_dwconv_multi_wgrad_workspace", N, q, H, W, like=x)), stream())
                grads = [None] * 8
        else:
            for i in range(4):
                sl = slice(i * q, (i + 1) * q)
                if dx is not None:
                    dwconv_raw(dy4[:, sl], wb[2 * i], None, flip=True, out=dx[:, sl], accumulate=acc)
        for i in range(4):
            gw, gb = grads[2 * i], grads[2 * i + 1]
            if gw is not None:
                sl = slice(i * q, (i + 1) * q)
                _dw_wgrad(dy4[:, sl], x[:, sl], gw, gb, wb[2 * i].shape[-1])
        dx = None if acc else _give(ctx.box, dx)
        _params_done(*ctx.refs)
        return (dx,) + (None,) * 8


def multi_dwconv(x, w3, b3, w5, b5, w7, b7, w9, b9):
    return MultiDwConvFn.apply(x, w3, b3, w5, b5, w7, b7, w9, b9)


# ------------------------------------------------------------------------------------------
# InstanceNorm (+scale, +residual, +act)
# ------------------------------------------------------------------------------------------

def instnorm_raw(x, scale=None, res=None, act=None, out=None):
    x, xbs = nchw(x)
    N, C, H, W = x.shape
    rbs = 0
    if res is not None:
        res, rbs = nchw(res)
    y = out if out is not None else _empty(N, C, H, W, x)
    y4, ybs = nchw(y)
    mean = torch.empty(N * C, device=x.device, dtype=torch.float32)
    rstd = torch.empty(N * C, device=x.device, dtype=torch.float32)
    # (scratch: the split forms for few large planes)
    with _timed(AUX_TIMER, 0.0, ("in_fwd", N, C, H, W, act, res is not None), "instnorm",
                (3 if res is not None else 2) * _nb(x)):
        call("dsgan_instnorm_fwd_ws", ptr(x), xbs, ptr(scale), ptr(res), rbs, ptr(y4), ybs, ptr(mean),
             ptr(rstd), N, C, H * W, _in_act(act), LRELU_SLOPE, IN_EPS,
             *wsa(_ws("dsgan_instnorm_workspace", N, C, H * W, like=x)), stream())
    return y4, mean, rstd


def instnorm_bwd_raw(dy, x, scale, res, mean, rstd, act, want_dres, want_dscale):
    dy, dybs = nchw(dy)
    x, xbs = nchw(x)
    N, C, H, W = x.shape
    rbs = 0
    if res is not None:
        res, rbs = nchw(res)
    dx = _empty(N, C, H, W, x)
    dres = _empty(N, C, H, W, x) if want_dres else None
    dscale = torch.empty(N * C, device=x.device, dtype=torch.float32) if want_dscale else None
    with _timed(AUX_TIMER, 0.0, ("in_bwd", N, C, H, W, act, res is not None), "instnorm",
                (3 + (res is not None) + want_dres) * _nb(x)):
        call("dsgan_instnorm_bwd_ws", ptr(dy), dybs, ptr(x), xbs, ptr(scale), ptr(res), rbs, ptr(mean),
             ptr(rstd), ptr(dx), C * H * W, ptr(dres), C * H * W, ptr(dscale), N, C, H * W, _in_act(act),
             LRELU_SLOPE, IN_EPS, *wsa(_ws("dsgan_instnorm_workspace", N, C, H * W, like=x)), stream())
    return dx, dres, dscale


class InstanceNormFn(torch.autograd.Function):
    """y = act(IN(x) + res) -- InstanceNorm2d(affine=False) fused with what follows it."""

    @staticmethod
    def forward(ctx, x, res, act):
        y, mean, rstd = instnorm_raw(x, None, res, act)
        ctx.act = act
        ctx.save_for_backward(x, res, mean, rstd)
        ctx.box_x, ctx.box_r = _box(x), (_box(res) if res is not None else None)
        return y

    @staticmethod
    def backward(ctx, dy):
        x, res, mean, rstd = ctx.saved_tensors
        dx, dres, _ = instnorm_bwd_raw(dy, x, None, res, mean, rstd, ctx.act,
                                       res is not None and ctx.needs_input_grad[1], False)
        return _give(ctx.box_x, dx), _give(ctx.box_r, dres), None


def instance_norm(x, act=None, res=None):
    return InstanceNormFn.apply(x, res, act)


# ------------------------------------------------------------------------------------------
# BatchNorm2d (affine, running statistics) + act: the PatchGAN under --norm batch (batchnorm.hip)
# ------------------------------------------------------------------------------------------

def _bn_check(shape, training, momentum):
    if momentum is None:
        raise NotImplementedError("batch_norm: momentum=None (a cumulative moving average) is not on the HIP path")
    if training and shape[0] * shape[2] * shape[3] == 1:   # torch's own error (F.batch_norm), before any launch
        raise ValueError("Expected more than 1 value per channel when training, got input size %s"
                         % (torch.Size(shape),))


def batchnorm_raw(x, weight, bias, running_mean, running_var, num_batches_tracked, training, momentum=0.1, eps=IN_EPS,
                  act=None, out=None):
    """y = act(BN(x)) with the batch's statistics (training: the running buffers and the int64 counter
    are updated on the device) or the running buffers (eval).  Returns (y, mean, rstd): what the
    output was normalised with, for batchnorm_bwd_raw."""
    x, xbs = nchw(x)
    N, C, H, W = x.shape
    _bn_check(x.shape, training, momentum)
    y = out if out is not None else _empty(N, C, H, W, x)
    y4, ybs = nchw(y)
    mean = torch.empty(C, device=x.device, dtype=torch.float32)
    rstd = torch.empty(C, device=x.device, dtype=torch.float32)
    with _timed(AUX_TIMER, 0.0, ("bn_fwd", N, C, H, W, act, bool(training)), "batchnorm", 2 * _nb(x)):
        call("dsgan_batchnorm_fwd", ptr(x), xbs, ptr(weight), ptr(bias), ptr(y4), ybs, ptr(mean), ptr(rstd),
             ptr(running_mean), ptr(running_var), ptr(num_batches_tracked), N, C, H * W, ACT[act], LRELU_SLOPE,
             float(eps), float(momentum), 1 if training else 0,
             *wsa(_ws("dsgan_batchnorm_workspace", N, C, H * W, like=x)), stream())
    return y4, mean, rstd


def batchnorm_bwd_raw(dy, x, weight, bias, mean, rstd, act, training, dweight=None, dbias=None):
    """dx of batchnorm_raw; dweight / dbias (a pair, or neither) are accumulated into."""
    dy, dybs = nchw(dy)
    x, xbs = nchw(x)
    N, C, H, W = x.shape
    dx = _empty(N, C, H, W, x)
    with _timed(AUX_TIMER, 0.0, ("bn_bwd", N, C, H, W, act, bool(training)), "batchnorm", 3 * _nb(x)):
        call("dsgan_batchnorm_bwd", ptr(dy), dybs, ptr(x), xbs, ptr(weight), ptr(bias), ptr(mean), ptr(rstd), ptr(dx),
             C * H * W, ptr(dweight), ptr(dbias), N, C, H * W, ACT[act], LRELU_SLOPE, 1 if training else 0,
             *wsa(_ws("dsgan_batchnorm_workspace", N, C, H * W, like=x)), stream())
    return dx


class BatchNormFn(torch.autograd.Function):
    """y = act(BatchNorm2d(x)) -- only x is saved; the backward recomputes z from x, mean, rstd."""

    @staticmethod
    def forward(ctx, x, weight, bias, bn, act):
        y, mean, rstd = batchnorm_raw(x, weight, bias, bn.running_mean, bn.running_var, bn.num_batches_tracked,
                                      bn.training, bn.momentum, bn.eps, act)
        ctx.act, ctx.training = act, bool(bn.training)
        ctx.save_for_backward(x, weight, bias, mean, rstd)
        ctx.w_ref, ctx.b_ref = weight, bias
        ctx.box = _box(x)
        return y

    @staticmethod
    def backward(ctx, dy):
        x, weight, bias, mean, rstd = ctx.saved_tensors
        gw = _grad_buf(ctx.w_ref) if ctx.needs_input_grad[1] else None
        gb = _grad_buf(ctx.b_ref) if ctx.needs_input_grad[2] else None
        if (gw is None) != (gb is None):
            raise RuntimeError("batch_norm: weight and bias must both need a gradient, or neither")
        dx = batchnorm_bwd_raw(dy, x, weight, bias, mean, rstd, ctx.act, ctx.training, gw, gb)
        _params_done(ctx.w_ref, ctx.b_ref)
        return _give(ctx.box, dx), None, None, None, None


def batch_norm(x, bn, act=None):
    """``act(bn(x))`` for an ``nn.BatchNorm2d`` (affine, with running statistics): its weight, bias,
    buffers, eps, momentum and ``training`` are read from the module."""
    if bn.weight is None or bn.running_mean is None:
        raise NotImplementedError("batch_norm: needs affine=True and track_running_stats=True (the reference's "
                                  "get_norm_layer('batch'))")
    _bn_check(x.shape, bn.training, bn.momentum)
    return BatchNormFn.apply(x, bn.weight, bn.bias, bn, act)


def _instnorm_cat(x, skip, act, slot):
    """(cat(act(IN(x)), skip), mean, rstd): the IN kernel writes into the first channels of the
    concatenation; the skip is copied behind them unless it already sits there (``slot``'s tail)."""
    N, Ca, H, W = x.shape
    held = slot is not None and slot.holds(skip, Ca)   # the skip's producer already wrote it into the tail
    out = slot.whole() if held else _empty(N, Ca + skip.shape[1], H, W, x)
    _, mean, rstd = instnorm_raw(x, None, None, act, out=out[:, :Ca])
    if not held:
        copy_into(out[:, Ca:], skip)
    return out, mean, rstd


class InstanceNormCatFn(torch.autograd.Function):
    """cat(act(IN(x)), skip) along channels: the IN kernel writes its plane straight into the
    first Ca channels of the concatenation (upSample, MixConvNeXtML.py:61-66), so only the skip
    is copied; the backward reads its slice of dy in place."""

    @staticmethod
    def forward(ctx, x, skip, act, slot=None):
        out, mean, rstd = _instnorm_cat(x, skip, act, slot)
        ctx.act, ctx.Ca = act, x.shape[1]
        ctx.save_for_backward(x, mean, rstd)
        ctx.box_x, ctx.box_s = _box(x), _box(skip)
        return out

    @staticmethod
    def backward(ctx, dy):
        x, mean, rstd = ctx.saved_tensors
        dx, _, _ = instnorm_bwd_raw(dy[:, :ctx.Ca], x, None, None, mean, rstd, ctx.act, False, False)
        return _give(ctx.box_x, dx), _give(ctx.box_s, dy[:, ctx.Ca:]), None, None


def instance_norm_cat(x, skip, act=None, slot=None):
    return InstanceNormCatFn.apply(x, skip, act, slot)


class ConvTNormFn(torch.autograd.Function):
    """ConvTranspose2d 3x3/s2 (pad 1, output_padding 1) feeding the decoder InstanceNorm:
    cat(act(IN(convT(x))), skip) (upSample, MixConvNeXtML.py:48-66) or act(IN(convT(x)) + res)
    (OriginMLKA tail, :150-152).  The forward is ConvT3s2Fn's then InstanceNorm(Cat)Fn's.  The
    backward keeps the ConvT output grad off fp32: dsgan_instnorm_bwd_h stores it in the 16-bit
    half type with its per-plane sums, the ConvT data-grad (dsgan_tconv_ws_xh) and weight-grad
    (dsgan_wconv_xh) read those 16 bits as MFMA operands -- exactly the values the fp32-input forms
    round to on load, so dx and dW are unchanged -- and the bias grad is the sum over images of
    the plane sums (the fp32 values, as channel_sum of the fp32 grad would add them)."""

    @staticmethod
    def forward(ctx, x, w, b, other, act, cat, slot=None):
        N, Ci, Hi, Wi = x.shape
        Co = w.shape[1]
        t = conv_dgrad_raw(x, w, (N, Co, 2 * Hi, 2 * Wi), 2, 1, bias=b)
        if cat:
            out, mean, rstd = _instnorm_cat(t, other, act, slot)
            ctx.save_for_backward(x, w, t, mean, rstd)
        else:
            out, mean, rstd = instnorm_raw(t, None, other, act)
            ctx.save_for_backward(x, w, t, mean, rstd, other)
        ctx.prec, ctx.act, ctx.cat, ctx.has_b = _state["prec"], act, cat, b is not None
        ctx.w_ref, ctx.b_ref = w, b
        ctx.box_x, ctx.box_o = _box(x), _box(other)
        return out

    @staticmethod
    def backward(ctx, dy):
        with precision(ctx.prec):
            return ConvTNormFn._backward(ctx, dy)

    @staticmethod
    def _backward(ctx, dy):
        if ctx.cat:
            x, w, t, mean, rstd = ctx.saved_tensors
            res = None
        else:
            x, w, t, mean, rstd, res = ctx.saved_tensors
        N, Ci, Hi, Wi = x.shape
        Co, H, W = t.shape[1], t.shape[2], t.shape[3]
        HW = H * W
        dyt, dybs = nchw(dy[:, :Co] if ctx.cat else dy)
        t4, tbs = nchw(t)
        rbs = 0
        if res is not None:
            res, rbs = nchw(res)
        want_dres = res is not None and ctx.needs_input_grad[3]
        dres = _empty(N, Co, H, W, t) if want_dres else None
        dth = torch.empty((N, Co, H, W), device=t.device, dtype=half_dtype())
        psum = torch.empty(N * Co, device=t.device, dtype=torch.float32)
        with _timed(AUX_TIMER, 0.0, ("in_bwd_h", N, Co, H, W, ctx.act, res is not None), "instnorm",
                    _nb(dyt, t4, res, dres) + _nb(dth)):
            call("dsgan_instnorm_bwd_h", ptr(dyt), dybs, ptr(t4), tbs, ptr(res), rbs, ptr(mean), ptr(rstd), ptr(dth),
                 Co * HW, ptr(psum), ptr(dres), Co * HW, N, Co, HW, _in_act(ctx.act), LRELU_SLOPE, IN_EPS, stream())
        dx = None
        if ctx.needs_input_grad[0]:
            dx = _empty(N, Ci, Hi, Wi, x)
            taps = [(kh - 1, kw - 1) for kh in range(3) for kw in range(3)]
            with _timed(IGEMM_TIMER, _conv_flops(N, Co, Ci, 3, 3, Hi, Wi), ("fwd", N, Co, H, W, Ci, 3, 2),
                        "tconv_kernel", _nb(dth, dx) + 2.0 * w.numel()):
                _tconv(dth, Co * HW, _wtrans_bf16(w, 0), None, dx, Ci * Hi * Wi, None, 0, N, Co, Ci, H, W, Hi, Wi, 2,
                       taps, Hi, Wi, 1, 0, 0, None, None, xh=True)
        gw = _grad_buf(ctx.w_ref) if ctx.needs_input_grad[1] else None
        if gw is not None:
            x4, xbs = nchw(x)
            with _timed(IGEMM_TIMER, _conv_flops(N, Co, Ci, 3, 3, Hi, Wi), ("wgrad", N, Co, H, W, Ci, 3, 2),
                        "wconv_kernel", _nb(x4, dth, gw)):
                call("dsgan_wconv_xh", ptr(x4), xbs, ptr(dth), Co * HW, ptr(gw),
                     *wsa(_ws("dsgan_wconv_workspace", N, Co, Ci, Hi, Wi, 3, 3, like=t)), N, Co, Ci, H, W, Hi, Wi, 3,
                     3, 2, 1, stream())
        gb = _grad_buf(ctx.b_ref) if (ctx.has_b and ctx.needs_input_grad[2]) else None
        if gb is not None:
            channel_sum_raw(psum.view(N, Co, 1, 1), gb)
        _params_done(ctx.w_ref, ctx.b_ref)
        dother = _give(ctx.box_o, dy[:, Co:]) if ctx.cat else _give(ctx.box_o, dres)
        return _give(ctx.box_x, dx), None, None, dother, None, None, None


def _convt_norm_fused(x, w, other, cat):
    """The fused ConvT + InstanceNorm backward's conditions: 16-bit operands (bf16 / fp16 mode),
    K (ConvT output channels) % 32 for the 16-bit-operand kernels, float4-aligned planes."""
    N, Ci, Hi, Wi = x.shape
    Co = w.shape[1]
    HW = 4 * Hi * Wi
    return (_is16() and w.dim() == 4 and w.shape[2] == 3 and w.shape[3] == 3 and Co % 32 == 0 and Ci % 32 == 0
            and HW % 4 == 0 and (2 * Wi) % 4 == 0 and bool(_lib.load().dsgan_wconv_supported(Co, 3, 3, 2)))


def convt_norm(x, w, b, other, act=None, cat=False, slot=None):
    """cat(act(IN(ConvT3s2(x))), other) if cat else act(IN(ConvT3s2(x)) + other) (other may be None).
    ``slot`` (CatSlot, cat only): when ``other`` is the slot's tail the concatenation is formed in
    place and returned as ``slot.whole()``."""
    if _convt_norm_fused(x, w, other, cat):
        return ConvTNormFn.apply(x, w, b, other, act, cat, slot)
    y = conv_transpose3s2(x, w, b)
    return instance_norm_cat(y, other, act, slot) if cat else instance_norm(y, act, other)


# ------------------------------------------------------------------------------------------
# MaxPool2d(k) with int32 plane-flat argmax
# ------------------------------------------------------------------------------------------

class MaxPoolFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, k):
        y, idx = maxpool_raw(x, k)
        ctx.k, ctx.shape = k, tuple(x.shape)
        ctx.save_for_backward(idx)
        ctx.mark_non_differentiable(idx)
        # (no zero-filled int grad for idx per backward: autograd would materialise one)
        ctx.set_materialize_grads(False)
        ctx.box = _box(x)
        return y, idx

    @staticmethod
    def backward(ctx, dy, _didx):
        if dy is None:
            return None, None
        (idx,) = ctx.saved_tensors
        N, C, H, W = ctx.shape
        dy4, dybs = nchw(dy)
        out, acc = _acc_target(ctx.box)
        dx = out if acc else torch.empty((N, C, H, W), device=dy.device, dtype=torch.float32)
        dx4, dxbs = nchw(dx)
        if dx4.data_ptr() != dx.data_ptr():
            raise RuntimeError("maxpool backward: gradient buffer must be per-sample dense")
        call("dsgan_maxpool_bwd", ptr(dy4), dybs, ptr(idx), ptr(dx4), dxbs, N, C, H, W, ctx.k, int(acc), stream())
        return (None if acc else _give(ctx.box, dx)), None


class MaxPoolPyrFn(torch.autograd.Function):
    """MaxPool2d(2), (4), ... (2^levels) of one tensor (the skip pyramids) in one launch each way
    (dsgan_maxpool_pyr_*): one read of x instead of one per k, and one read-modify-write of its
    gradient instead of one per k."""

    @staticmethod
    def forward(ctx, x, levels):
        x4, xbs = nchw(x)
        N, C, H, W = x4.shape
        ys, ids = [], []
        for lv in range(levels):
            k = 2 << lv
            ys.append(_empty(N, C, H // k, W // k, x4))
            ids.append(torch.empty((N, C, H // k, W // k), device=x4.device, dtype=torch.int32))
        args = []
        for lv in range(4):
            args += [ptr(ys[lv]), ptr(ids[lv])] if lv < levels else [None, None]
        call("dsgan_maxpool_pyr_fwd", ptr(x4), xbs, levels, *args, N, C, H, W, stream())
        ctx.levels, ctx.shape = levels, (N, C, H, W)
        ctx.save_for_backward(*ids)
        ctx.mark_non_differentiable(*ids)
        ctx.set_materialize_grads(False)
        ctx.box = _box(x)
        return tuple(ys) + tuple(ids)

    @staticmethod
    def backward(ctx, *grads):
        L = ctx.levels
        dys = grads[:L]
        if all(g is None for g in dys):
            return None, None
        ids = ctx.saved_tensors
        N, C, H, W = ctx.shape
        out, acc = _acc_target(ctx.box)
        dx = out if acc else torch.empty((N, C, H, W), device=ids[0].device, dtype=torch.float32)
        dx4, dxbs = nchw(dx)
        if dx4.data_ptr() != dx.data_ptr():
            raise RuntimeError("maxpool pyramid backward: gradient buffer must be per-sample dense")
        args, keep = [], []
        for lv in range(4):
            if lv < L and dys[lv] is not None:
                d4, dbs = nchw(dys[lv])
                keep.append(d4)
                args += [ptr(d4), dbs, ptr(ids[lv])]
            else:
                args += [None, 0, None]
        call("dsgan_maxpool_pyr_bwd", *args, ptr(dx4), dxbs, L, N, C, H, W, int(acc), stream())
        return (None if acc else _give(ctx.box, dx)), None


def max_pool_pyramid(x, levels):
    """[MaxPool2d(2)(x), MaxPool2d(4)(x), ..., MaxPool2d(2^levels)(x)]: one launch when the shape
    allows (H % 16 == 0, W % 64 == 0), else one max_pool2d per level."""
    N, C, H, W = x.shape
    if _lib.load().dsgan_maxpool_pyr_supported(H, W, levels):
        return list(MaxPoolPyrFn.apply(x, levels)[:levels])
    return [max_pool2d(x, 2 << lv) for lv in range(levels)]


def max_pool2d(x, k, return_indices=False):
    y, idx = MaxPoolFn.apply(x, k)
    return (y, idx) if return_indices else y


def maxpool_raw(x, k):
    """MaxPool2d(k) forward without autograd: (y, int32 plane-flat argmax)."""
    x4, xbs = nchw(x)
    N, C, H, W = x4.shape
    Ho, Wo = H // k, W // k
    y = _empty(N, C, Ho, Wo, x4)
    idx = torch.empty((N, C, Ho, Wo), device=x4.device, dtype=torch.int32)
    call("dsgan_maxpool_fwd", ptr(x4), xbs, ptr(y), C * Ho * Wo, ptr(idx), N, C, H, W, k, stream())
    return y, idx


# ------------------------------------------------------------------------------------------
# VGG16 perceptual term (DSGAN/models/vgg.py:30-42, pix2pix_model.py:180-186) as ONE autograd
# node: loss = L1(f1,r1) + L1(f2,r2) + L1(f3,r3) + L1(f0,r0), f = VGG16(fake), r = VGG16(real).
# Its backward walks the frozen VGG by hand (no weight-grads): each conv data-grad applies the
# ReLU mask of the layer below in its epilogue, and at each tapped layer one kernel forms
# (maxpool backward + L1 backward) * ReLU'  -- no standalone ReLU/L1 passes, no autograd adds.
# ------------------------------------------------------------------------------------------

def vgg_features_raw(x, blocks):
    """blocks = [(pool, [(w, b), ...]), ...] -> (feats, saved): feats = post-ReLU output of each
    block, saved = per block (pool argmax or None, input shape of the pool, [conv outputs])."""
    h = x
    feats, saved = [], []
    for pool, convs in blocks:
        idx, pin = None, None
        if pool:
            pin = tuple(h.shape)
            h, idx = maxpool_raw(h, 2)
        ys = []
        for w, b in convs:
            h = conv_fwd_raw(h, w, b, 1, 1, act="relu")
            ys.append(h)
        feats.append(h)
        saved.append((idx, pin, ys))
    return feats, saved


# ---- the same pass in channel-blocked bf16 (vggconv.hip, bf16 mode at image sizes % 256) ----
# Activations live as CB16 [N][C/16][H][W][16]: bf16 wherever the only consumers are bf16-operand
# MFMAs / ReLU signs / max (exact w.r.t. the bf16 arithmetic), fp32 for the four tapped features
# the L1 loss reads.  The backward's data-grads are stored as the bf16 the next conv consumes.

def vgg_cb16_ok(x):
    """bf16 mode and every VGG block resolution a multiple of 32 pixels wide (W % 256, H % 32)."""
    return _is16() and x.dim() == 4 and x.shape[3] % 256 == 0 and x.shape[2] % 32 == 0


def _cb16_empty(N, C, H, W, like, dtype):
    return torch.empty((N, C // 16, H, W, 16), device=like.device, dtype=dtype)


def _vgg_wt(w, dgrad):
    """bf16 weights of a VGG conv swizzled into vconv3x3's LDS image (dsgan_vconv_wtrans), cached."""
    def build():
        Co, Ci = w.shape[0], w.shape[1]
        wt = torch.empty(_lib.load().dsgan_vconv_wtrans_size(Co, Ci), device=w.device, dtype=half_dtype())
        call("dsgan_vconv_wtrans", ptr(w), ptr(wt), Co, Ci, int(dgrad), stream())
        return wt
    return _cached(_WT_CACHE, w, ("vconv", dgrad, half_dtype()), build)


def _vconv(x, wt, bias, mask, y, N, K, M, H, W, relu, tag):
    with _timed(IGEMM_TIMER, _conv_flops(N, K, M, 3, 3, H, W), (tag, N, K, H, W, M, 3, 1), "vconv_kernel",
                _nb(x, wt, bias, mask, y)):
        call("dsgan_vconv3x3", ptr(x), ptr(wt), ptr(bias), ptr(mask), ptr(y), int(y.dtype == torch.float32), int(relu),
             N, K, M, H, W, stream())
    return y


def vgg_features_cb16(x, blocks, keep=False, real=None, outs=None, codes=None):
    """relu1_2..relu4_3 of x (NCHW fp32) as fp32 CB16 tensors; with keep, also per block (pool
    argmax or None, [bf16 CB16 outputs of the block's convs below the tapped one]) for the backward.
    real / outs: the real image's features -- every tap that is max-pooled also gets its perceptual
    L1 mean |f - real| into outs[tap] from the pool's read of f (dsgan_cb16_maxpool_l1), and with a
    `codes` dict its backward's per-element codes (sign(f - real), f > 0) in codes[tap]."""
    x, xbs = nchw(x)
    N, _, H, W = x.shape
    feats, saved = [], []
    h = None
    for bi, (pool, convs) in enumerate(blocks):
        idx = None
        if pool:
            f = feats[-1]
            C = f.shape[1] * 16
            H, W = H // 2, W // 2
            h = _cb16_empty(N, C, H, W, x, half_dtype())
            idx = torch.empty(h.shape, device=x.device, dtype=torch.uint8)
            if real is not None:
                tap = len(feats) - 1
                part = torch.empty(_lib.load().dsgan_cb16_maxpool_l1_parts(N, C, 2 * H, 2 * W), device=x.device,
                                   dtype=torch.float32)
                cd = None
                if codes is not None:
                    cd = torch.empty(f.shape, device=x.device, dtype=torch.uint8)
                    codes[tap] = cd
                call("dsgan_cb16_maxpool_l1", ptr(f), ptr(real[tap]), ptr(h), ptr(idx), ptr(cd), ptr(outs[tap:]),
                     *wsa(part), N, C, 2 * H, 2 * W, stream())
            else:
                call("dsgan_cb16_maxpool", ptr(f), ptr(h), ptr(idx), N, C, 2 * H, 2 * W, stream())
        acts = []
        for li, (w, b) in enumerate(convs):
            last = li == len(convs) - 1
            Co, Ci = w.shape[0], w.shape[1]
            y = _cb16_empty(N, Co, H, W, x, torch.float32 if last else half_dtype())
            if bi == 0 and li == 0:   # conv1_1, 3 -> 64: exact fp32 FMAs from the NCHW image
                call("dsgan_vgg_conv1_fwd", ptr(x), xbs, ptr(w), ptr(b), ptr(y), N, H, W, stream())
            else:
                _vconv(h, _vgg_wt(w, 0), b, None, y, N, Ci, Co, H, W, True, "fwd")
            if keep and not last:
                acts.append(y)
            h = y
        feats.append(h)
        saved.append((idx, acts))
    return feats, saved


def _perceptual_bwd_cb16(ctx, g):
    """Backward of PerceptualL1Fn over the CB16 pass: tap (L1 + pool backward) x ReLU', then each
    conv's data-grad x the ReLU' of the conv below in its epilogue, down to conv1_1's data-grad."""
    d, d_idx = None, None
    dx = None
    for bi in range(len(ctx.blocks) - 1, -1, -1):
        pool, convs = ctx.blocks[bi]
        idx, acts = ctx.saved[bi]
        f, r = ctx.feats[bi], ctx.real[bi]
        N, Cb, H, W, _ = r.shape
        dpre = _cb16_empty(N, Cb * 16, H, W, r, half_dtype())
        if bi in ctx.codes:
            call("dsgan_cb16_tap_bwd_codes", ptr(d), ptr(d_idx), ptr(ctx.codes[bi]), ptr(dpre), N, Cb * 16, H, W, ptr(g),
                 stream())
        else:
            call("dsgan_cb16_tap_bwd", ptr(d), ptr(d_idx), ptr(f), ptr(r), ptr(dpre), N, Cb * 16, H, W, ptr(g),
                 stream())
        for li in range(len(convs) - 1, -1, -1):
            w = convs[li][0]
            Co, Ci = w.shape[0], w.shape[1]
            if bi == 0 and li == 0:
                dx = torch.empty(ctx.fake_shape, device=r.device, dtype=torch.float32)
                call("dsgan_vgg_conv1_dgrad", ptr(dpre), ptr(w), ptr(dx), Ci * H * W, N, H, W, stream())
            else:
                out = _cb16_empty(N, Ci, H, W, r, half_dtype())
                _vconv(dpre, _vgg_wt(w, 1), None, acts[li - 1] if li > 0 else None, out, N, Co, Ci, H, W, False, "dgrad")
                dpre = out
        d, d_idx = dpre, idx
    return dx


def _sum4_raw(outs):
    """((L1(f1) + L1(f2)) + L1(f3)) + L1(f0) -- the reference's order -- in one dsgan_loss_combine
    launch (the fp32 adds of the three torch adds it replaces)."""
    xp = (ctypes.c_void_p * 4)(*[outs[i:].data_ptr() for i in (1, 2, 3, 0)])
    ones, zeros = (ctypes.c_float * 4)(1, 1, 1, 1), (ctypes.c_float * 4)(0, 0, 0, 0)
    out = torch.empty((), device=outs.device, dtype=torch.float32)
    call("dsgan_loss_combine", ctypes.cast(xp, ctypes.c_void_p), ctypes.cast(ones, ctypes.c_void_p),
         ctypes.cast(zeros, ctypes.c_void_p), ctypes.cast(ones, ctypes.c_void_p), 4, 1.0, ptr(out), stream())
    return out


# the perceptual L1 of each max-pooled VGG tap from the pool's read of it (dsgan_cb16_maxpool_l1);
# DSGAN_VGG_POOL_L1=0: the separate L1 pass (A/B runs)
VGG_POOL_L1 = [os.environ.get("DSGAN_VGG_POOL_L1", "1") != "0"]


def _record_all(obj, stream):
    """record_stream(stream) on every tensor in a nest of lists / tuples / dicts."""
    if torch.is_tensor(obj):
        obj.record_stream(stream)
    elif isinstance(obj, (list, tuple)):
        for o in obj:
            _record_all(o, stream)
    elif isinstance(obj, dict):
        for o in obj.values():
            _record_all(o, stream)


class PerceptualL1Fn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, fake, blocks, real_feats, side=None):
        if side is not None:
            # the forward's kernels on the side stream (the caller joins it before reading the loss);
            # the autograd node was created on the current stream, so the backward runs there, and
            # every tensor it or the caller reads is handed over to that stream
            main = torch.cuda.current_stream()
            side.wait_stream(main)
            with torch.cuda.stream(side):
                out = PerceptualL1Fn.forward(ctx, fake, blocks, real_feats)
            _record_all([out, ctx.saved, getattr(ctx, "feats", None), getattr(ctx, "codes", None)], main)
            return out
        ctx.box = _box(fake)
        fake, _ = nchw(fake)
        ctx.cb16 = real_feats[0].dim() == 5
        if ctx.cb16:
            # the L1 of every tap that is max-pooled comes from the pool's read of it; the others here
            outs = torch.empty(4, device=fake.device, dtype=torch.float32)
            fuse = VGG_POOL_L1[0]
            codes = {}
            feats, saved = vgg_features_cb16(fake, blocks, keep=True, real=real_feats if fuse else None, outs=outs,
                                             codes=codes)
            for i, (f, r) in enumerate(zip(feats, real_feats)):
                if i in codes:
                    continue
                call("dsgan_l1_fwd", ptr(f), ptr(r), f.numel(), ptr(outs[i:]), ptr(_loss_part(f)), stream())
            # a tap with codes needs neither its feature nor the real one in the backward
            feats = [None if i in codes else t for i, t in enumerate(feats)]
            ctx.blocks, ctx.saved, ctx.real, ctx.feats, ctx.codes = blocks, saved, real_feats, feats, codes
            ctx.fake_shape = tuple(fake.shape)
            ctx.prec = _state["prec"]
            return _sum4_raw(outs)
        feats, saved = vgg_features_raw(fake, blocks)
        outs = torch.empty(4, device=fake.device, dtype=torch.float32)
        for i, (f, r) in enumerate(zip(feats, real_feats)):
            call("dsgan_l1_fwd", ptr(f), ptr(r.contiguous()), f.numel(), ptr(outs[i:]), ptr(_loss_part(f)), stream())
        ctx.blocks, ctx.saved, ctx.real = blocks, saved, real_feats
        ctx.fake_shape = tuple(fake.shape)
        ctx.prec = _state["prec"]
        return _sum4_raw(outs)

    @staticmethod
    def backward(ctx, g):
        if ctx.cb16:
            with precision(ctx.prec):
                dx = _perceptual_bwd_cb16(ctx, g.contiguous())
            ctx.saved = ctx.real = ctx.feats = ctx.codes = None
            return _give(ctx.box, dx), None, None, None
        with precision(ctx.prec):
            g = g.contiguous()
            d, d_idx = None, None   # grad at the pool output of the block above, and that pool's argmax
            for bi in range(len(ctx.blocks) - 1, -1, -1):
                pool, convs = ctx.blocks[bi]
                idx, pin, ys = ctx.saved[bi]
                y_top = ys[-1]
                N, C, H, W = y_top.shape
                dpre = torch.empty_like(y_top)
                # tapped layer: (pool backward of the block above + L1 backward) * ReLU'
                call("dsgan_vgg_tap_bwd", ptr(d), ptr(d_idx), ptr(y_top), ptr(ctx.real[bi].contiguous()), ptr(dpre),
                     N * C, H, W, ptr(g), stream())
                for li in range(len(convs) - 1, -1, -1):
                    w = convs[li][0]
                    if li > 0:
                        # data-grad into the conv below, masked by that conv's ReLU in the epilogue
                        below = ys[li - 1]
                        dpre = conv_dgrad_raw(dpre, w, tuple(below.shape), 1, 1, gpre=below, gact="relu")
                    else:
                        in_shape = (pin[0], pin[1], pin[2] // 2, pin[3] // 2) if pool else ctx.fake_shape
                        dpre = conv_dgrad_raw(dpre, w, in_shape, 1, 1)
                d, d_idx = dpre, idx
            ctx.saved = ctx.real = None
            return _give(ctx.box, d), None, None, None


def perceptual_l1(fake, blocks, real_feats, side=None):
    """side (nullable torch.cuda.Stream): run the forward's kernels there -- the caller joins it before
    reading the loss -- while the backward stays on the current stream."""
    return PerceptualL1Fn.apply(fake, blocks, real_feats, side)


# ------------------------------------------------------------------------------------------
# MidMLKA tail (MixConvNeXtML.py:112-116):  out = GELU( IN( v * CA(v) ) + x )
# ------------------------------------------------------------------------------------------

class MidTailFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, v, x, w1, pa, w2):
        v4, vbs = nchw(v)
        N, C, H, W = v4.shape
        R = w1.shape[0]
        avg = torch.empty(N * C, device=v.device, dtype=torch.float32)
        mx = torch.empty_like(avg)
        amax = torch.empty(N * C, device=v.device, dtype=torch.int32)
        call("dsgan_plane_stats", ptr(v4), vbs, ptr(avg), ptr(mx), ptr(amax), N, C, H * W, stream())
        att = torch.empty(N * C, device=v.device, dtype=torch.float32)
        hsave = torch.empty(N * R * 2, device=v.device, dtype=torch.float32)
        call("dsgan_ca_fwd", ptr(avg), ptr(mx), ptr(w1), ptr(w2), ptr(pa), ptr(att), ptr(hsave), N, C, R, stream())
        y, mean, rstd = instnorm_raw(v4, att, x, "gelu")
        ctx.save_for_backward(v4, x, w1, pa, w2, avg, mx, amax, att, hsave, mean, rstd)
        ctx.refs = (w1, pa, w2)
        ctx.box_v, ctx.box_x = _box(v), _box(x)
        return y

    @staticmethod
    def backward(ctx, dy):
        v, x, w1, pa, w2, avg, mx, amax, att, hsave, mean, rstd = ctx.saved_tensors
        N, C, H, W = v.shape
        R = w1.shape[0]
        dv, dx, datt = instnorm_bwd_raw(dy, v, att, x, mean, rstd, "gelu", ctx.needs_input_grad[1], True)
        davg = torch.empty(N * C, device=v.device, dtype=torch.float32)
        dmx = torch.empty_like(davg)
        w1r, par, w2r = ctx.refs
        call("dsgan_ca_bwd", ptr(datt), ptr(att), ptr(avg), ptr(mx), ptr(hsave), ptr(w1), ptr(w2), ptr(pa),
             ptr(davg), ptr(dmx), ptr(_grad_buf(w1r)), ptr(_grad_buf(w2r)), ptr(_grad_buf(par)), N, C, R,
             *wsa(torch.empty(N * (2 * R * C + 1), device=v.device, dtype=torch.float32)), stream())
        call("dsgan_plane_stats_bwd", ptr(davg), ptr(dmx), ptr(amax), ptr(dv), C * H * W, N, C, H * W, stream())
        _params_done(*ctx.refs)
        return _give(ctx.box_v, dv), _give(ctx.box_x, dx), None, None, None


def mid_tail(v, x, w1, pa, w2):
    """w1: CA.fc1 weight [C/8, C, 1, 1], pa: PReLU weight [1], w2: CA.fc2 weight [C, C/8, 1, 1]."""
    return MidTailFn.apply(v, x, w1, pa, w2)


# ------------------------------------------------------------------------------------------
# n-ary add and channel concat
# ------------------------------------------------------------------------------------------

class AddNFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, *xs):
        ts = [nchw(t) for t in xs]
        N, C, H, W = ts[0][0].shape
        out = _empty(N, C, H, W, ts[0][0])
        arr = (ctypes.c_void_p * len(ts))(*[t.data_ptr() for t, _ in ts])
        bss = (ctypes.c_long * len(ts))(*[bs for _, bs in ts])
        call("dsgan_add_n", ctypes.cast(arr, ctypes.c_void_p), ctypes.cast(bss, ctypes.c_void_p), len(ts),
             ptr(out), C * H * W, N, C * H * W, stream())
        ctx.n = len(xs)
        ctx.boxes = [_box(t) for t in xs]
        return out

    @staticmethod
    def backward(ctx, dy):
        # the same dy goes to every input: a shared input may only borrow it
        return tuple(_give(b, dy, adopt=False) for b in ctx.boxes)


def add_n(*xs):
    return AddNFn.apply(*xs)


class CatFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, a, b):
        N, Ca, H, W = a.shape
        Cb = b.shape[1]
        out = _empty(N, Ca + Cb, H, W, a)
        copy_into(out[:, :Ca], a)
        copy_into(out[:, Ca:], b)
        ctx.Ca = Ca
        ctx.box_a, ctx.box_b = _box(a), _box(b)
        return out

    @staticmethod
    def backward(ctx, dy):
        # disjoint channel slices of dy: a shared input may adopt its slice as its buffer
        return _give(ctx.box_a, dy[:, :ctx.Ca]), _give(ctx.box_b, dy[:, ctx.Ca:])


def cat_channels(a, b):
    return CatFn.apply(a, b)


# ------------------------------------------------------------------------------------------
# Losses (0-d device tensors; backward reads the upstream grad from device memory)
# ------------------------------------------------------------------------------------------

def _loss_part(like):
    """Block-partial scratch of the deterministic loss reductions (dsgan_loss_parts floats)."""
    return torch.empty(_lib.load().dsgan_loss_parts(), device=like.device, dtype=torch.float32)


class BCELogitsFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, target):
        x = x.contiguous()
        out = torch.empty((), device=x.device, dtype=torch.float32)
        call("dsgan_bce_logits_fwd", ptr(x), x.numel(), float(target), ptr(out), ptr(_loss_part(x)), stream())
        ctx.target = float(target)
        ctx.save_for_backward(x)
        return out

    @staticmethod
    def backward(ctx, g):
        (x,) = ctx.saved_tensors
        dx = torch.empty_like(x)
        g = g.contiguous()
        call("dsgan_bce_logits_bwd", ptr(x), x.numel(), ctx.target, ptr(g), ptr(dx), 0, stream())
        return dx, None


def bce_with_logits(x, target):
    return BCELogitsFn.apply(x, target)


def _loss_grad(box, like, run):
    """Input-grad of a loss w.r.t. a (possibly shared, HF.share) image: a shared input whose buffer
    is owned and dense gets the grad accumulated in-kernel (run(buf, 1)); otherwise a fresh grad
    (run(d, 0)) is handed to the box or returned.  Either way the grads of a shared tensor are
    summed in arrival order, old + new, as autograd sums them."""
    buf, acc = _acc_target(box)
    if acc and buf.is_contiguous() and buf.shape == like.shape and buf.dtype == torch.float32:
        run(buf, 1)
        return None
    d = torch.empty_like(like)
    run(d, 0)
    return _give(box, d)


class L1Fn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, a, b):
        ctx.box_a, ctx.box_b = _box(a), _box(b)
        a, b = a.contiguous(), b.contiguous()
        out = torch.empty((), device=a.device, dtype=torch.float32)
        call("dsgan_l1_fwd", ptr(a), ptr(b), a.numel(), ptr(out), ptr(_loss_part(a)), stream())
        ctx.save_for_backward(a, b)
        return out

    @staticmethod
    def backward(ctx, g):
        a, b = ctx.saved_tensors
        g = g.contiguous()
        da = db = None
        if ctx.needs_input_grad[0]:
            da = _loss_grad(ctx.box_a, a, lambda d, acc: call("dsgan_l1_bwd", ptr(a), ptr(b), a.numel(), ptr(g),
                                                              ptr(d), acc, stream()))
        if ctx.needs_input_grad[1]:
            db = _loss_grad(ctx.box_b, b, lambda d, acc: call("dsgan_l1_bwd", ptr(b), ptr(a), b.numel(), ptr(g),
                                                              ptr(d), acc, stream()))
        return da, db


def l1_loss(a, b):
    return L1Fn.apply(a, b)


class TVFn(torch.autograd.Function):
    """(sum|dW| + sum|dH|) * coef over the whole batch (pix2pix_model.py:189-191, coef=1/(320*256))."""

    @staticmethod
    def forward(ctx, y, coef):
        ctx.box = _box(y)
        y = y.contiguous()
        N, C, H, W = y.shape
        out = torch.empty((), device=y.device, dtype=torch.float32)
        call("dsgan_tv_fwd", ptr(y), N * C, H, W, float(coef), ptr(out), ptr(_loss_part(y)), stream())
        ctx.coef = float(coef)
        ctx.save_for_backward(y)
        return out

    @staticmethod
    def backward(ctx, g):
        (y,) = ctx.saved_tensors
        N, C, H, W = y.shape
        g = g.contiguous()
        dy = _loss_grad(ctx.box, y, lambda d, acc: call("dsgan_tv_bwd", ptr(y), N * C, H, W, ctx.coef, ptr(g), ptr(d),
                                                        acc, stream()))
        return dy, None


def tv_loss(y, coef=1.0 / (320 * 256)):
    return TVFn.apply(y, coef)


class LossSumFn(torch.autograd.Function):
    """scale * sum_i a_i * (b_i + c_i * x_i) over 0-d fp32 losses in one launch each way
    (dsgan_loss_combine): the same fp32 roundings as the torch scalar-op chain it replaces, which
    costs one launch per multiply / add / rsub forward and per multiply backward."""

    @staticmethod
    def forward(ctx, coefs, scale, *xs):
        n = len(xs)
        fa = ctypes.c_float * n
        ctx.a = fa(*[float(a) for a, _, _ in coefs])
        ctx.c = fa(*[float(c) for _, _, c in coefs])
        ctx.scale = float(scale)
        b = fa(*[float(b) for _, b, _ in coefs])
        xp = (ctypes.c_void_p * n)(*[ptr(x) for x in xs])
        out = torch.empty((), device=xs[0].device, dtype=torch.float32)
        call("dsgan_loss_combine", ctypes.cast(xp, ctypes.c_void_p), ctypes.cast(ctx.a, ctypes.c_void_p),
             ctypes.cast(b, ctypes.c_void_p), ctypes.cast(ctx.c, ctypes.c_void_p), n, ctx.scale, ptr(out), stream())
        ctx.n = n
        return out

    @staticmethod
    def backward(ctx, g):
        gx = torch.empty(ctx.n, device=g.device, dtype=torch.float32)
        call("dsgan_loss_combine_bwd", ptr(g.contiguous()), ctypes.cast(ctx.a, ctypes.c_void_p),
             ctypes.cast(ctx.c, ctypes.c_void_p), ctx.n, ctx.scale, ptr(gx), stream())
        return (None, None) + tuple(gx[i] for i in range(ctx.n))


def loss_sum(terms, scale=1.0):
    """scale * (t_0 + t_1 + ...), t_i = a * (b + c * x) for terms (x, a[, b, c]) with c = +-1, summed
    left to right -- e.g. ``loss_sum([(gan, w_gan), (l1, 1), (ssim, w_ss, 1, -1)])`` is
    ``gan * w_gan + l1 + w_ss * (1 - ssim)`` rounded as torch rounds that expression.  Terms whose x
    is a python 0 (a disabled loss) are dropped, as ``0 * w + t`` is t."""
    xs, coefs = [], []
    for t in terms:
        x, a = t[0], t[1]
        b, c = (t[2], t[3]) if len(t) > 2 else (0.0, 1.0)
        if not torch.is_tensor(x):
            if x == 0 and b == 0:
                continue
            raise ValueError("loss_sum: non-tensor term %r" % (x,))
        if x.dim() != 0 or x.dtype != torch.float32 or not x.is_cuda or c not in (1, -1, 1.0, -1.0):
            raise ValueError("loss_sum: 0-d fp32 device losses and c = +-1 only")
        xs.append(x)
        coefs.append((a, b, c))
    if not xs or len(xs) > 8:
        raise ValueError("loss_sum: 1..8 tensor terms")
    return LossSumFn.apply(tuple(coefs), scale, *xs)


_WIN_CACHE = {}


def gauss_win(device, size=11, sigma=1.5):
    """_fspecial_gauss_1d (DSGAN/MS_SSIM.py:9-23), built in fp32 on the host, cached on device."""
    key = (str(device), size, sigma)
    if key not in _WIN_CACHE:
        c = torch.arange(size, dtype=torch.float) - size // 2
        g = torch.exp(-(c ** 2) / (2 * sigma ** 2))
        _WIN_CACHE[key] = (g / g.sum()).to(device)
    return _WIN_CACHE[key]


class SSIMFn(torch.autograd.Function):
    """mean SSIM of (a*real+b, a*fake+b) with data_range 1 (MS_SSIM.py:95-150); grad w.r.t. fake."""

    @staticmethod
    def forward(ctx, real, fake, a, b, data_range):
        ctx.box = _box(fake)
        real, fake = real.contiguous(), fake.contiguous()
        N, C, H, W = real.shape
        Ho, Wo = H - 10, W - 10
        coef = torch.empty((3, N * C, Ho, Wo), device=real.device, dtype=torch.float32)
        s = torch.empty((), device=real.device, dtype=torch.float32)
        win = gauss_win(real.device)
        C1 = (0.01 * data_range) ** 2
        C2 = (0.03 * data_range) ** 2
        part = torch.empty(_lib.load().dsgan_ssim_parts(N * C, H, W), device=real.device, dtype=torch.float32)
        call("dsgan_ssim_fwd", ptr(real), ptr(fake), float(a), float(b), N * C, H, W, ptr(win),
             float(C1), float(C2), ptr(coef), ptr(s), ptr(part), stream())
        cnt = float(N * C * Ho * Wo)
        ctx.save_for_backward(real, fake, coef)
        ctx.ab, ctx.cnt = (float(a), float(b)), cnt
        return s / cnt

    @staticmethod
    def backward(ctx, g):
        real, fake, coef = ctx.saved_tensors
        N, C, H, W = real.shape
        g = g.contiguous()
        dfake = _loss_grad(ctx.box, fake, lambda d, acc: call(
            "dsgan_ssim_bwd", ptr(real), ptr(fake), ctx.ab[0], ctx.ab[1], N * C, H, W, ptr(gauss_win(real.device)),
            ptr(coef), ptr(g), 1.0 / ctx.cnt, ptr(d), acc, stream()))
        return None, dfake, None, None, None


def ssim_affine(real, fake, a=0.5, b=0.5, data_range=1.0):
    return SSIMFn.apply(real, fake, a, b, data_range)


MS_SSIM_WEIGHTS = (0.0448, 0.2856, 0.3001, 0.2363, 0.1333)


def ms_ssim_affine(real, fake, a=1.0, b=0.0, data_range=1.0, weights=MS_SSIM_WEIGHTS, size_average=True):
    """MS-SSIM of (a*real+b, a*fake+b) (DSGAN/MS_SSIM.py:153-225), evaluation only (no autograd):
    a 0-d tensor (size_average) or the per-image values [N]."""
    real, fake = real.detach().contiguous(), fake.detach().contiguous()
    if real.shape != fake.shape or real.dim() != 4:
        raise ValueError("ms_ssim: two (N,C,H,W) tensors of the same shape required")
    N, C, H, W = real.shape
    work = _ws("dsgan_ms_ssim_workspace", N, C, H, W, like=real)
    stats = torch.empty(2 * len(weights) * N * C, device=real.device, dtype=torch.float32)
    out = torch.empty(N + 1, device=real.device, dtype=torch.float32)
    wh = (ctypes.c_float * len(weights))(*[float(w) for w in weights])
    C1 = (0.01 * data_range) ** 2
    C2 = (0.03 * data_range) ** 2
    call("dsgan_ms_ssim", ptr(real), ptr(fake), float(a), float(b), N, C, H, W, ptr(gauss_win(real.device)),
         float(C1), float(C2), ctypes.cast(wh, ctypes.c_void_p), len(weights), *wsa(work), ptr(stats), ptr(out),
         stream())
    return out[N] if size_average else out[:N]


class MSSSIMFn(torch.autograd.Function):
    """Batch-mean MS-SSIM of (a*real+b, a*fake+b) (DSGAN/MS_SSIM.py:153-225, size_average=True)
    as a loss term: gradient w.r.t. fake through the 5-level pyramid (losses.hip)."""

    @staticmethod
    def forward(ctx, real, fake, a, b, data_range, weights):
        real, fake = real.contiguous(), fake.contiguous()
        if real.shape != fake.shape or real.dim() != 4:
            raise ValueError("ms_ssim: two (N,C,H,W) tensors of the same shape required")
        N, C, H, W = real.shape
        L = len(weights)
        work = _ws("dsgan_ms_ssim_train_workspace", N, C, H, W, L, like=real)
        stats = torch.empty(2 * L * N * C, device=real.device, dtype=torch.float32)
        out = torch.empty(N + 1, device=real.device, dtype=torch.float32)
        wh = (ctypes.c_float * L)(*[float(w) for w in weights])
        C1, C2 = (0.01 * data_range) ** 2, (0.03 * data_range) ** 2
        call("dsgan_ms_ssim_fwd_train", ptr(real), ptr(fake), float(a), float(b), N, C, H, W,
             ptr(gauss_win(real.device)), float(C1), float(C2), ctypes.cast(wh, ctypes.c_void_p), L, *wsa(work),
             ptr(stats), ptr(out), stream())
        ctx.save_for_backward(real, fake, work, stats)
        ctx.args = (float(a), float(b), float(C1), float(C2), tuple(float(w) for w in weights))
        return out[N]

    @staticmethod
    def backward(ctx, g):
        real, fake, work, stats = ctx.saved_tensors
        a, b, C1, C2, weights = ctx.args
        N, C, H, W = real.shape
        wh = (ctypes.c_float * len(weights))(*weights)
        dfake = torch.empty_like(fake)
        call("dsgan_ms_ssim_bwd", ptr(real), ptr(fake), a, b, N, C, H, W, ptr(gauss_win(real.device)), C1, C2,
             ctypes.cast(wh, ctypes.c_void_p), len(weights), *wsa(work), ptr(stats), ptr(g.contiguous()), ptr(dfake),
             0, stream())
        return None, dfake, None, None, None, None


def ms_ssim_loss_affine(real, fake, a=0.5, b=0.5, data_range=1.0, weights=MS_SSIM_WEIGHTS):
    """Differentiable batch-mean MS-SSIM of (a*real+b, a*fake+b); gradient w.r.t. fake only."""
    return MSSSIMFn.apply(real, fake, a, b, data_range, tuple(weights))


# ------------------------------------------------------------------------------------------
# Test-set evaluation (evalimg.hip): no autograd, no host sync -- every call only enqueues work
# ------------------------------------------------------------------------------------------

def _eval4(*ts):
    """Detached contiguous fp32 (N,C,H,W) operands of one shape."""
    out = [t.detach().contiguous() for t in ts]
    if any(t.dim() != 4 or t.dtype != torch.float32 or t.shape != out[0].shape for t in out):
        raise ValueError("expected fp32 (N,C,H,W) tensors of one shape, got %s" % ([tuple(t.shape) for t in out],))
    return out


def img_metrics_batch(fake, real):
    """[N,2] = (skimage-style SSIM, PSNR) of every image pair of two [N,C,H,W] batches in [-1, 1]:
    per image what ``dsgan_img_metrics`` (util.metrics.TrainMetrics) computes for one."""
    fake, real = _eval4(fake, real)
    N, C, H, W = fake.shape
    out = torch.empty((N, 2), device=fake.device, dtype=torch.float32)
    n = _lib.load().dsgan_img_metrics_batch_parts(N, C, H, W)
    part = torch.empty(max(n, 1), device=fake.device, dtype=torch.float64)
    call("dsgan_img_metrics_batch", ptr(fake), ptr(real), N, C, H, W, ptr(part), ptr(out), stream())
    return out


def images_to_u8(*imgs):
    """uint8 [N,H,k*W,3]: one to three [N,C,H,W] batches in [-1, 1] (C 1 or 3, a one-channel image
    repeated to three) side by side as the reference's uint8 HWC images (train.py:110-128)."""
    if not 1 <= len(imgs) <= 3:
        raise ValueError("images_to_u8 takes one to three image batches")
    imgs = [t.detach().contiguous() for t in imgs]
    N, _, H, W = imgs[0].shape
    for t in imgs:
        if t.dim() != 4 or t.dtype != torch.float32 or (t.shape[0], t.shape[2], t.shape[3]) != (N, H, W):
            raise ValueError("images_to_u8: fp32 (N,C,H,W) batches of one N, H, W required")
    out = torch.empty((N, H, len(imgs) * W, 3), device=imgs[0].device, dtype=torch.uint8)
    args = []
    for i in range(3):
        args += [ptr(imgs[i]), int(imgs[i].shape[1])] if i < len(imgs) else [None, 0]
    call("dsgan_images_to_u8", *args, N, H, W, ptr(out), stream())
    return out


def _origins(oy, ox, dev):
    """The two device int32 origin arrays of a tile plan (a TilePlan's, or anything as_tensor takes)."""
    out = []
    for o in (oy, ox):
        o = torch.as_tensor(o, dtype=torch.int32).to(dev).contiguous()
        if o.dim() != 1 or o.numel() == 0:
            raise ValueError("tile origins: a non-empty 1-D list per axis, got shape %s" % (tuple(o.shape),))
        out.append(o)
    return out


def u8_tiles(frame_u8, oy, ox, th, tw, t0=0, T=None, gray=False):
    """fp32 [T, 3|1, th, tw]: tiles t0 .. t0+T-1 (t = iy*nx + ix, corner (oy[iy], ox[ix])) of one uint8
    [H, W, 3] device frame, converted as ``data.to_images`` converts a crop (bit-exact, no flip)."""
    if frame_u8.dim() != 3 or frame_u8.shape[2] != 3 or frame_u8.dtype != torch.uint8:
        raise ValueError("u8_tiles: a uint8 (H,W,3) frame required, got %s %s" % (tuple(frame_u8.shape), frame_u8.dtype))
    frame_u8 = frame_u8.contiguous()
    oy, ox = _origins(oy, ox, frame_u8.device)
    H, W, _ = frame_u8.shape
    T = oy.numel() * ox.numel() - t0 if T is None else int(T)
    out = torch.empty((max(T, 0), 1 if gray else 3, int(th), int(tw)), device=frame_u8.device, dtype=torch.float32)
    call("dsgan_u8_tiles", ptr(frame_u8), H, W, ptr(oy), oy.numel(), ptr(ox), ox.numel(), int(th), int(tw), int(t0), T,
         int(bool(gray)), ptr(out), stream())
    return out


def tiles_blend(tiles, oy, ox, overlap, H, W):
    """fp32 [C, H, W]: the [ny*nx, C, th, tw] tiles of a plan blended into one frame.  Every pixel is the
    mean of the tiles that cover it under the integer ramp weight w1(y-oy) * w1(x-ox), w1(i) = min(i+1, L-i,
    overlap), summed iy then ix ascending in fp32 (``dsgan_tiles_blend``); a pixel one tile covers is that
    tile's value bit for bit."""
    if tiles.dim() != 4 or tiles.dtype != torch.float32:
        raise ValueError("tiles_blend: fp32 (T,C,th,tw) tiles required, got %s %s" % (tuple(tiles.shape), tiles.dtype))
    tiles = tiles.detach().contiguous()
    oy, ox = _origins(oy, ox, tiles.device)
    T, C, th, tw = tiles.shape
    if T != oy.numel() * ox.numel():
        raise ValueError("tiles_blend: %d tiles for a %d x %d plan" % (T, oy.numel(), ox.numel()))
    out = torch.empty((C, max(int(H), 0), max(int(W), 0)), device=tiles.device, dtype=torch.float32)
    call("dsgan_tiles_blend", ptr(tiles), C, th, tw, ptr(oy), oy.numel(), ptr(ox), ox.numel(), int(overlap), int(H), int(W),
         ptr(out), stream())
    return out


def ssim_eval_affine(real, fake, a=0.5, b=0.5, data_range=1.0, size_average=True, nonnegative=False):
    """Gaussian SSIM of (a*real+b, a*fake+b) (DSGAN/MS_SSIM.py:95-150), evaluation only: the per-image
    values [N] (channel mean of the plane means, relu'd per plane when ``nonnegative``) or their mean."""
    real, fake = _eval4(real, fake)
    N, C, H, W = real.shape
    n = _lib.load().dsgan_ssim_eval_parts(N, C, H, W)
    part = torch.empty(max(n, 1), device=real.device, dtype=torch.float32)
    out = torch.empty(N + 1, device=real.device, dtype=torch.float32)
    C1, C2 = (0.01 * data_range) ** 2, (0.03 * data_range) ** 2
    call("dsgan_ssim_eval", ptr(real), ptr(fake), float(a), float(b), N, C, H, W, ptr(gauss_win(real.device)),
         float(C1), float(C2), int(bool(nonnegative)), ptr(part), ptr(out), stream())
    return out[N] if size_average else out[:N]


# ------------------------------------------------------------------------------------------
# LSGAN objective (--no_lsgan, quirk q3) and the multi-scale D's input pyramid (lsgan.hip)
# ------------------------------------------------------------------------------------------

class SigmoidFn(torch.autograd.Function):
    """nn.Sigmoid in fp32 with the accurate exp (a loss input, not a gate); the backward reads the
    saved output, as torch's does."""

    @staticmethod
    def forward(ctx, x):
        x = x.contiguous()
        y = torch.empty_like(x)
        with _timed(AUX_TIMER, 0.0, ("sigmoid_fwd", x.numel()), "sigmoid", _nb(x, y)):
            call("dsgan_sigmoid_fwd", ptr(x), x.numel(), ptr(y), stream())
        ctx.save_for_backward(y)
        return y

    @staticmethod
    def backward(ctx, dy):
        (y,) = ctx.saved_tensors
        dy = dy.contiguous()
        dx = torch.empty_like(y)
        with _timed(AUX_TIMER, 0.0, ("sigmoid_bwd", y.numel()), "sigmoid", _nb(y, dy, dx)):
            call("dsgan_sigmoid_bwd", ptr(y), ptr(dy), y.numel(), ptr(dx), 0, stream())
        return dx


def sigmoid(x):
    return SigmoidFn.apply(x)


class MseConstFn(torch.autograd.Function):
    """mean((x - target)^2) against a constant label (nn.MSELoss of GANLoss / GANLoss_multi)."""

    @staticmethod
    def forward(ctx, x, target):
        ctx.box = _box(x)
        x = x.contiguous()
        out = torch.empty((), device=x.device, dtype=torch.float32)
        with _timed(AUX_TIMER, 0.0, ("mse_fwd", x.numel()), "mse_const", _nb(x)):
            call("dsgan_mse_const_fwd", ptr(x), x.numel(), float(target), ptr(out), ptr(_loss_part(x)), stream())
        ctx.target = float(target)
        ctx.save_for_backward(x)
        return out

    @staticmethod
    def backward(ctx, g):
        (x,) = ctx.saved_tensors
        g = g.contiguous()

        def run(d, acc):
            with _timed(AUX_TIMER, 0.0, ("mse_bwd", x.numel()), "mse_const", _nb(x, d) + (_nb(d) if acc else 0.0)):
                call("dsgan_mse_const_bwd", ptr(x), x.numel(), ctx.target, ptr(g), ptr(d), acc, stream())
        return _loss_grad(ctx.box, x, run), None


def mse_const(x, target):
    return MseConstFn.apply(x, target)


# AvgPool2d(3, 2, 1, count_include_pad=False) on the 16-byte form where it applies (off: the scalar
# form everywhere; tests / A-B -- the two give the same bits)
AVGPOOL_FAST = [True]


def avg_pool3s2_raw(x, out=None):
    x, xbs = nchw(x)
    N, C, H, W = x.shape
    y = out if out is not None else _empty(N, C, (H - 1) // 2 + 1, (W - 1) // 2 + 1, x)
    y, ybs = nchw(y)
    with _timed(AUX_TIMER, 0.0, ("avgpool_fwd", N, C, H, W), "avgpool3s2", _nb(x, y)):
        call("dsgan_avgpool3s2_fwd", ptr(x), xbs, ptr(y), ybs, N, C, H, W, 0 if AVGPOOL_FAST[0] else 1, stream())
    return y


def avg_pool3s2_bwd_raw(dy, x_shape, out=None, accumulate=False):
    dy, dybs = nchw(dy)
    N, C, H, W = x_shape
    dx = out if out is not None else torch.empty((N, C, H, W), device=dy.device, dtype=torch.float32)
    dx4, dxbs = nchw(dx)
    if dx4.data_ptr() != dx.data_ptr():
        raise RuntimeError("avg_pool3s2: gradient target is not NCHW-dense")
    with _timed(AUX_TIMER, 0.0, ("avgpool_bwd", N, C, H, W), "avgpool3s2", _nb(dy, dx) + (_nb(dx) if accumulate else 0.0)):
        call("dsgan_avgpool3s2_bwd", ptr(dy), dybs, ptr(dx), dxbs, N, C, H, W, int(accumulate),
             0 if AVGPOOL_FAST[0] else 1, stream())
    return dx


class AvgPool3s2Fn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x):
        ctx.box = _box(x)
        ctx.x_shape = tuple(x.shape)
        return avg_pool3s2_raw(x)

    @staticmethod
    def backward(ctx, dy):
        buf, acc = _acc_target(ctx.box)
        if acc and buf.dtype == torch.float32 and tuple(buf.shape) == ctx.x_shape and nchw(buf)[0] is buf:
            avg_pool3s2_bwd_raw(dy, ctx.x_shape, out=buf, accumulate=True)   # a shared input: old + new in-kernel
            return None
        return _give(ctx.box, avg_pool3s2_bwd_raw(dy, ctx.x_shape))


def avg_pool3s2(x):
    """AvgPool2d(3, stride=2, padding=1, count_include_pad=False) (MultiscaleDiscriminator.downsample)."""
    return AvgPool3s2Fn.apply(x)


# ------------------------------------------------------------------------------------------
# U-Net generator glue (unet.hip; DSGAN/models/networks.py:445-529): ConvTranspose2d 4x4/s2/p1,
# nn.PReLU() over a channel concatenation, nn.Dropout from a counter-based generator, nn.Tanh
# ------------------------------------------------------------------------------------------

# ConvTranspose2d(k4, s2, p1) doubles the plane exactly as (k3, s2, p1, op1) does, and ConvT3s2Fn reads
# the kernel size off the weight: forward conv_dgrad_raw(.., 2, 1, bias), backward conv_fwd_raw(dy, w,
# None, 2, 1), conv_wgrad_raw(x, dy, gw, 2, 1), channel_sum_raw.
ConvT4s2Fn = ConvT3s2Fn


def conv_transpose4s2(x, w, b=None):
    """nn.ConvTranspose2d(Cin, Cout, kernel_size=4, stride=2, padding=1): w is [Cin, Cout, 4, 4]."""
    if w.dim() != 4 or tuple(w.shape[2:]) != (4, 4) or w.shape[0] != x.shape[1]:
        raise ValueError("conv_transpose4s2: weight %s does not fit input %s" % (tuple(w.shape), tuple(x.shape)))
    return ConvT4s2Fn.apply(x, w, b)


def _dense4(t, what):
    """(t, batch stride) of a per-sample dense NCHW tensor a kernel writes into."""
    t4, bs = nchw(t)
    if t4.data_ptr() != t.data_ptr():
        raise ValueError("%s: destination must be per-sample dense" % what)
    return t4, bs


class PReluCatFn(torch.autograd.Function):
    """y = prelu(cat(a, b), weight) for an ``nn.PReLU()`` weight of one element (b None: prelu(a)).
    The halves are read where they lie (own batch strides, e.g. a CatSlot's head and tail), the slope
    from device memory.  The backward writes both input grads into one buffer (its channel slices are
    da / db) and adds the slope's gradient into ``weight.grad`` through block partials summed in a
    fixed order."""

    @staticmethod
    def forward(ctx, a, b, weight, out):
        if weight.numel() != 1:
            raise NotImplementedError("prelu: one slope (nn.PReLU(num_parameters=1)) only")
        ctx.box_a, ctx.box_b = _box(a), (_box(b) if b is not None else None)
        a, abs_ = nchw(a)
        N, Ca, H, W = a.shape
        Cb, bbs = 0, 0
        if b is not None:
            b, bbs = nchw(b)
            if b.shape[0] != N or tuple(b.shape[2:]) != (H, W):
                raise ValueError("prelu_cat: %s and %s do not concatenate" % (tuple(a.shape), tuple(b.shape)))
            Cb = b.shape[1]
        y = out if out is not None else _empty(N, Ca + Cb, H, W, a)
        if tuple(y.shape) != (N, Ca + Cb, H, W):
            raise ValueError("prelu_cat: out has shape %s" % (tuple(y.shape),))
        y, ybs = _dense4(y, "prelu_cat")
        with _timed(AUX_TIMER, 0.0, ("prelu_fwd", N, Ca, Cb, H, W), "prelu", 2 * _nb(y)):
            call("dsgan_prelu_fwd", ptr(a), abs_, Ca * H * W, ptr(b), bbs, Cb * H * W, ptr(weight), ptr(y), ybs, N,
                 stream())
        ctx.save_for_backward(a, b, weight)
        ctx.w_ref = weight
        return y

    @staticmethod
    def backward(ctx, dy):
        a, b, weight = ctx.saved_tensors
        dy, dybs = nchw(dy)
        N, Ca, H, W = a.shape
        Cb = b.shape[1] if b is not None else 0
        E = (Ca + Cb) * H * W
        d = _empty(N, Ca + Cb, H, W, dy)
        da, db = (d[:, :Ca], d[:, Ca:]) if b is not None else (d, None)
        gw = _grad_buf(ctx.w_ref) if ctx.needs_input_grad[2] else None
        with _timed(AUX_TIMER, 0.0, ("prelu_bwd", N, Ca, Cb, H, W), "prelu", 3 * _nb(d)):
            call("dsgan_prelu_bwd", ptr(dy), dybs, ptr(a), nchw(a)[1], Ca * H * W, ptr(b),
                 nchw(b)[1] if b is not None else 0, Cb * H * W, ptr(weight), ptr(da), E, ptr(db), E, ptr(gw), N,
                 *wsa(_ws("dsgan_prelu_workspace", N, E, like=dy)), stream())
        _params_done(ctx.w_ref)
        return _give(ctx.box_a, da), (_give(ctx.box_b, db) if b is not None else None), None, None


def prelu_cat(a, b, prelu_weight, out=None):
    """``prelu(cat(a, b))`` with the learnable slope ``prelu_weight`` (pass the Parameter itself)."""
    return PReluCatFn.apply(a, b, prelu_weight, out)


def prelu(x, prelu_weight, out=None):
    return PReluCatFn.apply(x, None, prelu_weight, out)


class DropoutState:
    """What fixes a dropout layer's masks: the 64-bit ``seed``, the ``stream`` id of the layer (the
    rank is folded into it) and ``counter``, an int64 device tensor of one element that the forward
    kernel advances -- a captured graph draws a fresh mask on every replay, nothing touches the host.
    Call k of the layer drops element i iff word (i & 3) of Philox-4x32-10(key = seed, counter =
    (i >> 2, k, stream)) is below round(p * 2^32)."""
    __slots__ = ("seed", "stream", "counter")

    def __init__(self, seed, stream, counter):
        self.seed, self.stream, self.counter = int(seed) & (2 ** 63 - 1), int(stream), counter
        if not 0 <= self.stream < 2 ** 32:
            raise ValueError("DropoutState: stream id out of range")
        if counter.dtype != torch.int64 or counter.numel() != 1:
            raise ValueError("DropoutState: counter must be an int64 tensor of one element")


def _dropout_thresh(p):
    p = float(p)
    if not 0.0 <= p < 1.0:
        raise ValueError("dropout: p must be in [0, 1), got %r" % p)
    return int(round(p * 2.0 ** 32))


class DropoutFn(torch.autograd.Function):
    """y = x * mask / (1 - p).  No mask tensor: the backward regenerates it from the call counter the
    forward drew (a one-element device tensor)."""

    @staticmethod
    def forward(ctx, x, p, state, out):
        ctx.box = _box(x)
        x, xbs = nchw(x)
        N, C, H, W = x.shape
        y = out if out is not None else _empty(N, C, H, W, x)
        y, ybs = _dense4(y, "dropout")
        used = torch.empty(1, device=x.device, dtype=torch.int64)
        ctx.args = (N, C * H * W, state.seed, state.stream, _dropout_thresh(p), 1.0 / (1.0 - float(p)))
        N, E, seed, sid, thresh, scale = ctx.args
        with _timed(AUX_TIMER, 0.0, ("dropout_fwd", N, C, H, W), "dropout", 2 * _nb(x)):
            call("dsgan_dropout_fwd", ptr(x), xbs, ptr(y), ybs, N, E, seed, sid, ptr(state.counter), ptr(used), thresh,
                 scale, stream())
        ctx.save_for_backward(used)
        ctx.shape = (N, C, H, W)
        return y

    @staticmethod
    def backward(ctx, dy):
        (used,) = ctx.saved_tensors
        dy, dybs = nchw(dy)
        N, E, seed, sid, thresh, scale = ctx.args
        dx = _empty(*ctx.shape, dy)
        with _timed(AUX_TIMER, 0.0, ("dropout_bwd",) + ctx.shape, "dropout", 2 * _nb(dx)):
            call("dsgan_dropout_apply", ptr(dy), dybs, ptr(dx), E, N, E, seed, sid, ptr(used), 0, thresh, scale,
                 stream())
        return _give(ctx.box, dx), None, None, None


def dropout(x, p, state, training, out=None):
    """nn.Dropout(p) with the masks of ``state`` (a DropoutState).  Eval mode is the identity and
    leaves the counter alone.  ``out``: a per-sample dense destination (e.g. a CatSlot's tail)."""
    if not training or float(p) == 0.0:
        if out is None:
            return x
        if torch.is_grad_enabled() and x.requires_grad:
            raise NotImplementedError("dropout: eval mode into `out` is a plain copy and records no gradient")
        copy_into(out, x)
        return out
    return DropoutFn.apply(x, p, state, out)


def dropout_mask(shape, seed, stream_id, counter, p=0.5, device="cuda"):
    """The 0/1 mask (fp32, ``shape``) the dropout kernels use for call ``counter`` of the layer
    (seed, stream_id): 1 where the element is kept."""
    shape = tuple(int(s) for s in shape)
    m = torch.empty(shape, device=device, dtype=torch.float32)
    N = shape[0] if len(shape) > 1 else 1
    E = m.numel() // N
    call("dsgan_dropout_apply", None, 0, ptr(m), E, N, E, int(seed) & (2 ** 63 - 1), int(stream_id), None, int(counter),
         _dropout_thresh(p), 1.0, stream())
    return m


class TanhFn(torch.autograd.Function):
    """nn.Tanh in fp32; the backward reads the saved output, dx = dy * (1 - y^2), as torch's does."""

    @staticmethod
    def forward(ctx, x):
        ctx.box = _box(x)
        x = x.contiguous()
        y = torch.empty_like(x)
        with _timed(AUX_TIMER, 0.0, ("tanh_fwd", x.numel()), "tanh", _nb(x, y)):
            call("dsgan_tanh_fwd", ptr(x), x.numel(), ptr(y), stream())
        ctx.save_for_backward(y)
        return y

    @staticmethod
    def backward(ctx, dy):
        (y,) = ctx.saved_tensors
        dy = dy.contiguous()
        dx = torch.empty_like(y)
        with _timed(AUX_TIMER, 0.0, ("tanh_bwd", y.numel()), "tanh", _nb(y, dy, dx)):
            call("dsgan_tanh_bwd", ptr(y), ptr(dy), y.numel(), ptr(dx), 0, stream())
        return _give(ctx.box, dx)


def tanh(x):
    return TanhFn.apply(x)


# ------------------------------------------------------------------------------------------
# Differentiable augmentation of the D input (--diffaug; csrc/diffaug.hip, restated in diffaug.py)
# ------------------------------------------------------------------------------------------

class DiffAugState:
    """What fixes the augmentation's draws: the 64-bit ``seed``, the ``stream`` id (the rank is folded
    into it) and ``counter``, an int64 device tensor of one element that the forward advances by the
    number of calls it draws -- a captured graph augments afresh on every replay.  Sample i of call k
    draws Philox-4x32-10(key = seed, counter = (i, 0 / 1, k, stream)): see dsgan_hip.diffaug."""
    __slots__ = ("seed", "stream", "counter")

    def __init__(self, seed, stream, counter):
        self.seed, self.stream, self.counter = int(seed) & (2 ** 63 - 1), int(stream), counter
        if not 0 <= self.stream < 2 ** 32:
            raise ValueError("DiffAugState: stream id out of range")
        if counter.dtype != torch.int64 or counter.numel() != 1:
            raise ValueError("DiffAugState: counter must be an int64 tensor of one element")


class DiffAugFn(torch.autograd.Function):
    """y = augment(cat(a, b)) in one pass over a and b (a None: the image alone).  Linear in b once the
    parameters are drawn: nothing is saved but the call counter drawn, and the backward regenerates
    the parameters from it.  The condition ``a`` gets no gradient."""

    @staticmethod
    def forward(ctx, a, b, bits, state, group, out):
        ctx.box_b = _box(b)
        b, bbs = nchw(b)
        N, Cb, H, W = b.shape
        Ca, abs_ = 0, 0
        if a is not None:
            a, abs_ = nchw(a)
            if a.shape[0] != N or tuple(a.shape[2:]) != (H, W):
                raise ValueError("diffaug_cat: %s and %s do not concatenate" % (tuple(a.shape), tuple(b.shape)))
            Ca = a.shape[1]
        group = N if group is None else int(group)
        y = out if out is not None else _empty(N, Ca + Cb, H, W, b)
        if tuple(y.shape) != (N, Ca + Cb, H, W):
            raise ValueError("diffaug_cat: out has shape %s" % (tuple(y.shape),))
        y, ybs = _dense4(y, "diffaug_cat")
        used = torch.empty(1, device=b.device, dtype=torch.int64)
        ctx.args = (N, Ca, Cb, H, W, int(bits), state.seed, state.stream, group)
        with _timed(AUX_TIMER, 0.0, ("diffaug_fwd", N, Ca, Cb, H, W, int(bits)), "diffaug",
                    2 * _nb(y) + (_nb(b) if bits & 1 else 0.0)):
            call("dsgan_diffaug_fwd", ptr(a), abs_, ptr(b), bbs, ptr(y), ybs, N, Ca, Cb, H, W, int(bits), state.seed,
                 state.stream, ptr(state.counter), ptr(used), group,
                 *wsa(_ws("dsgan_diffaug_workspace", N, Cb, H, W, like=b) if bits & 1 else None), stream())
        ctx.save_for_backward(used)
        return y

    @staticmethod
    def backward(ctx, dy):
        if not ctx.needs_input_grad[1]:
            return None, None, None, None, None, None
        (used,) = ctx.saved_tensors
        N, Ca, Cb, H, W, bits, seed, sid, group = ctx.args
        dy, dybs = nchw(dy)
        dx = _empty(N, Cb, H, W, dy)
        with _timed(AUX_TIMER, 0.0, ("diffaug_bwd", N, Ca, Cb, H, W, bits), "diffaug",
                    (2 + (bits & 1)) * _nb(dx)):
            call("dsgan_diffaug_bwd", ptr(dy), dybs, ptr(dx), Cb * H * W, N, Ca, Cb, H, W, bits, seed, sid, ptr(used),
                 group, *wsa(_ws("dsgan_diffaug_workspace", N, Cb, H, W, like=dy) if bits & 1 else None), stream())
        return None, _give(ctx.box_b, dx), None, None, None, None


def diffaug_cat(a, b, policy, state, group=None, out=None):
    """The augmented channel concatenation cat(a, b) [N, Ca+Cb, H, W] for the discriminator (``a`` None:
    ``b`` alone).  ``policy``: a --diffaug string or parse_policy's tuple; ``state``: a DiffAugState.
    Sample n belongs to call ``counter + n // group`` with index ``n % group`` (group None: N, one call),
    and the counter advances by ceil(N / group).  ``out``: a per-sample dense destination (e.g. a half
    of a stacked batch); it may not overlap ``a`` or ``b`` (refused by the library)."""
    from . import diffaug as _da
    bits = _da.policy_bits(policy)
    if bits == 0:
        raise ValueError("diffaug_cat: empty policy (use cat_channels)")
    return DiffAugFn.apply(a, b, bits, state, group, out)


def diffaug_params(seed, stream_id, call_index, n, H, W, device="cuda"):
    """The draws the kernels make for samples 0..n-1 of call ``call_index``: diffaug.draw_params' dict,
    computed on the device (dsgan_diffaug_params)."""
    from . import diffaug as _da
    t = torch.empty((int(n), 8), device=device, dtype=torch.float32)
    call("dsgan_diffaug_params", ptr(t), int(n), int(seed) & (2 ** 63 - 1), int(stream_id), int(call_index), int(H),
         int(W), stream())
    return _da.unpack_params(t.cpu().numpy())


# ------------------------------------------------------------------------------------------
# Spectral normalisation of the D's conv weights (--spectral_norm; csrc/spectral.hip, restated in spectral.py)
# ------------------------------------------------------------------------------------------

class SpectralTable:
    """The device table of dsgan_sn_refresh / dsgan_sn_backward over n layers and the two batched calls.
    ``layers``: one (W, W_sn, u, v, G, dW) per layer -- the weight [Cout, ...] (viewed [R, C] = [Cout, rest]),
    the buffer W_sn is written to, the unit vectors u [R] and v [C], the scratch G the weight-grad kernels
    accumulated into and weight_orig's gradient dW (both None in a table that only refreshes); fp32, dense,
    on one device.  ``sigma`` [n] (allocated when None) receives the layers' sigma; the temporaries
    t [C], a [R] and the backward's partial sums live here.  The table holds addresses: it is valid while
    the tensors are (it keeps them alive) and must be rebuilt when one is replaced."""

    def __init__(self, layers, sigma=None):
        lib = _lib.load()
        self.layers = [tuple(l) for l in layers]
        if not self.layers:
            raise ValueError("SpectralTable: no layer")
        dev = self.layers[0][0].device
        n = len(self.layers)
        self.sigma = sigma if sigma is not None else torch.zeros(n, device=dev, dtype=torch.float32)
        if tuple(self.sigma.shape) != (n,):
            raise ValueError("SpectralTable: sigma must have one element per layer")
        self.can_backward = all(l[4] is not None and l[5] is not None for l in self.layers)
        rows, self.tmp, self.shapes = [], [], []
        for i, (W, Wsn, u, v, G, dW) in enumerate(self.layers):
            R, C = int(W.shape[0]), int(W[0].numel())
            want = {"W": (W, R * C), "W_sn": (Wsn, R * C), "u": (u, R), "v": (v, C), "G": (G, R * C), "dW": (dW, R * C),
                    "sigma": (self.sigma, n)}
            for name, (t, k) in want.items():
                if t is None and name in ("G", "dW"):
                    continue
                if t is None or t.device != dev or not t.is_cuda or t.dtype != torch.float32 or not t.is_contiguous() \
                        or t.numel() != k:
                    raise ValueError("SpectralTable: layer %d: %s must be a dense fp32 tensor of %d elements on %s"
                                     % (i, name, k, dev))
            tmp = (torch.zeros(C, device=dev), torch.zeros(R, device=dev),
                   torch.zeros(lib.dsgan_sn_parts(R, C), device=dev))
            self.tmp.append(tmp)
            self.shapes.append((R, C))
            rows.append([ptr(W), ptr(Wsn), ptr(u), ptr(v), ptr(self.sigma[i:]), ptr(tmp[0]), ptr(tmp[1]), ptr(tmp[2]),
                         ptr(G) or 0, ptr(dW) or 0, R, C])
        if len(rows[0]) != lib.dsgan_sn_fields():
            raise RuntimeError("SpectralTable: the library's table has %d fields" % lib.dsgan_sn_fields())
        self.max_r, self.max_c = max(r for r, _ in self.shapes), max(c for _, c in self.shapes)
        self.nbytes = 4.0 * sum(r * c for r, c in self.shapes)
        self.desc = torch.tensor(rows, dtype=torch.int64).to(dev)

    def refresh(self, iterate=True):
        """u, v, sigma and W_sn of every layer from its W: one power iteration, or (``iterate`` False) sigma
        and W_sn again from the stored (u, v).  The caller bumps the weight generation of the W_sn tensors."""
        with _timed(AUX_TIMER, 0.0, ("sn_refresh", len(self.layers), int(bool(iterate))), "spectral",
                    (4 if iterate else 3) * self.nbytes):
            call("dsgan_sn_refresh", ptr(self.desc), len(self.layers), self.max_r, self.max_c, int(bool(iterate)), stream())

    def backward(self):
        """dW += (G - <G, W_sn> u v^T) / sigma per layer; G is left zeroed."""
        if not self.can_backward:
            raise RuntimeError("SpectralTable.backward: the table was built without G / dW")
        with _timed(AUX_TIMER, 0.0, ("sn_backward", len(self.layers)), "spectral", 6 * self.nbytes):
            call("dsgan_sn_backward", ptr(self.desc), len(self.layers), self.max_r, self.max_c, stream())
