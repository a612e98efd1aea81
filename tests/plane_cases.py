"""Case tables and judges for the plane-wise kernels: InstanceNorm (instnorm.hip) and the depthwise
convs (dwconv.hip).

A plain helper module, the plane-wise counterpart of tests/conv_cases.py, whose guarded tensors it
imports (conv_cases.Slot: NaN before and after every input view, MOAT_BITS around every output,
compared as int32 after the launch).  tests/test_plane_cases_cpu.py checks the tables and the judges
without a GPU, tests/test_plane_families_gpu.py runs the tables through the kernels.

InstanceNorm.  A case is (entry points, N, C, HW) with the launch form the plan query
(dsgan_instnorm_plan) must name for it; a bundle is a set of operands and options on top of it; the
data classes are "normal" (3 N(0,1) + 1), "offset" (1000 + N(0,1)), "sym" (integers of {+-1..+-4}
whose planes sum to exactly 0 while no float4 does) and "spike" (normal with +-2^10 at the first,
the last and 8 seeded elements of every plane, in x and in dy).  The judge is elementwise against
fp64 with the derived bound of in_bounds_fwd / in_bounds_bwd.

Depthwise.  A case is (op, N, C, H, W, K) with the tile configuration dsgan_dwconv_plan must name;
the judges are conv_cases' two: "int" (integer operands, bitwise equal to fp64) and "rnd" (every
element within n * 2^-23 * A of fp64, A the same op on absolute values).

Every Problem also runs on the CPU (device "cpu"): in_standin / dw_standin compute it with torch's
fp32 ops in place of the kernels, optionally with one injected defect (``mut``).
"""
import collections
import ctypes
import math
import zlib

import torch
import torch.nn.functional as F

from conv_cases import EPS, SLOPE32, U16, Slot, _where, gelu_exact, gelu_grad_exact

U = 2.0 ** -24                                               # fp32 unit roundoff
IN_EPS32 = float(torch.tensor(1e-5, dtype=torch.float32))    # eps as the kernels receive it
ACT_CODE = {None: 0, "gelu": 1, "relu": 2, "lrelu": 3, "gelu_fast": 5}
MOAT16 = 0x3C2D                                              # 16-bit output moats (finite in bf16 and fp16)
TINY16 = {"bf16": 0.0, "fp16": 2.0 ** -25}                   # half the spacing of fp16's subnormals
GELU_FAST_ERR = 1.5e-7                                       # common.h: A&S 7.1.26, on erfc
GELU_LIP = 1.13                                              # max gelu' = 1.1289
GELU_CURV = 0.8                                              # max |gelu''| = 2 phi(0) = 0.798


def hdt(prec):
    return torch.float16 if prec == "fp16" else torch.bfloat16


def _seed(*parts):
    return zlib.crc32("|".join(str(p) for p in parts).encode())


class HSlot(Slot):
    """conv_cases.Slot for a 16-bit output: (N, C, 1, HW) elements of ``dtype`` with MOAT16 around."""

    def __init__(self, shape, dtype, device, moat=1 << 14):
        self.kind = "out"
        n = 1
        for k in shape:
            n *= k
        self.buf = torch.full((2 * moat + n,), MOAT16, dtype=torch.int16)
        self.moat_mask = torch.ones(self.buf.numel(), dtype=torch.bool)
        self.moat_mask[moat:moat + n] = False
        self.buf = self.buf.to(device)
        self.view = self.buf[moat:moat + n].view(dtype).view(shape)
        self.before = self.bits().clone()

    def bits(self):
        return self.buf.cpu()


def poison_allocator(device):
    """The caching allocator's free blocks start as NaN, as in conv_cases.launch."""
    if device == "cpu":
        return
    for n in (1 << 14, 1 << 18, (1 << 20) + (1 << 18)):
        t = torch.full((n,), float("nan"), device=device)
        del t


def _bs(t):
    N, C, H, W = t.shape
    return t.stride(0) if N > 1 else C * H * W


def _al16(*ts):
    return int(all(t is None or (t.data_ptr() % 16 == 0 and _bs(t) % 4 == 0) for t in ts))


# ==========================================================================================
# InstanceNorm: the table
# ==========================================================================================
IN_FORMS = ("scalar", "v4", "split")
IN_RUNGS = ("wave", "256x4", "256x16", "1024", "stream")
InPlan = collections.namedtuple("InPlan", "form rung full S")


def in_plan(lib, N, C, HW, aligned16, bwd, ws):
    """dsgan_instnorm_plan decoded (include/dsgan_hip.h)."""
    code = lib.dsgan_instnorm_plan(N, C, HW, int(aligned16), int(bwd), int(ws))
    assert code >= 0, (N, C, HW, code)
    form = IN_FORMS[code & 3]
    return InPlan(form, None if form == "split" else IN_RUNGS[(code >> 2) & 7], bool(code & 32), code >> 8)


# entry: "one" dsgan_instnorm_fwd / _bwd, "ws" the _ws pair, "h16" dsgan_instnorm_fwd_bf16 / _bwd_h.
# form / rung / full / S: what the plan query must report for aligned operands (full: forward only).
INCase = collections.namedtuple("INCase", "entry prec N C HW form rung full S")


def _ic(entry, HW, form, rung, full=False, S=0, N=None, C=3, precs=("fp32",)):
    N = N if N is not None else (3 if HW <= 4100 else 2)
    return [INCase(entry, pr, N, C, HW, form, rung, full, S) for pr in precs]


H16 = ("bf16", "fp16")
IN_CASES = sum([
    # float4 one-workgroup forms, on and beside every ladder edge
    _ic("one", 16, "v4", "wave"), _ic("one", 1020, "v4", "wave"), _ic("one", 1024, "v4", "wave", full=True),
    _ic("one", 1028, "v4", "256x4"), _ic("one", 4092, "v4", "256x4"), _ic("one", 4096, "v4", "256x4", full=True),
    _ic("one", 4100, "v4", "256x16"), _ic("one", 16380, "v4", "256x16"), _ic("one", 16384, "v4", "256x16"),
    _ic("one", 16388, "v4", "1024"), _ic("one", 65532, "v4", "1024"), _ic("one", 65536, "v4", "1024"),
    _ic("one", 65540, "v4", "stream"), _ic("one", 98308, "v4", "stream"),
    # scalar forms (HW % 4 != 0)
    _ic("one", 15, "scalar", "wave"), _ic("one", 961, "scalar", "wave"), _ic("one", 1023, "scalar", "wave"),
    _ic("one", 1025, "scalar", "256x4"), _ic("one", 4095, "scalar", "256x4"),
    _ic("one", 4097, "scalar", "1024"), _ic("one", 16383, "scalar", "1024"),
    _ic("one", 16385, "scalar", "stream"), _ic("one", 66561, "scalar", "stream"),
    # split forms: 6 and 127 planes split, 128 do not
    _ic("ws", 16384, "split", None, S=4), _ic("ws", 16388, "split", None, S=5), _ic("ws", 65540, "split", None, S=17),
    _ic("ws", 16384, "split", None, S=4, N=1, C=127), _ic("ws", 16384, "v4", "256x16", N=2, C=64),
    # 16-bit outputs, one ragged HW per float4 rung
    _ic("h16", 1020, "v4", "wave", precs=H16), _ic("h16", 4092, "v4", "256x4", precs=H16),
    _ic("h16", 16380, "v4", "256x16", precs=H16), _ic("h16", 65532, "v4", "1024", precs=H16),
    _ic("h16", 65540, "v4", "stream", precs=H16),
], [])
# (form, rung, full, bwd) the plan query can return but no case exercises: at most 3, none of a form
# the training step uses (tests/test_plane_cases_cpu.py).  Nothing is left out.
LEFT_OUT = ()


def in_case_id(c):
    return "%s-%s-%dx%dx%d" % (c.entry, c.prec, c.N, c.C, c.HW)


def _ib(name, act=None, data="normal", scale=False, res=False, dres=False, dscale=False, dxsum=False,
        slice=False, misalign=False):
    return dict(name=name, act=act, data=data, scale=scale, res=res, dres=dres, dscale=dscale, dxsum=dxsum,
                slice=slice, misalign=misalign)


def in_bundles(c):
    """A few bundles per case, not the cross product: plain; everything on, as channel slices of
    wider buffers; each activation; each data class; and, for the float4 cases, everything shifted
    by one float (which must then take the scalar kernels)."""
    if c.entry == "h16":     # no scale in either entry point; the forward takes x alone
        return [_ib("plain"),
                _ib("allon", act="gelu_fast", data="spike", res=True, dres=True, dxsum=True, slice=True),
                _ib("lrelu", act="lrelu", res=True, dxsum=True)]
    if c.N * c.C > 9:        # the many-plane split cases: the split threshold alone
        return [_ib("plain")]
    out = [_ib("plain"),
           _ib("allon", act="gelu", data="spike", scale=True, res=True, dres=True, dscale=True, slice=True),
           _ib("fast", act="gelu_fast", res=True, dres=True)]
    if c.entry == "one":
        out += [_ib("lrelu", act="lrelu", scale=True, dscale=True, slice=True),
                _ib("offset", data="offset", scale=True, dscale=True),
                _ib("sym", data="sym", scale=True, dres=True),
                _ib("spike", data="spike")]
        if c.form == "v4":
            out.append(_ib("misalign", act="lrelu", scale=True, res=True, dres=True, dscale=True, slice=True,
                           misalign=True))
        if c.HW == 4092:     # the runtime-act default branch of in_bwd_launch
            out.append(_ib("relu", act="relu", res=True, dres=True))
    return out


def in_problems():
    return [("%s-%s" % (in_case_id(c), b["name"]), c, b) for c in IN_CASES for b in in_bundles(c)]


# ==========================================================================================
# InstanceNorm: data
# ==========================================================================================
def _sym_plane(n, g):
    """n integers of {+-1..+-4} that sum to 0, no aligned group of four (nor the ragged tail) summing
    to 0: float4 groups in (group, negated group) pairs, shuffled as groups, plus a searched tail."""
    def searched(m):
        for _ in range(10000):
            v = torch.randint(1, 5, (m,), generator=g) * (torch.randint(0, 2, (m,), generator=g) * 2 - 1)
            groups = [v[i:i + 4].sum().item() for i in range(0, m, 4)]
            if v.sum().item() == 0 and all(s != 0 for s in groups):
                return v
        raise AssertionError("no sym tail of %d" % m)
    if n < 24:
        return searched(n).double()
    tail = 8 + n % 8
    pairs = (n - tail) // 8
    half = torch.randint(1, 5, (pairs, 4), generator=g)
    half[:, 3] *= torch.randint(0, 2, (pairs,), generator=g) * 2 - 1     # sums of 1..16 or -2..11, never 0 ...
    half[:, 3] = torch.where(half.sum(1) == 0, -half[:, 3], half[:, 3])  # ... after this
    groups = torch.cat([half, -half])[torch.randperm(2 * pairs, generator=g)]
    assert (groups.sum(1) != 0).all()
    return torch.cat([groups.reshape(-1), searched(tail)]).double()


def in_data(c, b):
    """The fp64 operands of an InstanceNorm problem: x, dy (N, C, HW); scale (N, C); res."""
    g = torch.Generator().manual_seed(_seed(in_case_id(c), b["name"]))
    N, C, n = c.N, c.C, c.HW
    kind = b["data"]
    dy = torch.randn((N, C, n), generator=g)
    if kind == "offset":
        x = 1000.0 + torch.randn((N, C, n), generator=g)
    elif kind == "sym":
        x = torch.stack([_sym_plane(n, g) for _ in range(N * C)]).view(N, C, n)
    else:
        x = 3.0 * torch.randn((N, C, n), generator=g) + 1.0
    if kind == "spike":
        for t in (x, dy):
            pos = torch.cat([torch.tensor([0, n - 1]), torch.randint(0, n, (8,), generator=g)])
            sign = (torch.randint(0, 2, (N, C, 10), generator=g) * 2 - 1).to(t.dtype)
            t[:, :, pos] = sign * 1024.0
    x, dy = x.float().double(), dy.float().double()
    d = dict(x=x, dy=dy, scale=None, res=None)
    if b["scale"]:
        if kind == "sym":
            s = 2.0 ** torch.randint(-2, 3, (N, C), generator=g).double()
        else:
            s = (0.25 + 1.5 * torch.rand((N, C), generator=g)).float().double()
        s[0, 1] = -s[0, 1]
        d["scale"] = s
    if b["res"]:
        d["res"] = torch.randn((N, C, n), generator=g).float().double()
    return d


# ==========================================================================================
# InstanceNorm: the op in any dtype (fp64 the reference, fp32 the CPU stand-in), with defects
# ==========================================================================================
def _act(z, act):
    if act in ("gelu", "gelu_fast"):
        return gelu_exact(z)
    if act == "relu":
        return torch.clamp_min(z, 0.0)
    if act == "lrelu":
        return torch.where(z > 0, z, z * torch.tensor(SLOPE32, dtype=torch.float32).to(z.dtype))
    return z


def _act_grad(z, act, mask):
    if act in ("gelu", "gelu_fast"):
        return gelu_grad_exact(z)
    if act in ("relu", "lrelu"):
        slope = torch.tensor(SLOPE32 if act == "lrelu" else 0.0, dtype=torch.float32).to(z.dtype)
        return torch.where(mask if mask is not None else z > 0, torch.ones((), dtype=z.dtype), slope)
    return torch.ones_like(z)


def in_fwd(d, act, dt, mut=None):
    """y = act(IN(scale * x) + res) and its intermediates in dtype ``dt``.  mut: one injected defect
    ("onepass" variance, "drop4" a statistics pass without the last float4, "noscale", "sample0"
    sample 0's planes read for sample 1, "res_first")."""
    x = d["x"].to(dt)
    eps = torch.tensor(IN_EPS32, dtype=dt)
    a = x * d["scale"].to(dt)[..., None] if d["scale"] is not None and mut != "noscale" else x
    res = None if d["res"] is None else d["res"].to(dt)
    if mut == "sample0":
        a = a.clone()
        a[1] = a[0]
    if mut == "res_first":
        a = a + res
        res = None
    st = a[..., :-4] if mut == "drop4" else a
    mu = st.mean(-1, keepdim=True)
    if mut == "onepass":
        var = (st * st).mean(-1, keepdim=True) - mu * mu
    else:
        var = ((st - mu) ** 2).mean(-1, keepdim=True)
    r = 1.0 / torch.sqrt(var + eps)
    xhat = (a - mu) * r
    z = xhat if res is None else xhat + res
    return dict(a=a, mu=mu, var=var, r=r, xhat=xhat, z=z, y=_act(z, act))


def in_bwd(d, act, dt, mean, rstd, mask=None, mut=None, direct_dscale=False):
    """dx, dres (= g), dscale, dxsum of the backward in ``dt`` from the given statistics.  mask: the
    y > 0 of a relu / lrelu forward (None: the sign of this function's own z)."""
    x, dy = d["x"].to(dt), d["dy"].to(dt)
    n = x.shape[-1]
    s = d["scale"].to(dt)[..., None] if d["scale"] is not None else torch.ones((), dtype=dt)
    a = x * s if mut != "noscale" else x
    if mut == "sample0":
        a = a.clone()
        a[1] = a[0]
    mean, rstd = mean.to(dt).view(x.shape[0], x.shape[1], 1), rstd.to(dt).view(x.shape[0], x.shape[1], 1)
    xhat = (a - mean) * rstd
    z = xhat if d["res"] is None else xhat + d["res"].to(dt)
    g = dy * _act_grad(z, act, mask) if act else dy
    st = slice(None, -4) if mut == "drop4" else slice(None)
    mg = g[..., st].sum(-1, keepdim=True) / n
    mgh = (g * xhat)[..., st].sum(-1, keepdim=True) / n
    t = g - mg - xhat * mgh
    dx = s * rstd * t
    if direct_dscale:      # the definition: sum over the plane of d(loss)/d(scale * x) * x
        dscale = (rstd * t * x).sum(-1)
    else:                  # instnorm.hip's closed form
        dscale = (mgh * n * torch.tensor(IN_EPS32, dtype=dt) * rstd * rstd / s).view(x.shape[0], x.shape[1])
    return dict(xhat=xhat, z=z, g=g, mg=mg, mgh=mgh, t=t, dx=dx, dscale=dscale, s=s)


# ==========================================================================================
# InstanceNorm: the bound
#
# u = 2^-24, n = HW, D(n) = 96 + ceil(n / 1024): no form adds more terms than this in one chain (at
# most 64 per thread, 6 shuffle steps, 16 wave partials, plus chunk partials or stream iterations).
# ==========================================================================================
def in_D(n):
    return 96 + math.ceil(n / 1024)


def in_bounds_fwd(R, n, act, prec=None):
    """R: in_fwd in fp64.  Returns dmu (|mean - mu|), rho (|rstd / r - 1|), Bx (xhat), Bz, By."""
    D = in_D(n)
    a, mu, var, r, xhat, z, y = (R[k] for k in ("a", "mu", "var", "r", "xhat", "z", "y"))
    d = a - mu
    m = lambda t: t.mean(-1, keepdim=True)
    dmu = (D + 3) * U * m(a.abs())
    dd = dmu + U * (a.abs() + d.abs())
    rho = 0.5 * ((D + 6) * U + (2 * U * m(d.abs() * (a.abs() + d.abs())) + dmu ** 2) / (var + IN_EPS32)) + 3 * U
    Bx = r * dd + xhat.abs() * (rho + 2 * U)
    Bz = Bx + U * z.abs()
    if act in ("gelu", "gelu_fast"):
        # gelu is 1.13-Lipschitz; gelu_f in fp32 is within 2^-21 |z| of gelu (conv_cases.bound_rnd);
        # the A&S form adds its 1.5e-7 on erfc, that is on Phi: 1.5e-7 |z| on z Phi(z)
        By = GELU_LIP * Bz + 2.0 ** -21 * z.abs() + (GELU_FAST_ERR * z.abs() if act == "gelu_fast" else 0.0)
    elif act == "lrelu":
        By = Bz + U * y.abs()          # 1-Lipschitz, and one product
    else:
        By = Bz                        # none, relu
    if prec in U16:
        By = By + U16[prec] * y.abs() + TINY16[prec]
    return dict(dmu=dmu, rho=rho, Bx=Bx, Bz=Bz, By=By)


def in_bounds_bwd(R, Bf, B, d, n, act, prec=None):
    """R: in_fwd in fp64, Bf: in_bounds_fwd, B: in_bwd in fp64 (exact statistics)."""
    D = in_D(n)
    m = lambda t: t.mean(-1, keepdim=True)
    dy, g, xhat, t, dx, s = d["dy"], B["g"], B["xhat"], B["t"], B["dx"], B["s"]
    r, rho, Bx, Bz = R["r"], Bf["rho"], Bf["Bx"], Bf["Bz"]
    if act in ("gelu", "gelu_fast"):
        # |gelu''| <= 0.8; gelu_g in fp32 within 2^-21 (conv_cases.bound_rnd), the A&S form 1.5e-7 more
        allow = 2.0 ** -21 + (GELU_FAST_ERR if act == "gelu_fast" else 0.0)
        Bg = dy.abs() * (GELU_CURV * Bz + allow) + U * g.abs()
    elif act == "lrelu":
        Bg = U * g.abs()               # the mask is the launch's own; one product
    else:
        Bg = torch.zeros_like(g)       # none; relu multiplies by 1 or 0
    dmg = (D + 3) * U * m(g.abs()) + m(Bg)
    dmgh = (D + 4) * U * m((g * xhat).abs()) + m(g.abs() * Bx + xhat.abs() * Bg)
    mg, mgh = B["mg"], B["mgh"]
    Bt = Bg + dmg + xhat.abs() * dmgh + mgh.abs() * Bx + U * (g.abs() + mg.abs() + 2 * (xhat * mgh).abs() + 2 * t.abs())
    Bdx = s.abs() * r * Bt + dx.abs() * (rho + 4 * U)
    sq = lambda v: v.view(dy.shape[0], dy.shape[1])
    Bds = sq(n * IN_EPS32 * r * r / s.abs() * dmgh) + B["dscale"].abs() * sq(2 * rho + 6 * U)
    Bsum = Bdx.sum(-1) + D * U * dx.abs().sum(-1)
    Bdxh = Bdx + U16[prec] * dx.abs() + TINY16[prec] if prec in U16 else None
    return dict(Bg=Bg, Bdx=Bdx, Bdscale=Bds, Bdxsum=Bsum, Bdxh=Bdxh)


def mask_ok(y, z64):
    """test_batchnorm_ops_gpu.py's cap on a relu / lrelu launch's own mask against fp64's: at most
    1e-5 of the elements differ, and only where fp64 |z| < 1e-5."""
    mism = (y > 0) != (z64 > 0)
    return mism.double().mean().item() <= 1e-5 and bool((z64[mism].abs() < 1e-5).all())


# ==========================================================================================
# InstanceNorm: the problem, the launches, the stand-in, the judge
# ==========================================================================================
class INProblem:
    """A case x bundle with its operands: ``cpu`` the fp64 operands, ``slots`` the guarded tensors."""

    def __init__(self, case, b, device="cpu", lib=None):
        self.case, self.b, self.device = case, b, device
        c = case
        N, C, n = c.N, c.C, c.HW
        self.cpu = d = in_data(c, b)
        lead = 1 if b["misalign"] else 0
        wide = (4, 8) if b["slice"] else None
        moat = max(1 << 14, (n + 64 + 63) // 64 * 64)    # a whole neighbouring plane lies in the moat
        nan = torch.full((N, C, 1, n), float("nan"))

        def plane(t, kind):
            return Slot(t.view(N, C, 1, n), kind, device, wide=wide, lead=lead, moat=moat)

        def vec(t, kind):
            return Slot(t.reshape(N * C), kind, device, lead=lead)

        nanv = torch.full((N * C,), float("nan"))
        s_ = dict(x=plane(d["x"], "in"), dy=plane(d["dy"], "in"), mean=vec(nanv, "out"), rstd=vec(nanv, "out"))
        if d["scale"] is not None:
            s_["scale"] = vec(d["scale"], "in")
        if d["res"] is not None:
            s_["res"] = plane(d["res"], "in")
        h16 = c.entry == "h16"
        if h16:
            s_["yh"] = HSlot((N, C, 1, n), hdt(c.prec), device, moat=moat)
            s_["dxh"] = HSlot((N, C, 1, n), hdt(c.prec), device, moat=moat)
        if not h16 or b["act"] or b["res"]:
            s_["y"] = plane(nan, "out")
        if not h16:
            s_["dx"] = plane(nan, "out")
        if b["dres"]:
            s_["dres"] = plane(nan, "out")
        if b["dscale"]:
            s_["dscale"] = vec(nanv, "out")
        if b["dxsum"]:
            s_["dxsum"] = vec(nanv, "out")
        self.slots = s_
        if c.entry == "ws" and lib is not None:
            need = lib.dsgan_instnorm_workspace(N, C, n)
            if need:
                self.slots["ws"] = Slot(torch.full((need,), float("nan")), "out", device)
        self.mask = None       # the relu / lrelu launch's own y > 0

    def v(self, name):
        sl = self.slots.get(name)
        return None if sl is None else sl.view

    def aligned(self, bwd):
        names = ("dy", "x", "dx", "res", "dres") if bwd else ("x", "y", "res")
        return _al16(*[self.v(k) for k in names])

    def tag(self):
        return "%s %s" % (in_case_id(self.case), self.b["name"])


def in_expect_plan(lib, P):
    """The launch form P must take, asked of the plan query as the entry points ask it: the case's
    own, or under shifted views the scalar form.  Returns {0: forward plan, 1: backward plan}."""
    c = P.case
    out = {}
    for bwd in (0, 1):
        al = P.aligned(bwd)
        p = in_plan(lib, c.N, c.C, c.HW, al, bwd, c.entry == "ws")
        if P.b["misalign"]:
            assert not al and p.form == "scalar", "%s: the shifted views still take %r" % (P.tag(), (p,))
        else:
            assert al or c.HW % 4, "%s: the views are not 16-byte aligned" % P.tag()
            want = InPlan(c.form, c.rung, c.full and not bwd, c.S)
            assert p == want, "%s (bwd=%d) takes %r, the table says %r" % (P.tag(), bwd, p, want)
        out[bwd] = p
    return out


def _ws_args(P, ptr):
    w = P.v("ws")
    return (ptr(w), 0 if w is None else w.numel())


def in_launch_fwd(L, P):
    """The forward launches of P through the C ABI (L = dsgan_hip._lib)."""
    c, b = P.case, P.b
    ptr, st = L.ptr, L.stream()
    x, y, res = P.v("x"), P.v("y"), P.v("res")
    act = ACT_CODE[b["act"]]
    if c.entry == "h16":
        L.call("dsgan_instnorm_fwd_bf16", ptr(x), _bs(x), ptr(P.v("yh")), c.C * c.HW, ptr(P.v("mean")),
               ptr(P.v("rstd")), c.N, c.C, c.HW, IN_EPS32, st)
        if y is None:
            return
        # (the fp32 forward with the bundle's residual and activation: the statistics are the same
        # bits, tests/test_ops_gpu.py::test_instnorm_bf16_output; it gives the backward its mask)
    args = (ptr(x), _bs(x), ptr(P.v("scale")), ptr(res), 0 if res is None else _bs(res), ptr(y), _bs(y),
            ptr(P.v("mean")), ptr(P.v("rstd")), c.N, c.C, c.HW, act, SLOPE32, IN_EPS32)
    if c.entry == "ws":
        L.call("dsgan_instnorm_fwd_ws", *args, *_ws_args(P, ptr), st)
    else:
        L.call("dsgan_instnorm_fwd", *args, st)


def in_launch_bwd(L, P):
    c, b = P.case, P.b
    ptr, st = L.ptr, L.stream()
    x, dy, res, dres = P.v("x"), P.v("dy"), P.v("res"), P.v("dres")
    act = ACT_CODE[b["act"]]
    rb, db = (0 if res is None else _bs(res)), (0 if dres is None else _bs(dres))
    if c.entry == "h16":
        L.call("dsgan_instnorm_bwd_h", ptr(dy), _bs(dy), ptr(x), _bs(x), ptr(res), rb, ptr(P.v("mean")),
               ptr(P.v("rstd")), ptr(P.v("dxh")), c.C * c.HW, ptr(P.v("dxsum")), ptr(dres), db, c.N, c.C, c.HW, act,
               SLOPE32, IN_EPS32, st)
        return
    dx = P.v("dx")
    args = (ptr(dy), _bs(dy), ptr(x), _bs(x), ptr(P.v("scale")), ptr(res), rb, ptr(P.v("mean")), ptr(P.v("rstd")),
            ptr(dx), _bs(dx), ptr(dres), db, ptr(P.v("dscale")), c.N, c.C, c.HW, act, SLOPE32, IN_EPS32)
    if c.entry == "ws":
        if "ws" in P.slots:
            P.v("ws").fill_(float("nan"))
        L.call("dsgan_instnorm_bwd_ws", *args, *_ws_args(P, ptr), st)
    else:
        L.call("dsgan_instnorm_bwd", *args, st)


def in_standin(P, mut_fwd=None, mut_bwd=None):
    """torch's CPU fp32 two-pass InstanceNorm in place of the kernels (device "cpu")."""
    c, b, d = P.case, P.b, P.cpu
    N, C, n = c.N, c.C, c.HW
    sh = (N, C, 1, n)
    Rf = in_fwd(d, b["act"], torch.float32, mut=mut_fwd)
    P.v("mean").copy_(Rf["mu"].reshape(-1))
    P.v("rstd").copy_(Rf["r"].reshape(-1))
    if c.entry == "h16":
        plain = in_fwd(dict(d, res=None, scale=None), None, torch.float32, mut=mut_fwd)
        P.v("yh").copy_(plain["y"].view(sh).to(hdt(c.prec)))
    if "y" in P.slots:
        P.v("y").copy_(Rf["y"].view(sh))
    mask = (Rf["y"] > 0) if b["act"] in ("relu", "lrelu") else None
    Rb = in_bwd(d, b["act"], torch.float32, Rf["mu"], Rf["r"], mask=mask, mut=mut_bwd)
    if c.entry == "h16":
        P.v("dxh").copy_(Rb["dx"].view(sh).to(hdt(c.prec)))
    else:
        P.v("dx").copy_(Rb["dx"].view(sh))
    if b["dres"]:
        P.v("dres").copy_(Rb["g"].view(sh))
    if b["dscale"]:
        P.v("dscale").copy_(Rb["dscale"].reshape(-1))
    if b["dxsum"]:
        P.v("dxsum").copy_(Rb["dx"].sum(-1).reshape(-1))


def in_check_guards(P):
    for name, sl in P.slots.items():
        sl.check("%s: tensor '%s'" % (P.tag(), name))


def _ratio(P, what, got, ref, bound):
    """Every element of ``got`` finite and within ``bound`` of ``ref``; returns the largest ratio."""
    tag = "%s [%s]" % (P.tag(), what)
    got = got.double().reshape(ref.shape)
    assert torch.isfinite(got).all(), "%s: non-finite output at %s" % (
        tag, _where((~torch.isfinite(got)).nonzero()[0].tolist(), got.shape))
    err = (got - ref).abs()
    ratio = torch.where(err == 0, torch.zeros_like(err), err / bound.expand_as(err).clamp_min(1e-300))
    worst = int(ratio.argmax())
    r = float(ratio.reshape(-1)[worst])
    if not r <= 1.0:
        i = [int(k) for k in torch.unravel_index(torch.tensor(worst), got.shape)]
        t = tuple(i)
        raise AssertionError("%s: %d of %d elements outside the bound; worst at %s: got %.9g, ref %.9g, %.3g x the "
                             "bound %.3g" % (tag, int((ratio > 1).sum()), ratio.numel(), _where(i, got.shape),
                                             got[t].item(), ref[t].item(), r, bound.expand_as(err)[t].item()))
    return r


def in_check(P, fwd_only=False):
    """Guards, then every output of P against fp64 within the derived bound.  Returns the largest
    ratio to the bound per output: {"y": ..., "mean": ..., "dx": ...}."""
    in_check_guards(P)
    c, b, d = P.case, P.b, P.cpu
    N, C, n = c.N, c.C, c.HW
    act, prec = b["act"], c.prec
    cpu = lambda name: P.v(name).detach().cpu()
    out = {}
    R = in_fwd(d, act, torch.float64)
    Bf = in_bounds_fwd(R, n, act)
    mean, rstd = cpu("mean").view(N, C, 1), cpu("rstd").view(N, C, 1)
    out["mean"] = _ratio(P, "mean", mean, R["mu"], Bf["dmu"])
    out["rstd"] = _ratio(P, "rstd", rstd.double() / R["r"], torch.ones_like(R["r"]), Bf["rho"])
    if b["data"] == "sym":
        assert bool((mean == 0).all()), "%s: a plane that sums to exactly 0 has mean %r" % (P.tag(), mean.reshape(-1).tolist())
    if "y" in P.slots:
        y = cpu("y").view(N, C, n)
        out["y"] = _ratio(P, "y", y, R["y"], Bf["By"])
        if act in ("relu", "lrelu"):
            assert mask_ok(y, R["z"]), "%s: the launch's y > 0 is outside the mask cap against fp64" % P.tag()
            P.mask = y > 0
    if c.entry == "h16":
        R0 = in_fwd(dict(d, res=None, scale=None), None, torch.float64)
        B0 = in_bounds_fwd(R0, n, None, prec)
        out["yh"] = _ratio(P, "yh", cpu("yh").view(N, C, n), R0["y"], B0["By"])
    if fwd_only:
        return out
    if b["data"] == "offset":
        assert act is None, "the offset class runs its backward without an activation"
    # (dscale: the closed form in fp64.  The sum by the definition cancels to O(eps) and loses that
    # much even in fp64; tests/test_plane_cases_cpu.py checks the two against each other)
    B = in_bwd(d, act, torch.float64, R["mu"], R["r"], mask=P.mask)
    Bb = in_bounds_bwd(R, Bf, B, d, n, act, prec)
    if c.entry == "h16":
        out["dxh"] = _ratio(P, "dxh", cpu("dxh").view(N, C, n), B["dx"], Bb["Bdxh"])
    else:
        out["dx"] = _ratio(P, "dx", cpu("dx").view(N, C, n), B["dx"], Bb["Bdx"])
    if b["dres"]:
        dres = cpu("dres").view(N, C, n)
        if act is None:
            same = dres.view(torch.int32) == d["dy"].float().view(torch.int32)
            assert bool(same.all()), "%s: dres differs from dy in %d elements without an activation" % (
                P.tag(), int((~same).sum()))
        else:
            out["dres"] = _ratio(P, "dres", dres, B["g"], Bb["Bg"])
    if b["dscale"]:
        out["dscale"] = _ratio(P, "dscale", cpu("dscale").view(N, C), B["dscale"], Bb["Bdscale"])
    if b["dxsum"]:
        out["dxsum"] = _ratio(P, "dxsum", cpu("dxsum").view(N, C), torch.zeros(N, C, dtype=torch.float64), Bb["Bdxsum"])
    return out


# ==========================================================================================
# Depthwise: the table
# ==========================================================================================
# op: "fwd" HF.dwconv_raw, "wgrad" HF._dw_wgrad, "mfwd" / "mwgrad" the four-quarter entry points (C =
# channels per quarter, K unused).  cfg: the tile configuration the plan query must name for aligned
# operands; pf: the weight-grad must report the prefetch form (and nper >= 8).  big: the integer
# judge only (long reference).
DWCase = collections.namedtuple("DWCase", "op N C H W K cfg pf big")
KS = (3, 5, 7, 9)
# heights 8 and 40 / 70: the last tile row is ragged for every K's tile height (configuration 1: 64, 32
# or 16 rows; 2: 64 or 32; 3: 32)
DW_SHAPES = [((1, 2, 4, 4), 0), ((2, 3, 40, 37), 0), ((2, 3, 33, 36), 0), ((2, 2, 70, 65), 0),
             ((2, 3, 8, 32), 3), ((2, 3, 40, 32), 3), ((2, 3, 8, 64), 2), ((2, 3, 70, 64), 2),
             ((2, 3, 8, 128), 1), ((2, 2, 70, 128), 1), ((2, 2, 8, 256), 1), ((1, 2, 70, 256), 1)]
DW_CASES = (
    [DWCase(op, *s, K, cfg, False, False) for op in ("fwd", "wgrad") for s, cfg in DW_SHAPES for K in KS]
    # the generic kernels with one workgroup per plane
    + [DWCase(op, 2, 1024, 33, 36, 7, 0, False, True) for op in ("fwd", "wgrad")]
    # the weight-grad's prefetch form (K = 7, >= 8 images per workgroup); (17, ...): the last workgroup
    # walks fewer images; (5, ...): the plain form with an uneven split
    + [DWCase("wgrad", 16, 512, 8, 32, 7, 3, True, False), DWCase("wgrad", 16, 512, 8, 64, 7, 2, True, True),
       DWCase("wgrad", 16, 512, 8, 128, 7, 1, True, True), DWCase("wgrad", 16, 256, 40, 32, 7, 3, True, True),
       DWCase("wgrad", 17, 512, 8, 32, 7, 3, True, True), DWCase("wgrad", 5, 512, 8, 32, 7, 3, False, True)]
    + [DWCase(op, 2, 2, H, W, 0, cfg, False, False) for op in ("mfwd", "mwgrad")
       for W, cfg in ((128, 1), (64, 2), (32, 3)) for H in (8, 40)]
    + [DWCase("mwgrad", 16, 128, 8, 32, 0, 3, True, True), DWCase("mwgrad", 17, 128, 8, 32, 0, 3, True, True),
       DWCase("mwgrad", 16, 128, 8, 64, 0, 2, True, True), DWCase("mwgrad", 16, 128, 8, 128, 0, 1, True, True)]
)


def dw_case_id(c):
    return "%s-%dx%dx%dx%d-k%d" % (c.op, c.N, c.C, c.H, c.W, c.K)


def _db(name, flip=False, bias=False, acc=False, slice=False, misalign=False):
    return dict(name=name, flip=flip, bias=bias, acc=acc, slice=slice, misalign=misalign)


def dw_bundles(c):
    if c.big:
        return [_db("plain", bias=c.op == "fwd")]
    if c.op in ("fwd", "mfwd"):
        out = [_db("bias", bias=True), _db("flip+acc+slice", flip=True, acc=True, slice=True),
               _db("flip", flip=True), _db("bias+acc", bias=True, acc=True)]
    else:
        out = [_db("plain"), _db("slice", slice=True)]
    if c.cfg and c.op in ("fwd", "wgrad"):
        out.append(_db("misalign", bias=c.op == "fwd", slice=True, misalign=True))
    return out


def dw_judges(c, b):
    if c.big:
        return ["int", "rnd"] if (c.N, c.C, c.W) == (16, 512, 32) else ["int"]
    return ["int", "rnd"] if b["name"] in ("bias", "plain", "flip+acc+slice", "slice") else ["int"]


def dw_problems():
    return [("%s-%s-%s" % (dw_case_id(c), b["name"], j), c, b, j)
            for c in DW_CASES for b in dw_bundles(c) for j in dw_judges(c, b)]


DwPlan = collections.namedtuple("DwPlan", "cfg nsplit nper prefetch")


def dw_plan(lib, N, C, H, W, K, aligned16, op, multi):
    a, b, p = ctypes.c_int(-1), ctypes.c_int(-1), ctypes.c_int(-1)
    cfg = lib.dsgan_dwconv_plan(N, C, H, W, K, int(aligned16), int(op), int(multi), ctypes.addressof(a),
                                ctypes.addressof(b), ctypes.addressof(p))
    return DwPlan(cfg, a.value, b.value, p.value)


# ==========================================================================================
# Depthwise: the op by its definition, one tap at a time, in any dtype
# ==========================================================================================
def dw_conv(x, w, bias, K, flip, pad_mode="constant"):
    """y[n,c] = sum_taps w[c,kh,kw] x[n,c,h+kh-p,w+kw-p] (+ bias); flip: the kernel reversed."""
    N, C, H, W = x.shape
    p = K // 2
    w = w.reshape(C, K * K)
    if flip:
        w = w.flip(1)
    xp = F.pad(x, (p, p, p, p), mode=pad_mode)
    y = torch.zeros_like(x) if bias is None else bias.view(1, C, 1, 1).expand_as(x).clone()
    for kh in range(K):
        for kw in range(K):
            y += w[:, kh * K + kw].view(1, C, 1, 1) * xp[:, :, kh:kh + H, kw:kw + W]
    return y


def dw_wgrad(dy, x, K):
    N, C, H, W = x.shape
    p = K // 2
    xp = F.pad(x, (p, p, p, p))
    dw = torch.empty((C, K * K), dtype=x.dtype)
    for kh in range(K):
        for kw in range(K):
            dw[:, kh * K + kw] = (dy * xp[:, :, kh:kh + H, kw:kw + W]).sum((0, 2, 3))
    return dw.view(C, 1, K, K), dy.sum((0, 2, 3))


class DWProblem:
    """A depthwise case x bundle x judge with its operands; quarters: [(channel offset, q, K)]."""

    def __init__(self, case, b, judge, device="cpu"):
        self.case, self.b, self.judge, self.device = case, b, judge, device
        c = case
        multi = c.op in ("mfwd", "mwgrad")
        self.multi = multi
        Ct = 4 * c.C if multi else c.C
        self.quarters = [(i * c.C, c.C, 3 + 2 * i) for i in range(4)] if multi else [(0, c.C, c.K)]
        g = torch.Generator().manual_seed(_seed(dw_case_id(c), b["name"], judge))
        wg = c.op in ("wgrad", "mwgrad")
        shape = (c.N, Ct, c.H, c.W)

        def data(sh, lim, std=1.0):
            if judge == "int":
                return torch.randint(-lim, lim + 1, sh, generator=g).double()
            return (torch.randn(sh, generator=g) * std).float().double()

        d = {}
        d["x"] = data(shape, 2 if wg else 4)
        if wg:
            d["dy"] = data(shape, 2)
            d["dw0"] = [data((q, 1, K, K), 8) for _, q, K in self.quarters]
            d["db0"] = [data((q,), 8) for _, q, K in self.quarters]
        else:
            d["w"] = [data((q, 1, K, K), 4, 0.5) for _, q, K in self.quarters]
            d["bias"] = [data((q,), 8) for _, q, K in self.quarters] if b["bias"] else None
            d["y0"] = data(shape, 8) if b["acc"] else None
        self.cpu = d
        lead = 1 if b["misalign"] else 0
        wide = (4, (4 + Ct + 1 + 3) // 4 * 4) if (b["slice"] or b["misalign"]) else None
        moat = max(1 << 14, (c.H * c.W * 2 + 63) // 64 * 64)
        plane = lambda t, kind, wd=wide: Slot(t, kind, device, wide=wd, lead=lead, moat=moat)
        s_ = dict(x=plane(d["x"], "in"))
        if wg:
            s_["dy"] = plane(d["dy"], "in")
            for i, (_, q, K) in enumerate(self.quarters):
                s_["dw%d" % i] = Slot(d["dw0"][i], "out", device)
                s_["db%d" % i] = Slot(d["db0"][i], "out", device)
        else:
            for i, (_, q, K) in enumerate(self.quarters):
                s_["w%d" % i] = Slot(d["w"][i], "in", device)
                if b["bias"]:
                    s_["b%d" % i] = Slot(d["bias"][i], "in", device)
            y0 = d["y0"] if b["acc"] else torch.full(shape, float("nan"))
            # (the four-quarter forward writes a dense y: MultiDwConvFn hands it a fresh buffer)
            s_["y"] = plane(y0, "out", None if multi else wide)
        self.slots = s_

    def v(self, name):
        sl = self.slots.get(name)
        return None if sl is None else sl.view

    def tag(self):
        return "%s %s [%s]" % (dw_case_id(self.case), self.b["name"], self.judge)

    def aligned(self):
        return _al16(self.v("x"), self.v("dy") if "dy" in self.slots else self.v("y"))

    def n_terms(self, K):
        c, b = self.case, self.b
        if c.op in ("wgrad", "mwgrad"):
            return c.N * c.H * c.W + 1
        return K * K + int(b["bias"]) + int(b["acc"])


def dw_expect_plan(lib, P):
    c = P.case
    wg = c.op in ("wgrad", "mwgrad")
    al = P.aligned()
    p = dw_plan(lib, c.N, c.C, c.H, c.W, c.K or 9, al, wg, P.multi)
    if P.b["misalign"]:
        assert not al and p.cfg == 0, "%s: the shifted views still take configuration %d" % (P.tag(), p.cfg)
    else:
        assert al and p.cfg == c.cfg, "%s takes configuration %d (aligned %d), the table says %d" % (
            P.tag(), p.cfg, al, c.cfg)
        if wg and c.cfg:
            assert bool(p.prefetch) == c.pf and (not c.pf or p.nper >= 8), (P.tag(), p)
            assert (p.nsplit - 1) * p.nper < c.N <= p.nsplit * p.nper, (P.tag(), p)
        if wg and not c.cfg and c.N * c.C >= 2048:
            assert p.nsplit == 1, "%s: %d workgroups per plane, not one" % (P.tag(), p.nsplit)
    return p


def dw_compute(P, dt, mode="ref", mut=None):
    """{slot name: value} of P's outputs in ``dt``; mode "abs": the same op on absolute values.  mut:
    "noflip", "clamp" (halo replicated instead of zero), "bias_twice" (under accumulate)."""
    c, b, d = P.case, P.b, P.cpu
    ab = (lambda t: t.abs()) if mode == "abs" else (lambda t: t)
    x = ab(d["x"].to(dt))
    out = {}
    if c.op in ("wgrad", "mwgrad"):
        dy = ab(d["dy"].to(dt))
        for i, (o, q, K) in enumerate(P.quarters):
            dw, db = dw_wgrad(dy[:, o:o + q], x[:, o:o + q], K)
            out["dw%d" % i] = ab(d["dw0"][i].to(dt)) + dw
            out["db%d" % i] = ab(d["db0"][i].to(dt)) + db
        return out
    ys = []
    for i, (o, q, K) in enumerate(P.quarters):
        bias = ab(d["bias"][i].to(dt)) if b["bias"] else None
        y = dw_conv(x[:, o:o + q], ab(d["w"][i].to(dt)), bias, K, b["flip"] and mut != "noflip",
                    "replicate" if mut == "clamp" else "constant")
        if mut == "bias_twice":
            y = y + bias.view(1, -1, 1, 1)
        ys.append(y)
    y = torch.cat(ys, 1)
    if b["acc"]:
        y = y + ab(d["y0"].to(dt))
    out["y"] = y
    return out


def dw_standin(P, mut=None):
    for k, v in dw_compute(P, torch.float32, mut=mut).items():
        P.v(k).copy_(v)


def dw_launch(HF, P):
    """The launch of P on the GPU, scratch and allocator blocks poisoned with NaN first."""
    c, b = P.case, P.b
    L = HF._lib
    ptr = L.ptr
    poison_allocator(P.device)
    real_ws = HF._ws

    def nan_ws(query, *dims, like):
        t = real_ws(query, *dims, like=like)
        if t is not None:
            t.fill_(float("nan"))
        return t
    HF._ws = nan_ws
    try:
        x = P.v("x")
        if c.op == "fwd":
            HF.dwconv_raw(x, P.v("w0"), P.v("b0"), flip=b["flip"], out=P.v("y"), accumulate=b["acc"])
        elif c.op == "wgrad":
            HF._dw_wgrad(P.v("dy"), x, P.v("dw0"), P.v("db0"), c.K)
        elif c.op == "mfwd":
            y = P.v("y")
            wb = []
            for i in range(4):
                wb += [ptr(P.v("w%d" % i)), ptr(P.v("b%d" % i))]
            L.call("dsgan_dwconv_multi_fwd", ptr(x), _bs(x), *wb, ptr(y), _bs(y), c.N, c.C, c.H, c.W, int(b["flip"]),
                   int(b["acc"]), L.stream())
        else:
            dy = P.v("dy")
            gs = []
            for i in range(4):
                gs += [ptr(P.v("dw%d" % i)), ptr(P.v("db%d" % i))]
            ws = nan_ws("dsgan_dwconv_multi_wgrad_workspace", c.N, c.C, c.H, c.W, like=x)
            L.call("dsgan_dwconv_multi_wgrad", ptr(dy), _bs(dy), ptr(x), _bs(x), *gs, c.N, c.C, c.H, c.W, ptr(ws),
                   ws.numel(), L.stream())
    finally:
        HF._ws = real_ws
    torch.cuda.synchronize()


def dw_check(P):
    """Guards, then P's judge on every output; returns the largest judge-"rnd" ratio (0 for "int")."""
    for name, sl in P.slots.items():
        sl.check("%s: tensor '%s'" % (P.tag(), name))
    ref = dw_compute(P, torch.float64)
    A = dw_compute(P, torch.float64, mode="abs") if P.judge == "rnd" else None
    worst = 0.0
    for name, want in ref.items():
        got = P.v(name).detach().cpu().contiguous()
        tag = "%s '%s'" % (P.tag(), name)
        assert torch.isfinite(got).all(), "%s: non-finite output at %s" % (
            tag, _where((~torch.isfinite(got)).nonzero()[0].tolist(), got.shape))
        if name == "y":     # per quarter: each has its own K
            n = torch.cat([torch.full((q,), float(P.n_terms(K))) for _, q, K in P.quarters]).double().view(1, -1, 1, 1)
            nmax = int(n.max())
        else:
            n = nmax = P.n_terms(P.quarters[int(name[-1])][2])
        if P.judge == "int":
            lim = 16 * nmax + 16 if name == "y" else 4 * nmax + 16
            assert lim < 2 ** 24, "integer data no longer exact at n = %d" % nmax
            bad = got != want.to(torch.float32)
            if bad.any():
                i = bad.nonzero()[0].tolist()
                t = tuple(i)
                raise AssertionError("%s: %d of %d elements differ on integer data; first at %s: got %r, exact %r" % (
                    tag, int(bad.sum()), bad.numel(), _where(i, got.shape), got[t].item(), want[t].item()))
        else:
            bound = n * EPS * A[name]
            err = (got.double() - want).abs()
            ratio = torch.where(err == 0, torch.zeros_like(err), err / bound.clamp_min(1e-300))
            k = int(ratio.argmax())
            r = float(ratio.reshape(-1)[k])
            if not r <= 1.0:
                i = [int(j) for j in torch.unravel_index(torch.tensor(k), got.shape)]
                t = tuple(i)
                raise AssertionError("%s: %d of %d elements outside n*2^-23*A (n = %d); worst at %s: got %.9g, ref "
                                     "%.9g, %.3g x the bound" % (tag, int((ratio > 1).sum()), ratio.numel(), nmax,
                                                                 _where(i, got.shape), got[t].item(), want[t].item(), r))
            worst = max(worst, r)
    return worst
