"""Record what the Python layer asks of libdsgan_hip.so, to compare two trees of it.

  python tools/call_trace.py --config a|b|extra --out DIR      (GPU) writes
      DIR/trace_<config>.txt  the ordered C-ABI calls of the recorded steps: the entry point plus
                              every argument typed by _lib.SIGNATURES -- integers and floats by
                              value, device pointers and the stream as null / p<address % 16>, host
                              arrays (ctypes casts: tap tables, pointer lists) as "host"
      DIR/rows_<config>.json  the plain inputs of every conv_{fwd,dgrad,wgrad}_raw call, with the
                              kernel family that call recorded on IGEMM_TIMER and its launch form
    a: eager training steps at the benchmark's config (256^2, B=16, bf16, as tools/launch_table.py
       builds it); b: eager fp32 steps at 64^2, B=2; extra: hand-made raw calls at the smallest
       shapes that reach the families a training step does not (EXTRA below).
  python tools/call_trace.py --compare OLD.txt NEW.txt         call counts per entry point, then
      "identical" or the differing calls (a scratch pointer that is null with size 0 on both sides
      of an otherwise equal call is listed as a permitted normalisation, not a difference)
  python tools/call_trace.py --merge ROWS.json ... --table OUT.json   deduplicated dispatch table
      (tests/golden/conv_dispatch_v1.json, read by tests/test_dispatch_cpu.py)

It patches dsgan_hip._lib.call (and the binding of it in every dsgan_hip module already imported:
the package's __init__ imports functional, so there is no moment before that) and wraps the three
raw conv launchers; it relies on nothing else of functional.py, so the same file runs on trees
before and after a change of that module."""
import argparse
import collections
import ctypes
import json
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [REPO, os.path.join(REPO, "ds-gan_amd")]

CALLS = []   # (entry point, typed argument strings)


def _typed(sig, args):
    out = []
    for t, a in zip(sig, args):
        if t is ctypes.c_void_p:
            if isinstance(a, ctypes.c_void_p):
                out.append("host" if a.value else "null")
            else:
                out.append("null" if not a else "p%d" % (int(a) % 16))
        elif t in (ctypes.c_float, ctypes.c_double):
            out.append(repr(float(a)))
        else:
            out.append(str(int(a)))
    if len(args) != len(sig):
        out.append("ARGC=%d" % len(args))
    return out


def install():
    """Route every _lib.call through the recorder; returns dsgan_hip.functional."""
    import dsgan_hip
    from dsgan_hip import _lib
    from dsgan_hip import functional as HF
    orig = _lib.call

    def rec(name, *args):
        CALLS.append((name, _typed(_lib.SIGNATURES[name], args)))
        return orig(name, *args)

    _lib.call = rec
    for name, mod in list(sys.modules.items()):
        if name.startswith("dsgan_hip") and mod is not None and getattr(mod, "call", None) is orig:
            mod.call = rec
    return HF


# ---- the raw conv launchers' plain inputs ---------------------------------------------------

ROWS = []


def _dense(HF, t):
    """(pointer % 256, batch stride) as the raw launcher will see the operand after nchw() (a copy
    it makes is a fresh allocation: 256-byte aligned, dense)."""
    if t is None:
        return None, 0
    t4, bs = HF.nchw(t)
    return (t4.data_ptr() % 256 if t4.data_ptr() == t.data_ptr() else 0), int(bs)


def _form(names):
    if any(n in ("dsgan_pw_fwd_io_ws", "dsgan_pw_dgrad_io_ws") for n in names):
        return "io_ws"
    if "dsgan_pw_gemm" in names:
        return "gemm"
    if "dsgan_wconv_db" in names:
        return "db"
    if "dsgan_wconv" in names:
        return "plain"
    return None


def _wshape(w):
    return (tuple(w.shape) if w.dim() == 4 else (w.shape[0], w.shape[1], 1, 1))


def _finish(HF, row, n0, c0):
    fam = HF.IGEMM_TIMER.rec[-1][4] if len(HF.IGEMM_TIMER.rec) > n0 else None
    form = _form([n for n, _ in CALLS[c0:]])
    row.update(prec=HF.get_precision(), pglast=bool(HF.PGLAST[0]), db_fold=bool(HF.WCONV_DB_FOLD), fam=fam,
               form=form if fam in ("pwgemm_kernel", "wconv_kernel") else None)
    ROWS.append(row)


def wrap_raw(HF):
    fwd, dgrad, wgrad = HF.conv_fwd_raw, HF.conv_dgrad_raw, HF.conv_wgrad_raw

    def conv_fwd_raw(x, w, b, stride, pad, act=None, out=None, pre=None, accumulate=False, xact=None):
        xp, xbs = _dense(HF, x)
        pp, pbs = _dense(HF, pre)
        N, Cin, H, W = x.shape
        Cout, _, KH, KW = _wshape(w)
        n0, c0 = len(HF.IGEMM_TIMER.rec), len(CALLS)
        y = fwd(x, w, b, stride, pad, act, out, pre, accumulate, xact)
        yp, ybs = _dense(HF, y)
        _finish(HF, dict(op="fwd", N=N, Cin=Cin, H=H, W=W, Cout=Cout, KH=KH, KW=KW, stride=stride, pad=pad,
                         xbs=xbs, ybs=ybs, pbs=pbs, x_ptr=xp, y_ptr=yp, w_ptr=w.data_ptr() % 256, pre_ptr=pp,
                         w_dim=w.dim(), w_contig=bool(w.is_contiguous()), act=act, xact=xact,
                         has_bias=b is not None, accumulate=bool(accumulate)), n0, c0)
        return y

    def conv_dgrad_raw(dy, w, x_shape, stride, pad, bias=None, act=None, gpre=None, gact=None, out=None,
                       accumulate=False):
        dyp, dybs = _dense(HF, dy)
        gp, gbs = _dense(HF, gpre)
        N, Cin, H, W = x_shape
        Cout, _, KH, KW = _wshape(w)
        n0, c0 = len(HF.IGEMM_TIMER.rec), len(CALLS)
        dx = dgrad(dy, w, x_shape, stride, pad, bias, act, gpre, gact, out, accumulate)
        dxp, dxbs = _dense(HF, dx)
        _finish(HF, dict(op="dgrad", N=N, Cin=Cin, H=H, W=W, Cout=Cout, KH=KH, KW=KW, stride=stride, pad=pad,
                         Ho=dy.shape[2], Wo=dy.shape[3], dybs=dybs, dxbs=dxbs, gbs=gbs, dy_ptr=dyp, dx_ptr=dxp,
                         w_ptr=w.data_ptr() % 256, gpre_ptr=gp, w_dim=w.dim(), w_contig=bool(w.is_contiguous()),
                         act=act, gact=gact, has_bias=bias is not None, accumulate=bool(accumulate)), n0, c0)
        return dx

    def conv_wgrad_raw(dy, x, dw, stride, pad, xact=None, db=None):
        dyp, dybs = _dense(HF, dy)
        xp, xbs = _dense(HF, x)
        N, Cin, H, W = x.shape
        KH, KW = (dw.shape[2], dw.shape[3]) if dw.dim() == 4 else (1, 1)
        n0, c0 = len(HF.IGEMM_TIMER.rec), len(CALLS)
        did = wgrad(dy, x, dw, stride, pad, xact, db)
        _finish(HF, dict(op="wgrad", N=N, Cin=Cin, H=H, W=W, Cout=dy.shape[1], KH=KH, KW=KW, stride=stride,
                         pad=pad, dybs=dybs, xbs=xbs, dy_ptr=dyp, x_ptr=xp, w_dim=dw.dim(),
                         w_contig=bool(dw.is_contiguous()), xact=xact, has_db=db is not None), n0, c0)
        return did

    HF.conv_fwd_raw, HF.conv_dgrad_raw, HF.conv_wgrad_raw = conv_fwd_raw, conv_dgrad_raw, conv_wgrad_raw


# ---- what is recorded -------------------------------------------------------------------------

CONFIGS = {"a": ("bf16", 16, 256), "b": ("fp32", 2, 64)}

# (precision, op, N, Cin, H, W, Cout, K, stride, pad, extras): raw calls that reach the families a
# training step at either config does not
EXTRA = [
    ("fp32", "fwd", 1, 16, 8, 8, 16, 3, 1, 1, {}),                       # igemm
    ("fp32", "dgrad", 1, 16, 8, 8, 16, 3, 1, 1, {}),
    ("fp32", "wgrad", 1, 16, 8, 8, 16, 3, 1, 1, {}),
    ("fp32", "wgrad", 1, 16, 16, 16, 3, 3, 1, 1, {}),                    # wgrad_small (no thin3: W % 256)
    ("bf16", "fwd", 1, 32, 8, 8, 16, 3, 2, 1, {}),                       # tconv fwd (3x3 stride 2: no pconv)
    ("bf16", "dgrad", 1, 16, 8, 8, 32, 3, 1, 1, {"bias": True}),         # tconv stride 1 (bias: no pconv)
    ("bf16", "dgrad", 1, 16, 7, 7, 32, 3, 2, 1, {}),                     # tconv stride 2 (odd W: no pconvt)
    ("bf16", "fwd", 1, 32, 16, 16, 32, 1, 1, 0, {"xact": "gelu"}),       # pwgemm, the dsgan_pw_gemm form
    ("bf16", "dgrad", 1, 32, 16, 16, 32, 1, 1, 0, {"gpre": True, "gact": "gelu"}),
    ("bf16", "wgrad", 1, 32, 16, 16, 32, 1, 1, 0, {}),
    ("bf16", "wgrad", 1, 32, 16, 16, 32, 4, 2, 1, {}),                   # wconv without a bias grad
]


def run_extra(HF, torch):
    g = torch.Generator().manual_seed(7)
    dev = "cuda"

    def rnd(*shape):
        return torch.randn(*shape, generator=g).to(dev)
    for prec, op, N, Cin, H, W, Cout, K, s, p, ex in EXTRA:
        HF.set_precision(prec)
        Ho, Wo = (H + 2 * p - K) // s + 1, (W + 2 * p - K) // s + 1
        w = rnd(Cout, Cin, K, K)
        if op == "fwd":
            HF.conv_fwd_raw(rnd(N, Cin, H, W), w, rnd(Cout), s, p, xact=ex.get("xact"))
        elif op == "dgrad":
            HF.conv_dgrad_raw(rnd(N, Cout, Ho, Wo), w, (N, Cin, H, W), s, p, bias=rnd(Cin) if ex.get("bias") else None,
                              gpre=rnd(N, Cin, H, W) if ex.get("gpre") else None, gact=ex.get("gact"))
        else:
            HF.conv_wgrad_raw(rnd(N, Cout, Ho, Wo), rnd(N, Cin, H, W), torch.zeros_like(w), s, p)
        torch.cuda.synchronize()
    HF.set_precision("fp32")


def run_steps(HF, torch, prec, batch, size, steps):
    from options.train_options import default_train_opt
    from models import create_model
    from oracle.recipe import synth_pair
    torch.manual_seed(20)
    m = create_model(default_train_opt(gpu_ids=[0], precision=prec, batchSize=batch, cuda_graph=0))
    A, B = synth_pair(batch, size, seed=0)
    m.set_input({"A": A.cuda(), "B": B.cuda(), "A_paths": [""] * batch, "B_paths": [""] * batch})
    torch.cuda.synchronize()
    del CALLS[:], ROWS[:]   # the model's construction is not part of a step
    for _ in range(steps):
        m.optimize_parameters()
    torch.cuda.synchronize()


def record(config, out, steps):
    import torch
    HF = install()
    wrap_raw(HF)
    # the timer's records carry the family each raw launcher reports; switched on without the
    # library's kernel-only event pairs, which nothing here reads
    HF.IGEMM_TIMER._on = True
    if config == "extra":
        run_extra(HF, torch)
    else:
        run_steps(HF, torch, *CONFIGS[config], steps)
    os.makedirs(out, exist_ok=True)
    with open(os.path.join(out, "trace_%s.txt" % config), "w") as f:
        for name, args in CALLS:
            f.write(name + " " + " ".join(args) + "\n")
    with open(os.path.join(out, "rows_%s.json" % config), "w") as f:
        json.dump(ROWS, f)
    fams = collections.Counter((r["op"], r["fam"], r["form"]) for r in ROWS)
    print("%s: %d calls, %d raw conv calls" % (config, len(CALLS), len(ROWS)))
    for k, n in sorted(fams.items(), key=str):
        print("  %-6s %-20s %-6s %d" % (k[0], k[1], k[2], n))


# ---- compare / merge (no GPU) -------------------------------------------------------------------

def _scratch_slots(line_a, line_b):
    """Positions where a null scratch pointer with size 0 stands against a pointer with size 0."""
    a, b = line_a.split(), line_b.split()
    if len(a) != len(b) or a[0] != b[0]:
        return None
    slots = []
    for i in range(1, len(a)):
        if a[i] == b[i]:
            continue
        if (i + 1 < len(a) and a[i + 1] == "0" and b[i + 1] == "0" and {a[i], b[i]} <= {"null", "p0"}):
            slots.append(i)
        else:
            return None
    return slots


def compare(old, new):
    A = open(old).read().splitlines()
    B = open(new).read().splitlines()
    ca = collections.Counter(l.split()[0] for l in A)
    cb = collections.Counter(l.split()[0] for l in B)
    print("%-32s %8s %8s" % ("entry point", "old", "new"))
    for k in sorted(set(ca) | set(cb)):
        print("%-32s %8d %8d%s" % (k, ca[k], cb[k], "" if ca[k] == cb[k] else "   <-- differs"))
    print("total %d / %d calls" % (len(A), len(B)))
    bad, norm = [], collections.Counter()
    for i, (a, b) in enumerate(zip(A, B)):
        if a == b:
            continue
        s = _scratch_slots(a, b)
        if s is None:
            bad.append((i, a, b))
        else:
            norm[a.split()[0]] += 1
    if len(A) != len(B):
        bad.append((min(len(A), len(B)), "<length %d>" % len(A), "<length %d>" % len(B)))
    for name, n in sorted(norm.items()):
        print("permitted: %s: %d calls pass (null, 0) scratch where the other tree passes a zero-element tensor"
              % (name, n))
    for i, a, b in bad[:40]:
        print("call %d differs:\n  old %s\n  new %s" % (i, a, b))
    print("identical" if not bad and not norm else
          "identical but for the permitted scratch normalisation" if not bad else "DIFFERENT: %d calls" % len(bad))
    return 1 if bad else 0


def merge(files, table):
    seen, rows = set(), []
    for fn in files:
        for r in json.load(open(fn)):
            k = json.dumps(r, sort_keys=True)
            if k not in seen:
                seen.add(k)
                rows.append(r)
    rows.sort(key=lambda r: (r["op"], r["prec"], str(r["fam"]), str(r["form"]), json.dumps(r, sort_keys=True)))
    with open(table, "w") as f:
        f.write("[\n" + ",\n".join(json.dumps(r, sort_keys=True) for r in rows) + "\n]\n")
    print("%d rows" % len(rows))
    for k, n in sorted(collections.Counter((r["fam"], r["form"]) for r in rows).items(), key=str):
        print("  %-20s %-6s %d" % (k[0], k[1], n))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", choices=["a", "b", "extra"])
    ap.add_argument("--out", default="call_trace_out")
    ap.add_argument("--steps", type=int, default=1)
    ap.add_argument("--compare", nargs=2)
    ap.add_argument("--merge", nargs="+")
    ap.add_argument("--table")
    a = ap.parse_args()
    if a.compare:
        sys.exit(compare(*a.compare))
    if a.merge:
        return merge(a.merge, a.table)
    record(a.config, a.out, a.steps)


if __name__ == "__main__":
    main()
