"""Measurements of the U-Net generator ("U-Net generator"):

  layers  unet_128, ngf 64, batch 16, 256^2, bf16: per conv layer (the down conv and the ConvTranspose of
          every level; forward, data-grad, weight-grad) the kernel family taken and the device time per
          call, from a captured graph of 8 calls over 4 rotating buffer sets, median of the replays;
  stream  the new streaming kernels against launches that move the same tensor, in the same run:
          prelu_cat forward / backward against instnorm forward / backward at the two largest
          concatenations, dropout against dsgan_copy_strided at the two dropout tensors.  Bytes are counted
          from shapes (forward 2 tensors, backward 3, dropout / copy 2);
  step    ms/step of optimize_parameters at 256^2, batch 16, bf16 with --which_model_netG unet_128 (both
          norms, with dropout), and one eager step under the launch timers: the share of the timed device
          time per kernel family (what fell to igemm_kernel, what the norms of the tiny planes cost).

usage: python tools/unet_micro.py layers|stream|step [--out FILE.json]"""
import argparse
import json
import os
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [REPO, os.path.join(REPO, "ds-gan_amd")]

import torch  # noqa: E402

N, SIZE, NGF, DOWNS = 16, 256, 64, 7
NBUF, REPS = 4, 8


def _graph_us(fn, warm=3, iters=30):
    """Median device time per call of fn(i), i = 0..REPS-1, replayed from one captured graph."""
    for i in range(REPS):
        fn(i)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        for i in range(REPS):
            fn(i)
    for _ in range(warm):
        g.replay()
    torch.cuda.synchronize()
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(iters)]
    for e0, e1 in ev:
        e0.record()
        g.replay()
        e1.record()
    torch.cuda.synchronize()
    t = sorted(e0.elapsed_time(e1) * 1e3 / REPS for e0, e1 in ev)
    return t[len(t) // 2]


def _levels():
    lv = [(3, NGF, 3)] + [(NGF * min(2 ** i, 8), NGF * min(2 ** (i + 1), 8), None) for i in range(DOWNS - 1)]
    return lv   # (input channels of the down conv, inner channels, output_nc for the outermost)


def layers():
    from dsgan_hip import functional as HF
    HF.set_precision("bf16")
    out = []
    s = SIZE
    rnd = lambda *sh: [torch.randn(*sh, device="cuda") for _ in range(NBUF)]   # noqa: E731
    for li, (cin, inner, _) in enumerate(_levels()):
        h = s // 2
        innermost = li == DOWNS - 1
        convs = [("down", cin, inner, False), ("up", cin, inner if innermost else 2 * inner, True)]
        for name, c_small, c_big, transposed in convs:
            # the conv whose forward is the down conv / whose data-grad is the ConvTranspose: [c_big, c_small, 4, 4]
            w = torch.randn(c_big, c_small, 4, 4, device="cuda") / (c_small * 16) ** 0.5
            xs, ys = rnd(N, c_small, s, s), rnd(N, c_big, h, h)
            dw = torch.zeros_like(w)
            fam = {}

            def timed(fn, key):
                HF.IGEMM_TIMER.on = True
                HF.IGEMM_TIMER.reset()
                fn(0)
                fam[key] = HF.IGEMM_TIMER.rec[-1][4]
                HF.IGEMM_TIMER.on = False
                return _graph_us(fn)
            t = {"conv_fwd": timed(lambda i: HF.conv_fwd_raw(xs[i % NBUF], w, None, 2, 1, out=ys[i % NBUF]), "conv_fwd"),
                 "conv_dgrad": timed(lambda i: HF.conv_dgrad_raw(ys[i % NBUF], w, (N, c_small, s, s), 2, 1, out=xs[i % NBUF]),
                                     "conv_dgrad"),
                 "conv_wgrad": timed(lambda i: HF.conv_wgrad_raw(ys[i % NBUF], xs[i % NBUF], dw, 2, 1), "conv_wgrad")}
            role = ({"conv_fwd": "dx", "conv_dgrad": "forward", "conv_wgrad": "dw"} if transposed else
                    {"conv_fwd": "forward", "conv_dgrad": "dx", "conv_wgrad": "dw"})
            for k, us in t.items():
                row = {"layer": "L%d.%s" % (li, name), "pass": role[k], "channels": [c_small, c_big], "plane": [s, h],
                       "family": fam[k], "us": us}
                out.append(row)
                print("L%d.%-4s %-7s %4d <-> %4d  %3d^2 <-> %3d^2  %-18s %9.1f us" % (li, name, role[k], c_small, c_big, s, h,
                                                                                     fam[k], us))
            del xs, ys
            torch.cuda.empty_cache()
        s = h
    tot = sum(r["us"] for r in out)
    ig = sum(r["us"] for r in out if r["family"] == "igemm_kernel")
    print("conv launches: %.1f us per step's worth, igemm_kernel %.1f us (%.1f %%)" % (tot, ig, 100 * ig / tot))
    HF.set_precision("fp32")
    return {"rows": out, "total_us": tot, "igemm_us": ig}


def stream():
    from dsgan_hip import functional as HF
    from dsgan_hip._lib import call, ptr, stream as cur
    out = {}
    for (C, S) in ((NGF, SIZE // 2), (2 * NGF, SIZE // 4)):
        a = [torch.randn(N, C, S, S, device="cuda") for _ in range(NBUF)]
        b = [torch.randn(N, C, S, S, device="cuda") for _ in range(NBUF)]
        x = [torch.randn(N, 2 * C, S, S, device="cuda") for _ in range(NBUF)]
        y = [torch.empty(N, 2 * C, S, S, device="cuda") for _ in range(NBUF)]
        w = torch.nn.Parameter(torch.tensor([0.25], device="cuda"))
        w.grad = torch.zeros(1, device="cuda")
        nbytes = x[0].numel() * 4
        E = 2 * C * S * S
        ws = torch.empty(int(HF._lib.load().dsgan_prelu_workspace(N, E)), device="cuda")
        _, mean, rstd = HF.instnorm_raw(x[0], None, None, "lrelu", out=y[0])
        row = {"bytes_per_tensor": nbytes}
        us = {
            "prelu_fwd": _graph_us(lambda i: call("dsgan_prelu_fwd", ptr(a[i % NBUF]), C * S * S, C * S * S, ptr(b[i % NBUF]),
                                                  C * S * S, C * S * S, ptr(w), ptr(y[i % NBUF]), E, N, cur())),
            "instnorm_fwd": _graph_us(lambda i: HF.instnorm_raw(x[i % NBUF], None, None, "lrelu", out=y[i % NBUF])),
            "prelu_bwd": _graph_us(lambda i: call("dsgan_prelu_bwd", ptr(x[i % NBUF]), E, ptr(a[i % NBUF]), C * S * S,
                                                  C * S * S, ptr(b[i % NBUF]), C * S * S, C * S * S, ptr(w), ptr(y[i % NBUF]),
                                                  E, ptr(y[i % NBUF][:, C:]), E, ptr(w.grad), N, ptr(ws), ws.numel(), cur())),
            "instnorm_bwd": _graph_us(lambda i: HF.instnorm_bwd_raw(y[i % NBUF], x[i % NBUF], None, None, mean, rstd, "lrelu",
                                                                    False, False)),
        }
        for k, t in us.items():
            row[k] = {"us": t, "TBps": (3 if k.endswith("bwd") else 2) * nbytes / t / 1e6}
        row["fwd_ok"] = row["prelu_fwd"]["TBps"] >= row["instnorm_fwd"]["TBps"]
        row["bwd_ok"] = row["prelu_bwd"]["TBps"] >= row["instnorm_bwd"]["TBps"]
        out["cat_%dx%dx%dx%d" % (N, 2 * C, S, S)] = row
        print("cat (%d, %d+%d, %d, %d): " % (N, C, C, S, S) + "  ".join("%s %.1f us %.2f TB/s" % (k, v["us"], v["TBps"])
                                                                      for k, v in row.items() if isinstance(v, dict)))
        del a, b, x, y
        torch.cuda.empty_cache()
    for S in (SIZE // 16, SIZE // 32):
        C = 8 * NGF
        x = [torch.randn(N, C, S, S, device="cuda") for _ in range(NBUF)]
        y = [torch.empty(N, C, S, S, device="cuda") for _ in range(NBUF)]
        st = HF.DropoutState(20, 0, torch.zeros(1, dtype=torch.int64, device="cuda"))
        used = torch.zeros(1, dtype=torch.int64, device="cuda")
        E = C * S * S
        nbytes = x[0].numel() * 4
        us = {"dropout_fwd": _graph_us(lambda i: call("dsgan_dropout_fwd", ptr(x[i % NBUF]), E, ptr(y[i % NBUF]), E, N, E, 20, 0,
                                                      ptr(st.counter), ptr(used), 1 << 31, 2.0, cur())),
              "dropout_bwd": _graph_us(lambda i: call("dsgan_dropout_apply", ptr(x[i % NBUF]), E, ptr(y[i % NBUF]), E, N, E, 20, 0,
                                                      ptr(used), 0, 1 << 31, 2.0, cur())),
              "copy_strided": _graph_us(lambda i: HF.copy_into(y[i % NBUF], x[i % NBUF]))}
        row = {k: {"us": t, "TBps": 2 * nbytes / t / 1e6} for k, t in us.items()}
        row["bytes_per_tensor"] = nbytes
        row["fwd_ok"] = row["dropout_fwd"]["TBps"] >= row["copy_strided"]["TBps"]
        row["bwd_ok"] = row["dropout_bwd"]["TBps"] >= row["copy_strided"]["TBps"]
        out["drop_%dx%dx%dx%d" % (N, C, S, S)] = row
        print("dropout (%d, %d, %d, %d): " % (N, C, S, S) + "  ".join("%s %.1f us %.2f TB/s" % (k, v["us"], v["TBps"])
                                                                     for k, v in row.items() if isinstance(v, dict)))
    return out


def step():
    from dsgan_hip import functional as HF
    from options.train_options import default_train_opt
    from models import create_model
    from oracle.recipe import synth_pair
    out = {}
    A, B = synth_pair(N, SIZE, seed=0)
    inp = {"A": A.cuda(), "B": B.cuda(), "A_paths": [""] * N, "B_paths": [""] * N}
    for norm in ("instance", "batch"):
        torch.manual_seed(20)
        m = create_model(default_train_opt(gpu_ids=[0], precision="bf16", batchSize=N, norm=norm, which_model_netG="unet_128",
                                           ngf=NGF))
        for _ in range(5):   # eager warm-up, capture, replays
            m.set_input(inp)
            m.optimize_parameters()
        torch.cuda.synchronize()
        ms = []
        for _ in range(3):
            t0 = time.perf_counter()
            for _ in range(10):
                m.set_input(inp)
                m.optimize_parameters()
            torch.cuda.synchronize()
            ms.append((time.perf_counter() - t0) / 10 * 1e3)
        # one eager step under the launch timers: device time per kernel family
        m.cuda_graph = False
        HF.IGEMM_TIMER.on = HF.AUX_TIMER.on = True
        HF.IGEMM_TIMER.reset()
        HF.AUX_TIMER.reset()
        m.set_input(inp)
        m.optimize_parameters()
        fam = {k: v[:2] for t in (HF.IGEMM_TIMER, HF.AUX_TIMER) for k, v in t.families().items()}
        tiny = sum(r[0].elapsed_time(r[1]) for r in HF.AUX_TIMER.rec
                   if r[3] and r[3][0] in ("in_fwd", "in_bwd", "bn_fwd", "bn_bwd") and r[3][3] <= 8)
        HF.IGEMM_TIMER.on = HF.AUX_TIMER.on = False
        tot = sum(v[1] for v in fam.values())
        out[norm] = {"ms_per_step": ms, "graph_step": bool(m._graphs), "skipped": m.nonfinite_report(),
                     "families_ms": fam, "timed_ms": tot, "tiny_plane_norm_ms": tiny}
        print("unet_128 --norm %-8s ms/step %s (graph step %s, skipped %s)" % (norm, ["%.3f" % x for x in ms], bool(m._graphs),
                                                                             m.nonfinite_report()))
        print("  eager step, timed launches %.2f ms: " % tot + ", ".join(
            "%s %.2f (%d)" % (k, v[1], v[0]) for k, v in sorted(fam.items(), key=lambda kv: -kv[1][1])))
        print("  igemm_kernel share %.1f %%; norms on planes <= 8x8: %.3f ms (%.1f %%)"
              % (100 * fam.get("igemm_kernel", [0, 0.0])[1] / tot, tiny, 100 * tiny / tot))
        del m
        torch.cuda.empty_cache()
    return out


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("what", choices=["layers", "stream", "step"])
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import dsgan_hip
    dsgan_hip.require_gpu()
    res = {"layers": layers, "stream": stream, "step": step}[a.what]()
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)
