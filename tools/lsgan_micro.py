"""Measurements of the --no_lsgan / multi-scale-discriminator path:

  pool      AvgPool2d(3, 2, 1, count_include_pad=False) forward and backward at (32, 6, 256, 256), both
            launch forms, device events over rotating buffers (8 x 50 MB, more than the 256 MB
            last-level cache holds), algorithmic bytes / time;
  families  the kernel family and time of every conv launch of one multi-D forward + backward
            (input and weight grads) at 256^2, batch 32 (the stacked D pass of batch 16), bf16;
  step      ms/step of optimize_parameters at 256^2, batch 16, bf16: the default objective, --no_lsgan
            with the basic D and with the multi D (host clock around synchronised windows, graph step).

usage: python tools/lsgan_micro.py pool|families|step [--out FILE.json]"""
import argparse
import json
import os
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [REPO, os.path.join(REPO, "ds-gan_amd")]

import torch  # noqa: E402


def _events(fn, bufs, warm=16, iters=160):
    for i in range(warm):
        fn(bufs[i % len(bufs)])
    torch.cuda.synchronize()
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(iters)]
    for i, (e0, e1) in enumerate(ev):
        e0.record()
        fn(bufs[i % len(bufs)])
        e1.record()
    torch.cuda.synchronize()
    t = sorted(e0.elapsed_time(e1) * 1e3 for e0, e1 in ev)
    return {"median_us": t[len(t) // 2], "min_us": t[0], "p90_us": t[int(len(t) * 0.9)], "iters": iters}


def pool():
    from dsgan_hip import functional as HF
    N, C, H, W = 32, 6, 256, 256
    xs = [torch.randn(N, C, H, W, device="cuda") for _ in range(8)]
    ys = [torch.empty(N, C, H // 2, W // 2, device="cuda") for _ in range(8)]
    dys = [torch.randn(N, C, H // 2, W // 2, device="cuda") for _ in range(8)]
    dxs = [torch.empty(N, C, H, W, device="cuda") for _ in range(8)]
    nb = (xs[0].numel() + ys[0].numel()) * 4
    out = {"shape": [N, C, H, W], "bytes": nb}
    for form, fast in (("fast", True), ("scalar", False)):
        HF.AVGPOOL_FAST[0] = fast
        f = _events(lambda p: HF.avg_pool3s2_raw(p[0], out=p[1]), list(zip(xs, ys)))
        b = _events(lambda p: HF.avg_pool3s2_bwd_raw(p[0], (N, C, H, W), out=p[1]), list(zip(dys, dxs)))
        ba = _events(lambda p: HF.avg_pool3s2_bwd_raw(p[0], (N, C, H, W), out=p[1], accumulate=True), list(zip(dys, dxs)))
        for k, r, by in (("fwd", f, nb), ("bwd", b, nb), ("bwd_accumulate", ba, nb + xs[0].numel() * 4)):
            r["TB_per_s"] = by / r["median_us"] / 1e6
            out["%s_%s" % (k, form)] = r
            print("%-16s %-6s median %7.1f us  min %7.1f  p90 %7.1f  %.2f TB/s (%.1f MB)"
                  % (k, form, r["median_us"], r["min_us"], r["p90_us"], r["TB_per_s"], by / 1e6))
    HF.AVGPOOL_FAST[0] = True
    return out


def families():
    from dsgan_hip import functional as HF
    from models.networks import define_D, GANLoss_multi
    HF.set_precision("bf16")
    torch.manual_seed(20)
    net = define_D(6, 64, "multi", 3, "instance", True, "normal", [0])
    x = torch.randn(32, 6, 256, 256, device="cuda").requires_grad_()
    crit = GANLoss_multi(True)
    for timed in (False, False, True):
        HF.IGEMM_TIMER.rec = []
        HF.IGEMM_TIMER.on = timed
        crit(net(x), True).backward()
        torch.cuda.synchronize()
    HF.IGEMM_TIMER.on = False
    rows = []
    for e0, e1, fl, tag, fam, by in HF.IGEMM_TIMER.rec:
        ms = e0.elapsed_time(e1)
        rows.append({"family": fam, "tag": list(tag), "us": ms * 1e3, "TF_per_s": fl / ms / 1e9})
        print("%8.1f us  %-20s %-44s %6.1f TF/s" % (ms * 1e3, fam, str(tag), fl / ms / 1e9))
    tot = {}
    for r in rows:
        tot[r["family"]] = tot.get(r["family"], 0.0) + r["us"]
    print("per family (us):", {k: round(v, 1) for k, v in sorted(tot.items(), key=lambda kv: -kv[1])})
    return {"launches": rows, "family_us": tot}


def step():
    from options.train_options import default_train_opt
    from models import create_model
    from oracle.recipe import synth_pair
    out = {}
    A, B = synth_pair(16, 256, seed=0)
    inp = {"A": A.cuda(), "B": B.cuda(), "A_paths": [""] * 16, "B_paths": [""] * 16}
    cases = (("default", {}), ("no_lsgan_basic", {"no_lsgan": True}),
             ("no_lsgan_multi", {"no_lsgan": True, "which_model_netD": "multi"}))
    models = {}
    for name, kw in cases:
        torch.manual_seed(20)
        m = create_model(default_train_opt(gpu_ids=[0], precision="bf16", batchSize=16, **kw))
        for _ in range(5):   # eager warm-up, capture, replays
            m.set_input(inp)
            m.optimize_parameters()
        torch.cuda.synchronize()
        models[name] = m
    for rnd in range(3):   # the three cases alternate, three windows each
        for name, _ in cases:
            m = models[name]
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(20):
                m.set_input(inp)
                m.optimize_parameters()
            torch.cuda.synchronize()
            out.setdefault(name, []).append((time.perf_counter() - t0) / 20 * 1e3)
    for name, v in out.items():
        print("%-16s ms/step %s  mean %.2f  (graph step %s, skipped %s)"
              % (name, ["%.2f" % x for x in v], sum(v) / len(v), bool(models[name]._graphs), models[name].nonfinite_report()))
    return out


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("what", choices=["pool", "families", "step"])
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import dsgan_hip
    dsgan_hip.require_gpu()
    res = {"pool": pool, "families": families, "step": step}[a.what]()
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)
