"""Measurements of the --norm batch path ("BatchNorm PatchGAN"):

  layers  BatchNorm2d + LeakyReLU forward and backward (HF.batchnorm_raw / batchnorm_bwd_raw) against
          the InstanceNorm + LeakyReLU launches of the same shape (HF.instnorm_raw / instnorm_bwd_raw:
          code this path does not touch) at the three norm shapes of the default D at 256^2, batch 16,
          ndf 32, and, where both apply, both BatchNorm launch forms (dsgan_batchnorm_tune).  Each leg
          is a captured graph of 16 calls over 8 rotating buffer sets (more than the 256 MB last-level
          cache holds at the two large shapes), replayed between device events: device time per
          call, without the host's launch cost;
  step    ms/step of optimize_parameters at 256^2, batch 16, bf16, graph step: --norm batch against
          --norm instance with the two-pass D (d_batch off: the like-for-like D step), the instance
          leg twice, the legs alternating in one process (host clock around synchronised windows).

usage: python tools/bn_micro.py layers|step [--out FILE.json]"""
import argparse
import json
import os
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [REPO, os.path.join(REPO, "ds-gan_amd")]

import torch  # noqa: E402

SHAPES = [(16, 64, 64, 64), (16, 128, 32, 32), (16, 256, 31, 31)]
NBUF, REPS = 8, 16


def _graph_us(fn, warm=3, iters=40):
    """Median / min device time per call of fn(i), i = 0..REPS-1, replayed from one captured graph."""
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
    return {"median_us": t[len(t) // 2], "min_us": t[0], "p90_us": t[int(len(t) * 0.9)], "graph_calls": REPS,
            "replays": iters}


def layers():
    from dsgan_hip import _lib
    from dsgan_hip import functional as HF
    lib = _lib.load()
    out = {}
    for N, C, H, W in SHAPES:
        xs = [torch.randn(N, C, H, W, device="cuda") for _ in range(NBUF)]
        ys = [torch.empty(N, C, H, W, device="cuda") for _ in range(NBUF)]
        dys = [torch.randn(N, C, H, W, device="cuda") for _ in range(NBUF)]
        bn = torch.nn.BatchNorm2d(C).cuda()
        gw, gb = torch.zeros(C, device="cuda"), torch.zeros(C, device="cuda")
        row = {"bytes_per_tensor": xs[0].numel() * 4}
        _, imean, irstd = HF.instnorm_raw(xs[0], None, None, "lrelu", out=ys[0])
        row["in_fwd"] = _graph_us(lambda i: HF.instnorm_raw(xs[i % NBUF], None, None, "lrelu", out=ys[i % NBUF]))
        row["in_bwd"] = _graph_us(lambda i: HF.instnorm_bwd_raw(dys[i % NBUF], xs[i % NBUF], None, None, imean, irstd,
                                                                "lrelu", False, False))
        forms = [(0, "bn")]
        if N * H * W <= 16384:   # both forms apply: price them
            forms += [(1, "bn_one"), (2, "bn_split")]
        for knob, tag in forms:
            lib.dsgan_batchnorm_tune(0, knob)
            _, mean, rstd = HF.batchnorm_raw(xs[0], bn.weight, bn.bias, bn.running_mean, bn.running_var,
                                             bn.num_batches_tracked, True, 0.1, 1e-5, "lrelu", out=ys[0])
            row[tag + "_form"] = int(lib.dsgan_batchnorm_plan(N, C, H * W))
            row[tag + "_fwd"] = _graph_us(lambda i: HF.batchnorm_raw(
                xs[i % NBUF], bn.weight, bn.bias, bn.running_mean, bn.running_var, bn.num_batches_tracked, True, 0.1,
                1e-5, "lrelu", out=ys[i % NBUF]))
            row[tag + "_bwd"] = _graph_us(lambda i: HF.batchnorm_bwd_raw(
                dys[i % NBUF], xs[i % NBUF], bn.weight, bn.bias, mean, rstd, "lrelu", True, gw, gb))
        lib.dsgan_batchnorm_tune(0, 0)
        for d in ("fwd", "bwd"):
            row["ratio_" + d] = row["bn_" + d]["median_us"] / row["in_" + d]["median_us"]
        out["%dx%dx%dx%d" % (N, C, H, W)] = row
        print("(%d, %d, %d, %d): " % (N, C, H, W) + "  ".join(
            "%s %.1f us" % (k, v["median_us"]) for k, v in row.items() if isinstance(v, dict))
            + "  | form %d, BN / IN fwd %.2fx bwd %.2fx" % (row["bn_form"], row["ratio_fwd"], row["ratio_bwd"]))
        del xs, ys, dys
        torch.cuda.empty_cache()
    return out


def step():
    from options.train_options import default_train_opt
    from models import create_model
    from oracle.recipe import synth_pair
    out = {}
    A, B = synth_pair(16, 256, seed=0)
    inp = {"A": A.cuda(), "B": B.cuda(), "A_paths": [""] * 16, "B_paths": [""] * 16}
    cases = (("instance_two_pass_a", "instance"), ("batch", "batch"), ("instance_two_pass_b", "instance"))
    models = {}
    for name, norm in cases:
        torch.manual_seed(20)
        m = create_model(default_train_opt(gpu_ids=[0], precision="bf16", batchSize=16, norm=norm))
        m.d_batch = False
        for _ in range(5):   # eager warm-up, capture, replays
            m.set_input(inp)
            m.optimize_parameters()
        torch.cuda.synchronize()
        models[name] = m
    for rnd in range(3):   # the legs alternate, three windows each
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
        print("%-22s ms/step %s  mean %.3f  (graph step %s, skipped %s)"
              % (name, ["%.3f" % x for x in v], sum(v) / len(v), bool(models[name]._graphs), models[name].nonfinite_report()))
    mean = {k: sum(v) / len(v) for k, v in out.items()}
    ia, ib = mean["instance_two_pass_a"], mean["instance_two_pass_b"]
    out["summary"] = {"instance_mean": (ia + ib) / 2, "instance_spread": abs(ia - ib), "batch_mean": mean["batch"],
                      "batch_over_instance": mean["batch"] / ((ia + ib) / 2),
                      "bar_ms": max(ia, ib) + 0.01 * (ia + ib) / 2}
    print("batch %.3f ms/step vs instance %.3f / %.3f (spread %.3f): %+.2f %%, bar %.3f"
          % (mean["batch"], ia, ib, abs(ia - ib), 100 * (out["summary"]["batch_over_instance"] - 1), out["summary"]["bar_ms"]))
    return out


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("what", choices=["layers", "step"])
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import dsgan_hip
    dsgan_hip.require_gpu()
    res = {"layers": layers, "step": step}[a.what]()
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)
