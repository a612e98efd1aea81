"""Measurements of --diffaug ("Differentiable augmentation"):

  kernel  functional.diffaug_cat forward and backward (full policy) beside functional.cat_channels on the
          same shape (batch 16, 3 + 3 channels, 256 x 256), alternately in one process: device time per call
          from a captured graph of 8 calls over 2 rotating buffer sets, median of the replays, several
          rounds.  Bytes are counted from the element counts: cat_channels reads and writes the 6-channel
          batch once (2 x 25.2 MB); the augmenting forward moves the same plus one more read of the image
          half by its sum kernel (+ 12.6 MB); the backward reads the image half of dy twice and writes dx
          (3 x 12.6 MB).  The forward with the colour off (no sum kernel) is timed too;
  step    ms/step of optimize_parameters at 256^2, batch 16, bf16 (graph step) with --diffaug off and
          color,translation,cutout, alternately.

usage: python tools/diffaug_micro.py kernel|step [--out FILE.json]"""
import argparse
import json
import os
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [REPO, os.path.join(REPO, "ds-gan_amd")]

import torch  # noqa: E402

N, CA, CB, SIZE = 16, 3, 3, 256
NBUF, REPS = 2, 8
FULL = "color,translation,cutout"


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


def kernel(rounds=3):
    from dsgan_hip import functional as HF
    from dsgan_hip._lib import call, ptr, stream as cur
    from dsgan_hip.diffaug import policy_bits
    sets = []
    for _ in range(NBUF):
        sets.append((torch.randn(N, CA, SIZE, SIZE, device="cuda"), torch.randn(N, CB, SIZE, SIZE, device="cuda"),
                     torch.empty(N, CA + CB, SIZE, SIZE, device="cuda"), torch.randn(N, CA + CB, SIZE, SIZE, device="cuda"),
                     torch.empty(N, CB, SIZE, SIZE, device="cuda")))
    st = HF.DiffAugState(20, 0xFFFF, torch.zeros(1, device="cuda", dtype=torch.int64))
    used = torch.zeros(1, device="cuda", dtype=torch.int64)
    ws = torch.empty(HF._lib.load().dsgan_diffaug_workspace(N, CB, SIZE, SIZE), device="cuda")
    E = SIZE * SIZE

    def cat(i):
        a, b, y, _, _ = sets[i % NBUF]
        HF.copy_into(y[:, :CA], a)
        HF.copy_into(y[:, CA:], b)

    def fwd(bits):
        def f(i):
            a, b, y, _, _ = sets[i % NBUF]
            call("dsgan_diffaug_fwd", ptr(a), CA * E, ptr(b), CB * E, ptr(y), (CA + CB) * E, N, CA, CB, SIZE, SIZE, bits,
                 st.seed, st.stream, ptr(st.counter), ptr(used), N, ptr(ws), ws.numel(), cur())
        return f

    def bwd(i):
        _, _, _, dy, dx = sets[i % NBUF]
        call("dsgan_diffaug_bwd", ptr(dy), (CA + CB) * E, ptr(dx), CB * E, N, CA, CB, SIZE, SIZE, policy_bits(FULL), st.seed,
             st.stream, ptr(used), N, ptr(ws), ws.numel(), cur())

    full = 4.0 * N * (CA + CB) * E   # bytes of the 6-channel batch
    img = 4.0 * N * CB * E
    legs = (("cat_channels", cat, 2 * full), ("diffaug_fwd", fwd(policy_bits(FULL)), 2 * full + img),
            ("diffaug_fwd_nocolor", fwd(policy_bits("translation,cutout")), 2 * full), ("diffaug_bwd", bwd, 3 * img))
    out = {"shape": [N, CA, CB, SIZE, SIZE], "rounds": []}
    for r in range(rounds):
        row = {}
        for name, fn, nbytes in legs:
            us = _graph_us(fn)
            row[name] = {"us": us, "bytes": nbytes, "TBps": nbytes / us / 1e6}
        out["rounds"].append(row)
        print("round %d: " % r + "  ".join("%s %.1f us %.2f TB/s" % (k, v["us"], v["TBps"]) for k, v in row.items()))
    return out


def step(rounds=3):
    from options.train_options import default_train_opt
    from models import create_model
    from oracle.recipe import synth_pair
    A, B = synth_pair(N, SIZE, seed=0)
    inp = {"A": A.cuda(), "B": B.cuda(), "A_paths": [""] * N, "B_paths": [""] * N}
    models = {}
    for policy in ("", FULL):
        torch.manual_seed(20)
        m = create_model(default_train_opt(gpu_ids=[0], precision="bf16", batchSize=N, diffaug=policy))
        for _ in range(5):   # eager warm-up, capture, replays
            m.set_input(inp)
            m.optimize_parameters()
        torch.cuda.synchronize()
        models[policy] = m
    out = {"ms_per_step": {p or "off": [] for p in models}, "graph_step": {p or "off": bool(m._graphs) for p, m in models.items()}}
    for _ in range(rounds):
        for policy, m in models.items():
            t0 = time.perf_counter()
            for _ in range(20):
                m.set_input(inp)
                m.optimize_parameters()
            torch.cuda.synchronize()
            out["ms_per_step"][policy or "off"].append((time.perf_counter() - t0) / 20 * 1e3)
    for p, ms in out["ms_per_step"].items():
        print("--diffaug %-26s ms/step %s (graph step %s)" % (p, ["%.3f" % x for x in ms], out["graph_step"][p]))
    return out


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("what", choices=["kernel", "step"])
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import dsgan_hip
    dsgan_hip.require_gpu()
    res = {"kernel": kernel, "step": step}[a.what]()
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)
