"""Measurements of --spectral_norm ("Spectral normalisation"):

  kernel  the two batched calls a D step adds, dsgan_sn_refresh (iterating) and dsgan_sn_backward, over the
          layers of each discriminator kind (basic, pixel, multi) at --ndf 32 (the default) and 64: device
          time per call from a captured graph of 8 calls, median of the replays, several rounds.  Bytes are
          counted from the element counts E = sum R C: the refresh reads W three times and writes W_sn
          (4 x 4 E), the backward reads G and W_sn, then reads G and dW and writes both (6 x 4 E);
  step    ms/step of optimize_parameters at 256^2, batch 16, bf16 (graph step) with --spectral_norm off and
          on, alternately.  (Flag on is another discriminator: no norm layers, LeakyReLU in the conv
          epilogue, so the difference is not the two calls' cost alone.)

usage: python tools/sn_micro.py kernel|step [--out FILE.json]"""
import argparse
import json
import os
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [REPO, os.path.join(REPO, "ds-gan_amd")]

import torch  # noqa: E402

N, SIZE = 16, 256
REPS = 8


def _graph_us(fn, warm=3, iters=30):
    """Median device time per call of fn(), replayed from one captured graph of REPS calls."""
    for _ in range(REPS):
        fn()
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        for _ in range(REPS):
            fn()
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
    from models.networks import define_D
    out = {"rounds": []}
    tabs = {}
    for ndf in (32, 64):
        for kind in ("basic", "pixel", "multi"):
            net = define_D(6, ndf, kind, 3, "instance", True, "normal", [0], spectral_norm=True)
            t = net.spectral.table()
            tabs["%s/%d" % (kind, ndf)] = (net, t)
    for r in range(rounds):
        row = {}
        for name, (net, t) in tabs.items():
            for leg, fn, mult in (("refresh", lambda: t.refresh(True), 4), ("backward", t.backward, 6)):
                us = _graph_us(fn)
                nbytes = mult * t.nbytes
                row["%s %s" % (name, leg)] = {"layers": len(t.layers), "us": us, "bytes": nbytes, "GBps": nbytes / us / 1e3}
        out["rounds"].append(row)
        print("round %d:\n  " % r + "\n  ".join("%-22s %2d layers %7.1f us %8.1f GB/s" % (k, v["layers"], v["us"], v["GBps"])
                                                for k, v in row.items()))
    return out


def step(rounds=3):
    from options.train_options import default_train_opt
    from models import create_model
    from oracle.recipe import synth_pair
    A, B = synth_pair(N, SIZE, seed=0)
    inp = {"A": A.cuda(), "B": B.cuda(), "A_paths": [""] * N, "B_paths": [""] * N}
    models = {}
    for flag in (False, True):
        torch.manual_seed(20)
        m = create_model(default_train_opt(gpu_ids=[0], precision="bf16", batchSize=N, spectral_norm=flag))
        for _ in range(5):   # eager warm-up, capture, replays
            m.set_input(inp)
            m.optimize_parameters()
        torch.cuda.synchronize()
        models["on" if flag else "off"] = m
    out = {"ms_per_step": {k: [] for k in models}, "graph_step": {k: bool(m._graphs) for k, m in models.items()}}
    for _ in range(rounds):
        for k, m in models.items():
            t0 = time.perf_counter()
            for _ in range(20):
                m.set_input(inp)
                m.optimize_parameters()
            torch.cuda.synchronize()
            out["ms_per_step"][k].append((time.perf_counter() - t0) / 20 * 1e3)
    for k, ms in out["ms_per_step"].items():
        print("--spectral_norm %-3s ms/step %s (graph step %s)" % (k, ["%.3f" % x for x in ms], out["graph_step"][k]))
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
