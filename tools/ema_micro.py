"""Measurements of the generator's moving average ("EMA generator weights"):

  kernel  plain Adam (dsgan_adam_amp, as the bf16 step launches it) against Adam + EMA
          (dsgan_adam_amp_ema) over a buffer of the generator's flat size, alternately in one process:
          device time per call from a captured graph of 8 calls over 2 rotating buffer sets (each set is
          larger than the last-level cache), median of the replays, several rounds.  Bytes are counted
          from the element count: 28 B/element for Adam (p, m, v read and written, g read), 36 with the
          average (ema read and written).  dsgan_swap (16 B/element) is timed the same way;
  step    ms/step of optimize_parameters at 256^2, batch 16, bf16 (graph step) with --ema_decay 0 and 0.999,
          alternately, and the cost of one ema_scope() entry + exit.

usage: python tools/ema_micro.py kernel|step [--out FILE.json]"""
import argparse
import json
import os
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [REPO, os.path.join(REPO, "ds-gan_amd")]

import torch  # noqa: E402

N, SIZE = 16, 256
NBUF, REPS = 2, 8
LR, B1, B2, EPS, DECAY = 2e-4, 0.5, 0.999, 1e-8, 0.999


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


def generator_numel():
    """Elements of the default generator's flat buffer (every tensor padded to 64 elements, flat.py)."""
    from options.train_options import default_train_opt
    from models import networks
    o = default_train_opt(gpu_ids=[0])
    net = networks.define_G(o.input_nc, o.output_nc, o.ngf, o.which_model_netG, o.norm, not o.no_dropout, o.init_type, [0])
    return sum((p.numel() + 63) // 64 * 64 for p in net.parameters())


def kernel(rounds=3):
    from dsgan_hip._lib import call, ptr, stream as cur
    n = generator_numel()
    sets = []
    for _ in range(NBUF):
        p, g = torch.randn(n, device="cuda") * 0.02, torch.randn(n, device="cuda") * 1e-3
        sets.append((p, g, torch.zeros_like(p), torch.zeros_like(p), p.clone()))
    state = torch.tensor([1.0, 0.0, 0.0, 1.0, 1.0], device="cuda")   # the bf16 guard's unit scale, step 1

    def plain(i):
        p, g, m, v, _ = sets[i % NBUF]
        call("dsgan_adam_amp", ptr(p), ptr(g), ptr(m), ptr(v), n, LR, B1, B2, EPS, ptr(state), cur())

    def fused(i):
        p, g, m, v, e = sets[i % NBUF]
        call("dsgan_adam_amp_ema", ptr(p), ptr(g), ptr(m), ptr(v), ptr(e), n, LR, B1, B2, EPS, DECAY, ptr(state), cur())

    def swap(i):
        p, _, _, _, e = sets[i % NBUF]
        call("dsgan_swap", ptr(p), ptr(e), n, cur())

    out = {"numel": n, "rounds": []}
    for r in range(rounds):
        row = {}
        for name, fn, bpe in (("adam", plain, 28), ("adam_ema", fused, 36), ("swap", swap, 16)):
            us = _graph_us(fn)
            row[name] = {"us": us, "TBps": bpe * n / us / 1e6}
        row["ratio"] = row["adam_ema"]["us"] / row["adam"]["us"]
        out["rounds"].append(row)
        print("round %d, %d elements: " % (r, n) + "  ".join(
            "%s %.1f us %.2f TB/s" % (k, v["us"], v["TBps"]) for k, v in row.items() if isinstance(v, dict))
            + "  adam_ema / adam = %.3f (bytes: %.3f)" % (row["ratio"], 36 / 28))
    return out


def step(rounds=2):
    from options.train_options import default_train_opt
    from models import create_model
    from oracle.recipe import synth_pair
    A, B = synth_pair(N, SIZE, seed=0)
    inp = {"A": A.cuda(), "B": B.cuda(), "A_paths": [""] * N, "B_paths": [""] * N}
    models = {}
    for decay in (0.0, DECAY):
        torch.manual_seed(20)
        m = create_model(default_train_opt(gpu_ids=[0], precision="bf16", batchSize=N, ema_decay=decay))
        for _ in range(5):   # eager warm-up, capture, replays
            m.set_input(inp)
            m.optimize_parameters()
        torch.cuda.synchronize()
        models[decay] = m
    out = {"ms_per_step": {str(d): [] for d in models}, "graph_step": {str(d): bool(m._graphs) for d, m in models.items()}}
    for _ in range(rounds):
        for decay, m in models.items():
            t0 = time.perf_counter()
            for _ in range(20):
                m.set_input(inp)
                m.optimize_parameters()
            torch.cuda.synchronize()
            out["ms_per_step"][str(decay)].append((time.perf_counter() - t0) / 20 * 1e3)
    m = models[DECAY]
    t = []
    for _ in range(5):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        with m.ema_scope():
            pass
        torch.cuda.synchronize()
        t.append((time.perf_counter() - t0) * 1e3)
    out["ema_scope_ms"] = sorted(t)[len(t) // 2]
    for d, ms in out["ms_per_step"].items():
        print("--ema_decay %-5s ms/step %s (graph step %s)" % (d, ["%.3f" % x for x in ms], out["graph_step"][d]))
    print("ema_scope() entry + exit: %.3f ms" % out["ema_scope_ms"])
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
