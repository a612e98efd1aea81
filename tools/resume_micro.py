"""Measurements of resumable training ("Resumable training"):

  kernel  dsgan_fingerprint over a buffer of the generator's flat size next to dsgan_amp_check on the same
          buffer (the existing read-only scan with the same access pattern, 4 B/element each), alternately in
          one process: device time per call from a captured graph of 8 calls over 4 rotating buffers
          (359 MB together, more than the 256 MB last-level cache, so every call reads from HBM), median of
          the replays, several rounds; the fingerprint also at a pointer offset by one word (its
          word-by-word form).
  run     seconds per save_train_state and per load_train_state of the default model (256^2, batch 16, bf16,
          --ema_decay 0.999, pool of 50 filled), the state file's size, and, for scale, the same for
          save_networks.

usage: python tools/resume_micro.py kernel|run [--out FILE.json]"""
import argparse
import json
import os
import sys
import tempfile
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [REPO, os.path.join(REPO, "ds-gan_amd")]

import torch  # noqa: E402

from tools.ema_micro import _graph_us, generator_numel  # noqa: E402

N, SIZE = 16, 256
NBUF = 4


def kernel(rounds=3):
    from dsgan_hip import _lib
    from dsgan_hip._lib import call, ptr, stream as cur
    n = generator_numel()
    bufs = [torch.randn(n + 4, device="cuda") * 1e-3 for _ in range(NBUF)]
    parts = int(_lib.load().dsgan_fingerprint_parts())
    fpart = torch.empty(parts + 1, device="cuda", dtype=torch.int64)
    apart = torch.empty(int(_lib.load().dsgan_amp_parts()), device="cuda", dtype=torch.int32)
    state = torch.tensor([1.0, 0.0, 0.0, 1.0, 0.0], device="cuda")

    def fp(i, off=0):
        call("dsgan_fingerprint", ptr(bufs[i % NBUF][off:]), n, ptr(fpart), parts, ptr(fpart[-1:]), cur())

    def amp(i):
        call("dsgan_amp_check", ptr(bufs[i % NBUF]), n, ptr(apart), ptr(state), 1.0, 1.0, 1 << 30, cur())

    out = {"numel": n, "rounds": []}
    for r in range(rounds):
        row = {}
        for name, fn in (("fingerprint", fp), ("amp_check", amp), ("fingerprint_unaligned", lambda i: fp(i, 1))):
            us = _graph_us(fn)
            row[name] = {"us": us, "TBps": 4 * n / us / 1e6}
        out["rounds"].append(row)
        print("round %d, %d elements (%.1f MB): " % (r, n, 4 * n / 1e6) + "  ".join(
            "%s %.1f us %.2f TB/s" % (k, v["us"], v["TBps"]) for k, v in row.items()))
    return out


def run(reps=3):
    from options.train_options import default_train_opt
    from models import create_model
    from oracle.recipe import synth_pair
    A, B = synth_pair(N, SIZE, seed=0)
    inp = {"A": A.cuda(), "B": B.cuda(), "A_paths": [""] * N, "B_paths": [""] * N}
    out = {"save_state_s": [], "load_state_s": [], "save_networks_s": []}
    with tempfile.TemporaryDirectory() as d:
        torch.manual_seed(20)
        m = create_model(default_train_opt(gpu_ids=[0], precision="bf16", batchSize=N, ema_decay=0.999, name="exp",
                                           checkpoints_dir=d))
        for _ in range(5):   # fills the pool of 50 (16 images a step), warms and captures the graph step
            m.set_input(inp)
            m.optimize_parameters()
        torch.cuda.synchronize()
        for _ in range(reps):
            t0 = time.perf_counter()
            m.save_networks("1")
            t1 = time.perf_counter()
            path = m.save_train_state("1")
            t2 = time.perf_counter()
            m.load_train_state("1")
            torch.cuda.synchronize()
            t3 = time.perf_counter()
            out["save_networks_s"].append(t1 - t0)
            out["save_state_s"].append(t2 - t1)
            out["load_state_s"].append(t3 - t2)
        out["state_file_bytes"] = os.path.getsize(path)
        out["network_files_bytes"] = sum(os.path.getsize(os.path.join(d, "exp", f)) for f in os.listdir(os.path.join(d, "exp"))
                                         if "_net_" in f)
        out["pool_images"] = m.fake_AB_pool.num_imgs
    for k in ("save_state_s", "load_state_s", "save_networks_s"):
        print("%-16s %s" % (k, ["%.3f" % x for x in out[k]]))
    print("state file %.1f MB (pool of %d images), network files %.1f MB"
          % (out["state_file_bytes"] / 1e6, out["pool_images"], out["network_files_bytes"] / 1e6))
    return out


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("what", choices=["kernel", "run"])
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import dsgan_hip
    dsgan_hip.require_gpu()
    res = {"kernel": kernel, "run": run}[a.what]()
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)
