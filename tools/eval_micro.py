"""Measurements of the evaluation path ("Evaluation"):

  metrics  dsgan_img_metrics_batch at (16, 3, 256, 256) against 16 calls of the per-image dsgan_img_metrics
           on the same images, in the same run: device us per call from a captured graph of 8 calls over 4
           rotating buffer sets, median of the replays.  The batched form must not be slower;
  stream   dsgan_images_to_u8 (three images in, one panel out) beside dsgan_u8_to_image on the same image
           count: us per call and bytes/s, bytes counted from shapes (fp32 in + uint8 out, and the reverse);
  run      images/s of evaluate.main at 256^2, batch 16, on a synthetic 64-pair test set, with and without
           --no_images (wall time of the pass: loader, generator, metrics, PNG encoding), and the device time
           of one batch's EvalMetrics.update beside the generator's eval forward.

usage: python tools/eval_micro.py metrics|stream|run [--out FILE.json]"""
import argparse
import json
import os
import sys
import tempfile
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [REPO, os.path.join(REPO, "ds-gan_amd")]

import torch  # noqa: E402

N, C, SIZE = 16, 3, 256
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


def _pairs():
    real = [torch.rand(N, C, SIZE, SIZE, device="cuda") * 2 - 1 for _ in range(NBUF)]
    fake = [(r + 0.2 * torch.randn_like(r)).clamp(-1, 1) for r in real]
    return fake, real


def metrics():
    from dsgan_hip import functional as HF
    from dsgan_hip._lib import call, ptr, stream as cur
    fake, real = _pairs()
    acc = torch.zeros(3, device="cuda")
    part = torch.empty(128, device="cuda", dtype=torch.float64)

    def per_image(i):
        f, r = fake[i % NBUF], real[i % NBUF]
        for n in range(N):
            call("dsgan_img_metrics", ptr(f[n]), ptr(r[n]), C, SIZE, SIZE, ptr(part), ptr(acc), cur())

    batched = _graph_us(lambda i: HF.img_metrics_batch(fake[i % NBUF], real[i % NBUF]))
    single = _graph_us(per_image)
    res = {"shape": [N, C, SIZE, SIZE], "batched_us": batched, "per_image_x%d_us" % N: single,
           "speedup": single / batched, "ok": batched <= single}
    print("img_metrics (%d, %d, %d, %d): batched %.1f us, %d per-image calls %.1f us (x%.1f) -> %s"
          % (N, C, SIZE, SIZE, batched, N, single, single / batched, "ok" if res["ok"] else "SLOWER"))
    return res


def stream():
    from dsgan_hip import functional as HF
    from dsgan_hip._lib import call, ptr, stream as cur
    fake, real = _pairs()
    px = N * SIZE * SIZE
    t_out = _graph_us(lambda i: HF.images_to_u8(real[i % NBUF], fake[i % NBUF], real[(i + 1) % NBUF]))
    b_out = 3 * px * (3 * 4 + 3)   # three fp32 RGB images read, their uint8 panel written
    u8 = [torch.randint(0, 256, (3 * N, SIZE, SIZE, 3), device="cuda", dtype=torch.uint8) for _ in range(NBUF)]
    flip = torch.zeros(3 * N, device="cuda", dtype=torch.int32)
    dst = [torch.empty(3 * N, 3, SIZE, SIZE, device="cuda") for _ in range(NBUF)]
    t_in = _graph_us(lambda i: call("dsgan_u8_to_image", ptr(u8[i % NBUF]), ptr(flip), ptr(dst[i % NBUF]), 3 * N, SIZE, SIZE,
                                    0, cur()))
    res = {"images": 3 * N, "size": SIZE, "bytes": b_out,
           "images_to_u8": {"us": t_out, "TBps": b_out / t_out / 1e6},
           "u8_to_image": {"us": t_in, "TBps": b_out / t_in / 1e6}}
    print("%d images of %d^2 (%.1f MB each way): images_to_u8 %.1f us %.2f TB/s, u8_to_image %.1f us %.2f TB/s"
          % (3 * N, SIZE, b_out / 1e6, t_out, b_out / t_out / 1e6, t_in, b_out / t_in / 1e6))
    return res


def run(images=64, precision="bf16"):
    import numpy as np
    from PIL import Image
    import evaluate as E
    from models import create_model
    from options.train_options import default_train_opt
    from util.metrics import EvalMetrics
    res = {"images": images, "size": SIZE, "batch": N, "precision": precision}
    with tempfile.TemporaryDirectory() as root:
        data, out = os.path.join(root, "data"), os.path.join(root, "out")
        os.makedirs(os.path.join(data, "test_all"))
        rng = np.random.default_rng(0)
        for i in range(images):
            for side in ("a", "b"):
                Image.fromarray(rng.integers(0, 256, (SIZE, SIZE, 3), dtype=np.uint8)).save(
                    os.path.join(data, "test_all", "%s_%03d.png" % (side, i)))
        torch.manual_seed(20)
        m = create_model(default_train_opt(gpu_ids=[0], isTrain=False, precision=precision, name="exp",
                                           checkpoints_dir=os.path.join(out, "checkpoints")))
        m.save_networks("1")
        args = ["--dataroot", data, "--out", out, "--name", "exp", "--which_epoch", "1", "--gpu_ids", "0",
                "--batchSize", str(N), "--precision", precision]
        spent = []
        inner = E.run_pass

        def timed_pass(*a, **k):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            n = inner(*a, **k)
            torch.cuda.synchronize()
            spent.append(time.perf_counter() - t0)
            return n
        E.run_pass = timed_pass
        try:
            for tag, extra in (("warm", ["--no_images"]), ("no_images", ["--no_images"]), ("with_images", [])):
                E.main(args + ["--results_dir", tag] + extra)
                res[tag] = {"pass_s": spent[-1], "images_per_s": images / spent[-1]}
        finally:
            E.run_pass = inner
        del res["warm"]
        # device time of one batch: the generator's eval forward beside EvalMetrics.update
        fake, real = _pairs()
        m.netG.eval()
        em = EvalMetrics(m.device, N)

        def upd(i):
            em.reset()
            em.update(fake[i % NBUF], real[i % NBUF])
        t_metrics = _graph_us(upd)
        with torch.no_grad():
            for _ in range(3):
                m.netG(real[0])
            ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(10)]
            for e0, e1 in ev:
                e0.record()
                m.netG(real[0])
                e1.record()
            torch.cuda.synchronize()
        t_fwd = sorted(e0.elapsed_time(e1) * 1e3 for e0, e1 in ev)[5]
        res["device_us_per_batch"] = {"generator_forward": t_fwd, "eval_metrics_update": t_metrics,
                                      "metrics_share": t_metrics / (t_metrics + t_fwd)}
    print("evaluate.main, %d images of %d^2, batch %d, %s: %.1f images/s without PNGs, %.1f with"
          % (images, SIZE, N, precision, res["no_images"]["images_per_s"], res["with_images"]["images_per_s"]))
    print("one batch on the device: generator forward %.0f us (eager launches), EvalMetrics.update %.0f us (%.1f %%)"
          % (t_fwd, t_metrics, 100 * res["device_us_per_batch"]["metrics_share"]))
    return res


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("what", choices=["metrics", "stream", "run"])
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import dsgan_hip
    dsgan_hip.require_gpu()
    res = {"metrics": metrics, "stream": stream, "run": run}[a.what]()
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)
