"""Measurements of whole-frame colourisation ("Whole-frame colourisation"):

  kernel   dsgan_u8_tiles and dsgan_tiles_blend on one 512x640 frame, 256^2 tiles, overlap 32 (9 tiles): device
           us per call from a captured graph of 8 calls over 4 rotating buffer sets, median of the replays, and
           bytes/s with the bytes counted from shapes; beside them dsgan_images_to_u8 on the same frame (the
           streaming yardstick) and a torch-op composition of the same blend on the device (per tile a weighted
           slice-add into the numerator and the denominator, then one divide) -- the baseline the kernel
           replaces, which it must not be slower than;
  run      frames/s of the full-frame pass (tiling.colorize_frame on an uploaded frame, batch 9) and the share of
           a frame's device time that the two tile kernels take, against the generator's time on the same 9 tiles.

usage: python tools/tile_micro.py kernel|run [--out FILE.json] [--precision fp32|bf16]"""
import argparse
import json
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [REPO, os.path.join(REPO, "ds-gan_amd"), os.path.join(REPO, "tools")]

import torch  # noqa: E402

from eval_micro import NBUF, _graph_us  # noqa: E402  (the same timing helper)

H, W, TILE, OVERLAP, C = 512, 640, 256, 32, 3


def _plan():
    from dsgan_hip.tiling import TilePlan
    return TilePlan(H, W, TILE, TILE, OVERLAP)


def _torch_blend(tiles, plan, w2, num, den):
    """The blend as torch ops on the device: weighted slice-adds, then a divide (no single-cover copy)."""
    num.zero_()
    den.zero_()
    for t in range(plan.T):
        y0, x0 = plan.corner(t)
        num[:, y0:y0 + plan.th, x0:x0 + plan.tw].addcmul_(tiles[t], w2)
        den[y0:y0 + plan.th, x0:x0 + plan.tw].add_(w2)
    return num / den


def kernel():
    from dsgan_hip import functional as HF
    from dsgan_hip import tiling
    plan = _plan()
    assert plan.T == 9
    frames = [torch.randint(0, 256, (H, W, 3), device="cuda", dtype=torch.uint8) for _ in range(NBUF)]
    tiles = [torch.rand(plan.T, C, TILE, TILE, device="cuda") * 2 - 1 for _ in range(NBUF)]
    full = [torch.rand(1, C, H, W, device="cuda") * 2 - 1 for _ in range(NBUF)]
    t_cut = _graph_us(lambda i: tiling.frame_tiles(frames[i % NBUF], plan))
    t_blend = _graph_us(lambda i: tiling.blend(tiles[i % NBUF], plan))
    t_u8 = _graph_us(lambda i: HF.images_to_u8(full[i % NBUF]))
    wy = torch.tensor(tiling.w1(TILE, OVERLAP), device="cuda", dtype=torch.float32)
    w2 = wy[:, None] * wy[None, :]
    num, den = torch.empty(C, H, W, device="cuda"), torch.empty(H, W, device="cuda")
    t_torch = _graph_us(lambda i: _torch_blend(tiles[i % NBUF], plan, w2, num, den))
    # the composition computes the blend too (it lacks only the single-cover copy: equal to rounding)
    err = float((_torch_blend(tiles[0], plan, w2, num, den) - tiling.blend(tiles[0], plan)).abs().max())
    b_cut = H * W * 3 + plan.T * C * TILE * TILE * 4          # the frame read once, the tiles written
    b_blend = plan.T * C * TILE * TILE * 4 + C * H * W * 4    # every tile read once, the frame written
    b_u8 = C * H * W * 4 + H * W * 3
    res = {"frame": [H, W], "tile": TILE, "overlap": OVERLAP, "tiles": plan.T,
           "u8_tiles": {"us": t_cut, "bytes": b_cut, "TBps": b_cut / t_cut / 1e6},
           "tiles_blend": {"us": t_blend, "bytes": b_blend, "TBps": b_blend / t_blend / 1e6},
           "images_to_u8": {"us": t_u8, "bytes": b_u8, "TBps": b_u8 / t_u8 / 1e6},
           "torch_blend": {"us": t_torch, "launches": 2 + 2 * plan.T + 1, "max_abs_diff": err},
           "speedup": t_torch / t_blend, "ok": t_blend <= t_torch}
    print("%dx%d frame, %d tiles of %d^2, overlap %d:" % (H, W, plan.T, TILE, OVERLAP))
    for k in ("u8_tiles", "tiles_blend", "images_to_u8"):
        print("  %-13s %7.1f us  %6.2f MB  %.2f TB/s" % (k, res[k]["us"], res[k]["bytes"] / 1e6, res[k]["TBps"]))
    print("  torch-op blend %6.1f us (%d launches, max |diff| %.2g) -> kernel x%.1f: %s"
          % (t_torch, res["torch_blend"]["launches"], err, res["speedup"], "ok" if res["ok"] else "SLOWER"))
    return res


def _event_us(fn, warm=3, iters=10):
    for _ in range(warm):
        fn()
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(iters)]
    for e0, e1 in ev:
        e0.record()
        fn()
        e1.record()
    torch.cuda.synchronize()
    return sorted(e0.elapsed_time(e1) * 1e3 for e0, e1 in ev)[iters // 2]


def run(precision="bf16"):
    import time
    from dsgan_hip import tiling
    from models import create_model
    from options.train_options import default_train_opt
    plan = _plan()
    torch.manual_seed(20)
    m = create_model(default_train_opt(gpu_ids=[0], isTrain=False, precision=precision, name="exp"))
    m.netG.eval()
    frame = torch.randint(0, 256, (H, W, 3), device="cuda", dtype=torch.uint8)
    with torch.no_grad():
        x = tiling.frame_tiles(frame, plan)
        y = m.netG(x).float()
        t_cut = _event_us(lambda: tiling.frame_tiles(frame, plan))
        t_gen = _event_us(lambda: m.netG(x))
        t_blend = _event_us(lambda: tiling.blend(y, plan))
        t_frame = _event_us(lambda: tiling.colorize_frame(m.netG, frame, plan, plan.T))
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        n = 20
        for _ in range(n):
            tiling.colorize_frame(m.netG, frame, plan, plan.T)
        torch.cuda.synchronize()
        wall = (time.perf_counter() - t0) / n
    res = {"frame": [H, W], "tiles": plan.T, "precision": precision, "frames_per_s": 1.0 / wall,
           "device_us": {"u8_tiles": t_cut, "generator_9_tiles": t_gen, "tiles_blend": t_blend, "colorize_frame": t_frame},
           "tile_kernels_share": (t_cut + t_blend) / (t_cut + t_blend + t_gen)}
    print("colorize_frame, %dx%d, %d tiles of %d^2 in one chunk, %s: %.1f frames/s (eager launches)"
          % (H, W, plan.T, TILE, precision, res["frames_per_s"]))
    print("one frame on the device: u8_tiles %.1f us + tiles_blend %.1f us beside the generator's %.0f us on the same "
          "tiles: %.2f %% of the frame" % (t_cut, t_blend, t_gen, 100 * res["tile_kernels_share"]))
    return res


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("what", choices=["kernel", "run"])
    ap.add_argument("--out", default=None)
    ap.add_argument("--precision", default="bf16", choices=["fp32", "bf16"])
    a = ap.parse_args()
    import dsgan_hip
    dsgan_hip.require_gpu()
    res = kernel() if a.what == "kernel" else run(a.precision)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)
