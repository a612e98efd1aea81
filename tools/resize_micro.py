"""Measurements of the load-time resize ("Load-time resize"):

  kernel   dsgan_u8_resize_crop_to_image on 16 frames of 512x640 -> load 286x286 -> crop 256x256 (bicubic and
           bilinear): device us per call from a captured graph of 8 calls over 4 rotating buffer sets, median of
           the replays, and source bytes/s (the uint8 frames, counted from shapes); beside it dsgan_u8_to_image
           on crops of the same size (what the loader runs without the flag) and PIL's Image.resize of one such
           frame on one host core, per image -- the host work the device call replaces;
  loader   images/s of the training loader (CreateDataLoader, aligned pairs, batch 16, --nThreads workers) over a
           synthetic set of 512x640 PNG pairs with --load_resize bicubic, against the same loader with the flag
           off over a dataset whose workers do the PIL resize before the crop.

usage: python tools/resize_micro.py kernel|loader [--out FILE.json] [--nThreads N] [--pairs N]"""
import argparse
import json
import os
import random
import sys
import tempfile
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [REPO, os.path.join(REPO, "ds-gan_amd"), os.path.join(REPO, "tools")]

import numpy as np  # noqa: E402
import torch  # noqa: E402
from PIL import Image  # noqa: E402

from eval_micro import NBUF, _graph_us  # noqa: E402  (the same timing helper)

N, HS, WS, LOAD, FINE = 16, 512, 640, 286, 256
PIL_FILTER = {"bicubic": Image.BICUBIC, "bilinear": Image.BILINEAR}


def _pil_us(frame, filt, iters=30):
    img = Image.fromarray(frame)
    img.resize((LOAD, LOAD), PIL_FILTER[filt])
    t = []
    for _ in range(iters):
        t0 = time.perf_counter()
        img.resize((LOAD, LOAD), PIL_FILTER[filt])
        t.append((time.perf_counter() - t0) * 1e6)
    return sorted(t)[iters // 2]


def kernel():
    from dsgan_hip import resample
    from dsgan_hip._lib import call, ptr, stream as cur
    dev = torch.device("cuda", torch.cuda.current_device())
    frames = [torch.randint(0, 256, (N, HS, WS, 3), device=dev, dtype=torch.uint8) for _ in range(NBUF)]
    crops = [torch.randint(0, 256, (N, FINE, FINE, 3), device=dev, dtype=torch.uint8) for _ in range(NBUF)]
    dst = [torch.empty(N, 3, FINE, FINE, device=dev) for _ in range(NBUF)]
    rng = random.Random(0)
    off = torch.tensor([(rng.randint(0, LOAD - FINE), rng.randint(0, LOAD - FINE)) for _ in range(N)],
                       dtype=torch.int32, device=dev)
    flip = torch.tensor([rng.randint(0, 1) for _ in range(N)], dtype=torch.int32, device=dev)
    src_bytes = N * HS * WS * 3
    res = {"frames": [N, HS, WS], "load": LOAD, "fine": FINE, "source_bytes": src_bytes}
    for filt in ("bicubic", "bilinear"):
        yb, yc, ky = resample.device_tables(HS, LOAD, filt, dev)
        xb, xc, kx = resample.device_tables(WS, LOAD, filt, dev)
        need = resample.tmp_bytes(N, HS, FINE, kx)
        tmp = [torch.empty(need, device=dev, dtype=torch.uint8) for _ in range(NBUF)]

        def one(i):
            call("dsgan_u8_resize_crop_to_image", ptr(frames[i % NBUF]), N, HS, WS, ptr(yb), ptr(yc), ky, ptr(xb), ptr(xc),
                 kx, LOAD, LOAD, ptr(off), ptr(flip), FINE, FINE, 0, ptr(tmp[i % NBUF]), need, ptr(dst[i % NBUF]), cur())

        t = _graph_us(one)
        pil = _pil_us(frames[0][0].cpu().numpy(), filt)
        res[filt] = {"us": t, "us_per_image": t / N, "source_GBps": src_bytes / t / 1e3, "taps": [ky, kx],
                     "pil_us_per_image": pil, "pil_over_device": pil / (t / N), "ok": t / N < pil}
    t_u8 = _graph_us(lambda i: call("dsgan_u8_to_image", ptr(crops[i % NBUF]), ptr(flip), ptr(dst[i % NBUF]), N, FINE,
                                    FINE, 0, cur()))
    res["u8_to_image"] = {"us": t_u8, "us_per_image": t_u8 / N, "source_GBps": N * FINE * FINE * 3 / t_u8 / 1e3}
    print("%d frames of %dx%d -> %d^2 -> crop %d^2 (%.1f MB of uint8 frames):" % (N, HS, WS, LOAD, FINE, src_bytes / 1e6))
    for filt in ("bicubic", "bilinear"):
        r = res[filt]
        print("  resize_crop_to_image %-8s %7.1f us  %6.2f us/image  %7.1f GB/s of source | PIL resize on one core "
              "%8.1f us/image (x%.0f): %s" % (filt, r["us"], r["us_per_image"], r["source_GBps"], r["pil_us_per_image"],
                                              r["pil_over_device"], "ok" if r["ok"] else "SLOWER"))
    print("  u8_to_image on %d^2 crops      %7.1f us  %6.2f us/image" % (FINE, t_u8, t_u8 / N))
    return res


def _write_set(root, pairs):
    rng = np.random.default_rng(0)
    d = os.path.join(root, "train_all")
    os.makedirs(d)
    # smooth ramps plus noise: PNG decode time nearer a camera frame's than pure noise would give
    yy, xx = np.mgrid[0:HS, 0:WS]
    for i in range(pairs):
        for side in ("a", "b"):
            base = ((yy * (i + 1) + xx * 2) % 256)[..., None] + rng.integers(0, 16, (HS, WS, 3))
            Image.fromarray(np.clip(base, 0, 255).astype(np.uint8)).save(os.path.join(d, "%s_%04d.png" % (side, i)),
                                                                         compress_level=1)


def _host_resize_dataset(opt):
    """AlignedDataset whose workers resize with PIL before the crop: the loader the flag replaces."""
    from data.aligned_dataset import AlignedDataset

    class HostResize(AlignedDataset):
        def _crop(self, path, h_off, w_off):
            img = Image.open(path).convert("RGB").resize((self.opt.loadSize_w, self.opt.loadSize_h), Image.BICUBIC)
            fh, fw = self.opt.fineSize_h, self.opt.fineSize_w
            return np.asarray(img, dtype=np.uint8)[h_off:h_off + fh, w_off:w_off + fw].copy()

    ds = HostResize()
    ds.initialize(opt)
    return ds


def _images_per_s(loader, epochs=2):
    n = 0
    for data in loader:   # the first epoch starts the workers and warms the page cache
        pass
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(epochs):
        for data in loader:
            n += data["A"].shape[0]
    torch.cuda.synchronize()
    return n / (time.perf_counter() - t0)


def loader(n_threads, pairs):
    from data import CreateDataLoader
    from options.train_options import default_train_opt
    res = {"frames": [HS, WS], "load": LOAD, "fine": FINE, "batch": N, "nThreads": n_threads, "pairs": pairs}
    with tempfile.TemporaryDirectory() as root:
        _write_set(root, pairs)
        kw = dict(gpu_ids=[0], dataroot=root, phase="train_all", loadSize_w=LOAD, loadSize_h=LOAD, fineSize_w=FINE,
                  fineSize_h=FINE, batchSize=N, nThreads=n_threads)
        on = CreateDataLoader(default_train_opt(load_resize="bicubic", **kw), "train").load_data()
        res["device_resize_images_per_s"] = _images_per_s(on)
        host = CreateDataLoader(default_train_opt(load_resize="none", **kw), "train")
        host.dataset = _host_resize_dataset(host.opt)
        host.dataloader = torch.utils.data.DataLoader(host.dataset, batch_size=N, shuffle=True, num_workers=n_threads,
                                                      pin_memory=True)
        res["host_resize_images_per_s"] = _images_per_s(host.load_data())
    res["speedup"] = res["device_resize_images_per_s"] / res["host_resize_images_per_s"]
    print("training loader, %d pairs of %dx%d PNG -> %d^2 -> %d^2, batch %d, %d workers: --load_resize bicubic %.0f "
          "images/s, PIL resize in the workers %.0f images/s (x%.2f)"
          % (pairs, HS, WS, LOAD, FINE, N, n_threads, res["device_resize_images_per_s"],
             res["host_resize_images_per_s"], res["speedup"]))
    return res


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("what", choices=["kernel", "loader"])
    ap.add_argument("--out", default=None)
    ap.add_argument("--nThreads", type=int, default=4, help="loader: worker processes of each loader")
    ap.add_argument("--pairs", type=int, default=64, help="loader: PNG pairs of the synthetic set")
    a = ap.parse_args()
    import dsgan_hip
    dsgan_hip.require_gpu()
    res = kernel() if a.what == "kernel" else loader(a.nThreads, a.pairs)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)
