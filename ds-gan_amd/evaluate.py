"""Test-set evaluation: load a checkpoint's generator, colourise a test split, write the panels and
report PSNR / SSIM per image (the per-epoch test pass DSGAN/train.py:58, 64-68, 80 prepares).

    python ds-gan_amd/evaluate.py --dataroot DATA --out RESULTS --name NAME --which_epoch 8 [TestOptions flags]

With the defaults (--model pix2pix, --dataset_mode aligned, --phase test_all/) every image pair of
DATA/test_all/ goes through the generator in eval mode under ``torch.no_grad()`` (dropout off, a
BatchNorm generator on its running buffers); each batch is scored on the device
(util.metrics.EvalMetrics: skimage-style SSIM, PSNR, gaussian SSIM, MS-SSIM) and written as one lossless
PNG panel ``[input | result | label]`` per image, named after the input file's stem
(dsgan_images_to_u8: the panels cross PCIe as uint8).  ``metrics.csv`` gets a header, one row per
image and a last ``mean`` row.  Everything lands in ``<results_dir>/<name>/<phase>_<which_epoch>/``; a
relative --results_dir is taken under --out.  ``--how_many`` images are evaluated, exactly.

``--model test --dataset_mode single`` has no labels: ``[input | result]`` panels and no CSV.
``--no_images`` skips the PNGs.  ``--use_ema`` scores the averaged generator a run with ``--ema_decay``
saved: it loads ``<which_epoch>_net_G_ema.pth`` (or ``<which_epoch>_useSE_net_G_ema.pth``) instead of the
raw generator's file and writes to ``<phase>_<which_epoch>_ema/``, beside the raw results; without such a
file it fails, naming the paths it tried.  Evaluation is single-process (WORLD_SIZE > 1 is refused), batches are
taken in order and never flipped, and ``--aspect_ratio`` other than 1.0 (the reference visualiser's
resize) is refused.  The seed is 20, as in train.py.

``--full_frame [--tile_overlap P]`` colourises whole frames instead of one fineSize crop per file: each file
is read as it is (data/frame_dataset.py: no crop, any size not smaller than the tile), cut on the device into
overlapping ``fineSize_h x fineSize_w`` tiles (dsgan_hip/tiling.py; P pixels of overlap, 32 by default, at most
half a tile), the tiles go through the generator in chunks of at most ``--batchSize`` tiles of that frame, and
the outputs are blended back under a linear ramp over the overlap (dsgan_tiles_blend).  Rows, panels and the
CSV are then per frame, at the frame's size, in ``<phase>_<which_epoch>_full/`` (``..._full_ema/`` with
``--use_ema``), beside the plain results.  Every tile is normalised by its own InstanceNorm statistics, as
every training crop was; the ramp hides the difference.
"""
import argparse
import copy
import csv
import math
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)

import torch  # noqa: E402


def results_dir(opt, out, use_ema=False, full_frame=False):
    """<results_dir>/<name>/<phase>_<which_epoch>, with ``_full`` appended for whole frames and ``_ema`` for
    the averaged generator; a relative --results_dir is taken under ``out``."""
    root = opt.results_dir if os.path.isabs(opt.results_dir) else os.path.join(out, opt.results_dir)
    leaf = "%s_%s" % (opt.phase.strip("/\\").replace("/", "_"), opt.which_epoch)
    return os.path.join(root, opt.name, leaf + ("_full" if full_frame else "") + ("_ema" if use_ema else ""))


def ema_checkpoint(save_dir, which_epoch):
    """The averaged generator's checkpoint for ``which_epoch`` in ``save_dir`` (either name form)."""
    paths = [os.path.join(save_dir, n % which_epoch) for n in ("%s_net_G_ema.pth", "%s_useSE_net_G_ema.pth")]
    for p in paths:
        if os.path.exists(p):
            return p
    raise FileNotFoundError("--use_ema: no EMA generator checkpoint (train with --ema_decay): tried %s"
                            % " and ".join(paths))


def check_options(opt, tile_overlap=None):
    """Refuse what evaluate.py does not do; ``tile_overlap`` is --tile_overlap of a --full_frame run."""
    if tile_overlap is not None:
        from dsgan_hip.tiling import check_overlap
        check_overlap(tile_overlap, opt.fineSize_h, opt.fineSize_w)
        if getattr(opt, "load_resize", "none") != "none":
            raise ValueError("--full_frame tiles the frame as decoded: --load_resize %s (a resize to loadSize %dx%d "
                             "before a fineSize crop) does not apply to it; use --load_resize none"
                             % (opt.load_resize, opt.loadSize_h, opt.loadSize_w))
    if float(opt.aspect_ratio) != 1.0:
        raise ValueError("evaluate.py writes the generator's pixels: --aspect_ratio %s (the reference visualiser's "
                         "resize) is not supported, only 1.0" % opt.aspect_ratio)
    if int(opt.how_many) < 1:
        raise ValueError("--how_many must be at least 1")


def eval_options(opt, phase=None):
    """A copy of ``opt`` with the loader settings every evaluation pass forces: batches in order, no
    flip, and ``phase`` when given."""
    o = copy.copy(opt)
    o.serial_batches, o.no_flip = True, True
    if phase is not None:
        o.phase = phase
    return o


def _cell(v):
    return "" if isinstance(v, float) and math.isnan(v) else "%.7g" % v


def write_metrics_csv(path, columns, names, rows, means):
    """Header, one row per image, a last ``mean`` row; NaN is written as an empty cell."""
    with open(path, "w", newline="") as f:
        w = csv.writer(f)
        w.writerow(["image"] + list(columns))
        for name, row in zip(names, rows):
            w.writerow([name] + [_cell(float(v)) for v in row])
        w.writerow(["mean"] + [_cell(float(v)) for v in means])


def run_pass(netG, dataset, AtoB=True, how_many=None, metrics=None, on_batch=None):
    """The generator in eval mode over ``dataset`` under no_grad, at most ``how_many`` images (the last
    batch is truncated).  ``metrics.update(fake, real)`` scores each labelled batch;
    ``on_batch(real_A, fake_B, real_B or None, input paths)`` sees each batch.  Every module's
    ``training`` flag is restored.  Returns the number of images."""
    flags = [(m, m.training) for m in netG.modules()]
    netG.eval()
    done = 0
    try:
        with torch.no_grad():
            for data in dataset:
                labelled = "B" in data
                A = data["A" if AtoB or not labelled else "B"]
                B = data["B" if AtoB else "A"] if labelled else None
                paths = data["A_paths" if AtoB or not labelled else "B_paths"]
                k = A.shape[0] if how_many is None else min(A.shape[0], how_many - done)
                if k < A.shape[0]:
                    A, paths = A[:k], paths[:k]
                    B = B[:k] if labelled else None
                fake = netG(A)
                if metrics is not None and labelled:
                    metrics.update(fake, B)
                if on_batch is not None:
                    on_batch(A, fake, B, paths)
                done += k
                if how_many is not None and done >= how_many:
                    break
    finally:
        for m, t in flags:
            m.training = t
    return done


def run_full_frame_pass(netG, frames, tile, overlap, batch, gray_in=False, gray_label=False, AtoB=True, how_many=None,
                        metrics=None, on_batch=None):
    """``run_pass`` on whole frames: ``frames`` yields FrameDataset items (uint8 frames of any size not smaller
    than ``tile`` = (th, tw)); each goes through ``tiling.colorize_frame`` -- its own tiles only, in chunks of
    at most ``batch`` -- and is scored and shown at its full size, one ``metrics.update`` per frame."""
    from data import to_images
    from dsgan_hip import tiling
    flags = [(m, m.training) for m in netG.modules()]
    netG.eval()
    plans = {}
    done = 0
    try:
        with torch.no_grad():
            for data in frames:
                labelled = "B_u8" in data
                src = "A" if AtoB or not labelled else "B"
                u8 = data[src + "_u8"].to("cuda", non_blocking=True)
                H, W = int(u8.shape[0]), int(u8.shape[1])
                if (H, W) not in plans:
                    plans[(H, W)] = tiling.TilePlan(H, W, tile[0], tile[1], overlap)
                fake = tiling.colorize_frame(netG, u8, plans[(H, W)], batch, gray_in).unsqueeze(0)
                A = to_images(u8.unsqueeze(0), [0], gray_in)
                B = to_images(data[("B" if AtoB else "A") + "_u8"].unsqueeze(0), [0], gray_label) if labelled else None
                if metrics is not None and labelled:
                    metrics.update(fake, B)
                if on_batch is not None:
                    on_batch(A, fake, B, [data[src + "_paths"]])
                done += 1
                if how_many is not None and done >= how_many:
                    break
    finally:
        for m, t in flags:
            m.training = t
    return done


def main(argv=None):
    from data import CreateDataLoader
    from dsgan_hip import functional as HF
    from models import create_model
    from options.test_options import TestOptions
    from train import setup_seed
    from util.metrics import EvalMetrics

    if int(os.environ.get("WORLD_SIZE", "1")) > 1:
        raise RuntimeError("evaluate.py is single-process: WORLD_SIZE=%s (run it without torchrun)"
                           % os.environ["WORLD_SIZE"])
    ap = argparse.ArgumentParser(add_help=False)
    ap.add_argument("--out", default=os.path.abspath(os.path.join("..", "resext50_vision1")))
    ap.add_argument("--dataroot", default="/root/dataset/256x256")
    ap.add_argument("--no_images", action="store_true", help="score only: write no PNG panels")
    ap.add_argument("--use_ema", action="store_true",
                    help="score the averaged generator (<which_epoch>_net_G_ema.pth) into <phase>_<which_epoch>_ema/")
    ap.add_argument("--full_frame", action="store_true",
                    help="colourise whole frames by overlapping fineSize tiles into <phase>_<which_epoch>_full/")
    ap.add_argument("--tile_overlap", type=int, default=32, help="--full_frame: pixels two neighbouring tiles share")
    known, rest = ap.parse_known_args(argv)
    overlap = known.tile_overlap if known.full_frame else None
    if known.full_frame:   # before anything is written (parse() below creates the checkpoint directory)
        check_options(TestOptions().gather_options(rest), overlap)
    setup_seed(20)
    opt = TestOptions().parse(known.dataroot, known.out, rest)
    check_options(opt, overlap)
    opt = eval_options(opt)
    if known.use_ema:   # before anything is written
        ema_checkpoint(os.path.join(opt.checkpoints_dir, opt.name), opt.which_epoch)
    dest = results_dir(opt, known.out, known.use_ema, known.full_frame)
    os.makedirs(dest, exist_ok=True)
    if known.full_frame:
        from data.frame_dataset import frame_loader
        dataset = frame_loader(opt)
    else:
        dataset = CreateDataLoader(opt, "test", local=True).load_data()
    how_many = min(int(opt.how_many), len(dataset))
    print("#test images = %d" % how_many)
    model = create_model(opt)
    if known.use_ema:   # load_networks then reads the _ema files (same name forms, same key handling)
        model.load_suffix = "_ema"
    model.setup(opt)
    model.eval()
    metrics = EvalMetrics(model.device, max(how_many, 1))
    names = []

    def on_batch(A, fake, B, paths):
        names.extend(os.path.splitext(os.path.basename(p))[0] for p in paths)
        if known.no_images:
            return
        from PIL import Image
        panels = HF.images_to_u8(*([A, fake] if B is None else [A, fake, B])).cpu().numpy()
        for p, arr in zip(names[-len(paths):], panels):
            # (zlib level 1: the encoder on the host, not the device, bounds a run that writes panels)
            Image.fromarray(arr).save(os.path.join(dest, p + ".png"), compress_level=1)

    if known.full_frame:
        n = run_full_frame_pass(model.netG, dataset, (opt.fineSize_h, opt.fineSize_w), overlap, opt.batchSize,
                                opt.input_nc == 1, opt.output_nc == 1, opt.which_direction == "AtoB", how_many, metrics,
                                on_batch)
    else:
        n = run_pass(model.netG, dataset, opt.which_direction == "AtoB", how_many, metrics, on_batch)
    if metrics.n == 0:   # --dataset_mode single: no labels, nothing to score
        print("%d panels -> %s" % (n, dest))
        return [], None
    rows, means = metrics.rows(), metrics.means()
    write_metrics_csv(os.path.join(dest, "metrics.csv"), EvalMetrics.COLUMNS, names, rows, means)
    print("%d images: " % n + " ".join("%s %s" % (c, _cell(v) or "n/a") for c, v in zip(EvalMetrics.COLUMNS, means))
          + " -> %s" % dest)
    return rows, means


if __name__ == "__main__":
    main()
