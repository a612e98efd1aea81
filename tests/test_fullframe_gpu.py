"""evaluate.py --full_frame end to end on small PNG sets of mixed frame sizes.

The reference is the same generator in eval mode on ``to_images`` of host crops of every frame's tile
windows, in the chunks evaluate.py forms (at most --batchSize tiles of one frame), followed by the torch-CPU
fp32 reference blend of tests/tiling_fixture.py.  Panels are bit-exact against the CPU oracle's uint8
conversion of that; rows meet tests/test_evaluate_gpu.py's bars (1e-5, 1e-4, 2e-5) against the oracle
metrics on it."""
import csv
import os
import shutil

import numpy as np
import pytest
import torch

from oracle import dsgan_cpu as O
from tiling_fixture import blend_ref, crops

pytestmark = pytest.mark.gpu
SIZES = [(96, 80), (96, 80), (96, 80), (64, 64)]   # (H, W) of pair i
TILE, OVERLAP, BATCH = 64, 16, 2


def _write_pairs(d, sizes, seed):
    from PIL import Image
    rng = np.random.default_rng(seed)
    os.makedirs(d)
    for i, (h, w) in enumerate(sizes):
        for side in ("a", "b"):
            Image.fromarray(rng.integers(0, 256, (h, w, 3), dtype=np.uint8)).save(os.path.join(d, "%s_%d.png" % (side, i)))


def _read(d, name):
    from PIL import Image
    return np.array(Image.open(os.path.join(d, name + ".png")).convert("RGB"))


def _same(a, b):
    return np.array_equal(np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64), equal_nan=True)


def _size_args(size):
    return ["--loadSize_w", str(size), "--fineSize_w", str(size), "--loadSize_h", str(size), "--fineSize_h", str(size)]


def _reference_frame(netG, frame_u8, batch):
    """[3, H, W] on the CPU: netG on to_images of the host crops, chunked, then the CPU fp32 blend."""
    from data import to_images
    from dsgan_hip.tiling import TilePlan
    plan = TilePlan(frame_u8.shape[0], frame_u8.shape[1], TILE, TILE, OVERLAP)
    x = to_images(torch.from_numpy(crops(frame_u8, plan)), [0] * plan.T)
    with torch.no_grad():
        y = torch.cat([netG(x[t:t + batch]) for t in range(0, plan.T, batch)])
    return blend_ref(y.cpu(), plan)


@pytest.fixture(scope="module")
def run(tmp_path_factory):
    """Three 96x80 pairs and one 64x64 pair, a checkpoint of a fresh training model, one
    evaluate.main --full_frame run and the reference frames."""
    import evaluate as E
    from data import to_images
    from models import create_model
    from options.train_options import default_train_opt
    root = tmp_path_factory.mktemp("fullframe")
    data, out = str(root / "data"), str(root / "out")
    d = os.path.join(data, "test_all")
    _write_pairs(d, SIZES, 3)
    torch.manual_seed(7)
    m = create_model(default_train_opt(gpu_ids=[0], pool_size=0, precision="fp32", name="exp",
                                       checkpoints_dir=os.path.join(out, "checkpoints")))
    m.save_networks("3")
    args = ["--dataroot", data, "--out", out, "--name", "exp", "--which_epoch", "3", "--gpu_ids", "0",
            "--batchSize", str(BATCH), "--nThreads", "0"] + _size_args(TILE)
    rows, means = E.main(args + ["--full_frame", "--tile_overlap", str(OVERLAP)])
    m.netG.eval()
    A, B, fake = [], [], []
    for i in range(len(SIZES)):
        a, b = _read(d, "a_%d" % i), _read(d, "b_%d" % i)
        A.append(to_images(torch.from_numpy(a[None]), [0])[0].cpu())
        B.append(to_images(torch.from_numpy(b[None]), [0])[0].cpu())
        fake.append(_reference_frame(m.netG, a, BATCH))
    base = os.path.join(out, "epoch_8_result_original/", "exp")
    return {"args": args, "rows": rows, "means": means, "A": A, "B": B, "fake": fake, "base": base, "out": out,
            "data": data, "ckpt": os.path.join(out, "checkpoints", "exp")}


def test_full_frame_rows_vs_oracle(run):
    rows = run["rows"]
    assert len(rows) == len(SIZES)
    for n, row in enumerate(rows):
        B, fake = run["B"][n], run["fake"][n]
        lab, res = O.to_u8_hwc(B), O.to_u8_hwc(fake)
        s, p = O.sk_ssim(lab, res), float(O.cal_psnr(lab, res))
        g = float(O.ssim((B[None] + 1) / 2, (fake[None] + 1) / 2))
        print("frame %d %s: ssim %.8f vs %.8f, psnr %.6f vs %.6f, gauss %.7f vs %.7f"
              % (n, SIZES[n], row[0], s, row[1], p, row[2], g))
        assert abs(row[0] - s) < 1e-5 and abs(row[1] - p) < 1e-4 and abs(row[2] - g) < 2e-5
        assert np.isnan(row[3])   # below the MS-SSIM minimum side
    for c in range(3):
        assert abs(run["means"][c] - np.mean([r[c] for r in rows])) < 1e-6
    assert np.isnan(run["means"][3])


def test_full_frame_panels_csv_and_directory(run):
    dest = os.path.join(run["base"], "test_all_3_full")
    assert os.listdir(run["base"]) == ["test_all_3_full"]   # the plain directory is not touched
    assert sorted(os.listdir(dest)) == ["a_%d.png" % i for i in range(len(SIZES))] + ["metrics.csv"]
    for n, (h, w) in enumerate(SIZES):
        got = _read(dest, "a_%d" % n)
        ref = np.hstack([O.to_u8_hwc(run[k][n]) for k in ("A", "fake", "B")])
        assert got.shape == (h, 3 * w, 3)
        assert np.array_equal(got, ref), (n, int((got != ref).sum()))
    with open(os.path.join(dest, "metrics.csv"), newline="") as f:
        lines = list(csv.reader(f))
    assert lines[0] == ["image", "ssim", "psnr", "ssim_gauss", "ms_ssim"]
    assert [l[0] for l in lines[1:]] == ["a_%d" % i for i in range(len(SIZES))] + ["mean"]
    for l, row in zip(lines[1:1 + len(SIZES)], run["rows"]):
        assert l[4] == "" and abs(float(l[1]) - row[0]) < 1e-6 and abs(float(l[2]) - row[1]) < 1e-4
    assert abs(float(lines[-1][1]) - run["means"][0]) < 1e-6 and lines[-1][4] == ""


def test_full_frame_on_tile_sized_frames_equals_the_plain_pass(run, tmp_path):
    """64x64 frames, tile 64, --batchSize 1: one tile per frame, copied by the blend -- the plain rows."""
    import evaluate as E
    data = str(tmp_path / "data")
    _write_pairs(os.path.join(data, "test_all"), [(64, 64)] * 3, 5)
    args = [a for a in run["args"]]
    args[args.index("--dataroot") + 1] = data
    args[args.index("--batchSize") + 1] = "1"
    plain, _ = E.main(args + ["--results_dir", "tile64", "--no_images"])
    full, _ = E.main(args + ["--results_dir", "tile64", "--no_images", "--full_frame"])   # default overlap 32 = tile // 2
    assert len(plain) == 3 and _same(plain, full)
    assert sorted(os.listdir(os.path.join(run["out"], "tile64", "exp"))) == ["test_all_3", "test_all_3_full"]


def test_full_frame_how_many_and_refusals(run, tmp_path):
    import evaluate as E
    rows, _ = E.main(run["args"] + ["--full_frame", "--tile_overlap", str(OVERLAP), "--how_many", "2", "--no_images",
                                    "--results_dir", "two"])
    assert len(rows) == 2 and _same(rows, run["rows"][:2])
    assert os.listdir(os.path.join(run["out"], "two", "exp", "test_all_3_full")) == ["metrics.csv"]
    # a frame smaller than the tile is refused by file name
    data = str(tmp_path / "data")
    _write_pairs(os.path.join(data, "test_all"), [(64, 64), (64, 60)], 6)
    args = [a for a in run["args"]]
    args[args.index("--dataroot") + 1] = data
    with pytest.raises(ValueError, match=r"a_1\.png is 64x60"):
        E.main(args + ["--full_frame", "--results_dir", "small", "--no_images"])


def test_full_frame_single_dataset_writes_input_result_panels(run, tmp_path):
    """--model test --dataset_mode single: the A half of the listing, [input | result] panels, no CSV."""
    import evaluate as E
    d = tmp_path / "single"
    d.mkdir()
    for i in range(4):
        shutil.copy(os.path.join(run["data"], "test_all", "a_%d.png" % i), str(d / ("a_%d.png" % i)))
    rows, means = E.main(["--dataroot", str(d), "--out", run["out"], "--name", "exp", "--which_epoch", "3",
                          "--gpu_ids", "0", "--batchSize", str(BATCH), "--nThreads", "0", "--model", "test",
                          "--dataset_mode", "single", "--results_dir", "single", "--full_frame", "--tile_overlap",
                          str(OVERLAP)] + _size_args(TILE))
    assert rows == [] and means is None
    dest = os.path.join(run["out"], "single", "exp", "test_3_full")
    assert sorted(os.listdir(dest)) == ["a_0.png", "a_1.png"]
    for n in range(2):
        got = _read(dest, "a_%d" % n)
        ref = np.hstack([O.to_u8_hwc(run[k][n]) for k in ("A", "fake")])
        assert got.shape == (96, 160, 3) and np.array_equal(got, ref), n


def test_full_frame_use_ema_writes_beside(run):
    import evaluate as E
    sd = torch.load(os.path.join(run["ckpt"], "3_useSE_net_G.pth"), weights_only=True)
    g = torch.Generator().manual_seed(1)
    ema = {k: v + 0.01 * torch.randn(v.shape, generator=g).to(v) if v.is_floating_point() else v for k, v in sd.items()}
    torch.save(ema, os.path.join(run["ckpt"], "3_useSE_net_G_ema.pth"))
    try:
        rows, _ = E.main(run["args"] + ["--full_frame", "--tile_overlap", str(OVERLAP), "--use_ema", "--no_images",
                                        "--results_dir", "ema"])
    finally:
        os.remove(os.path.join(run["ckpt"], "3_useSE_net_G_ema.pth"))
    assert os.listdir(os.path.join(run["out"], "ema", "exp")) == ["test_all_3_full_ema"]
    assert len(rows) == len(SIZES) and not _same(rows, run["rows"])
    assert all(np.isfinite(r[:3]).all() for r in rows)
