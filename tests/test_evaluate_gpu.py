"""evaluate.py end to end on small PNG test sets, and train.py's opt-in per-epoch test pass.

The references are the CPU oracle's uint8 conversion / skimage-style SSIM / PSNR / gaussian SSIM applied
to the same generator's eval-mode outputs, batched as evaluate.py batches them; bars as in
tests/test_evalimg_gpu.py (1e-5, 1e-4, 2e-5), panels bit-exact."""
import csv
import os

import numpy as np
import pytest
import torch

from oracle import dsgan_cpu as O

pytestmark = pytest.mark.gpu
DEV = "cuda"


def _write_pairs(d, n, size, seed):
    from PIL import Image
    rng = np.random.default_rng(seed)
    os.makedirs(d)
    for i in range(n):
        for side in ("a", "b"):
            Image.fromarray(rng.integers(0, 256, (size, size, 3), dtype=np.uint8)).save(os.path.join(d, "%s_%d.png" % (side, i)))


def _load(d, side, n):
    from PIL import Image
    from data import to_images
    u8 = np.stack([np.asarray(Image.open(os.path.join(d, "%s_%d.png" % (side, i))).convert("RGB")) for i in range(n)])
    return to_images(torch.from_numpy(u8), [0] * n)


def _same(a, b):
    """Row lists equal bit for bit (NaN cells included)."""
    return np.array_equal(np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64), equal_nan=True)


def _size_args(size):
    return ["--loadSize_w", str(size), "--fineSize_w", str(size), "--loadSize_h", str(size), "--fineSize_h", str(size)]


@pytest.fixture(scope="module")
def run64(tmp_path_factory):
    """Five 64x64 pairs, a checkpoint of a training model, one evaluate.main run (batch 2: a ragged last
    batch) and the same generator's eval-mode outputs on the same batches."""
    import evaluate as E
    from models import create_model
    from options.train_options import default_train_opt
    root = tmp_path_factory.mktemp("eval64")
    data, out = str(root / "data"), str(root / "out")
    _write_pairs(os.path.join(data, "test_all"), 5, 64, 3)
    torch.manual_seed(7)
    m = create_model(default_train_opt(gpu_ids=[0], pool_size=0, precision="fp32", name="exp",
                                       checkpoints_dir=os.path.join(out, "checkpoints")))
    m.save_networks("3")
    args = ["--dataroot", data, "--out", out, "--name", "exp", "--which_epoch", "3", "--gpu_ids", "0",
            "--batchSize", "2", "--nThreads", "0"] + _size_args(64)
    rows, means = E.main(args)
    A, B = _load(os.path.join(data, "test_all"), "a", 5), _load(os.path.join(data, "test_all"), "b", 5)
    m.netG.eval()
    with torch.no_grad():
        fake = torch.cat([m.netG(A[i:i + 2]) for i in (0, 2, 4)])
    dest = os.path.join(out, "epoch_8_result_original/", "exp", "test_all_3")
    return {"args": args, "rows": rows, "means": means, "A": A.cpu(), "B": B.cpu(), "fake": fake.cpu(), "dest": dest,
            "out": out}


def test_evaluate_rows_vs_oracle(run64):
    rows, fake, B = run64["rows"], run64["fake"], run64["B"]
    assert len(rows) == 5
    for n, row in enumerate(rows):
        lab, res = O.to_u8_hwc(B[n]), O.to_u8_hwc(fake[n])
        s, p = O.sk_ssim(lab, res), float(O.cal_psnr(lab, res))
        g = float(O.ssim((B[n:n + 1] + 1) / 2, (fake[n:n + 1] + 1) / 2))
        print("image %d: ssim %.8f vs %.8f, psnr %.6f vs %.6f, gauss %.7f vs %.7f" % (n, row[0], s, row[1], p, row[2], g))
        assert abs(row[0] - s) < 1e-5 and abs(row[1] - p) < 1e-4 and abs(row[2] - g) < 2e-5
        assert np.isnan(row[3])   # 64 px: below the MS-SSIM minimum
    for c in range(3):
        assert abs(run64["means"][c] - np.mean([r[c] for r in rows])) < 1e-6
    assert np.isnan(run64["means"][3])


def test_evaluate_panels_and_csv(run64):
    from PIL import Image
    dest = run64["dest"]
    assert sorted(os.listdir(dest)) == ["a_%d.png" % i for i in range(5)] + ["metrics.csv"]
    for n in range(5):
        got = np.asarray(Image.open(os.path.join(dest, "a_%d.png" % n)))
        ref = np.hstack([O.to_u8_hwc(run64[k][n]) for k in ("A", "fake", "B")])
        assert got.shape == (64, 192, 3) and np.array_equal(got, ref), n
    with open(os.path.join(dest, "metrics.csv"), newline="") as f:
        lines = list(csv.reader(f))
    assert lines[0] == ["image", "ssim", "psnr", "ssim_gauss", "ms_ssim"]
    assert [l[0] for l in lines[1:]] == ["a_%d" % i for i in range(5)] + ["mean"]
    for l, row in zip(lines[1:6], run64["rows"]):
        assert l[4] == "" and abs(float(l[1]) - row[0]) < 1e-6 and abs(float(l[2]) - row[1]) < 1e-4


def test_evaluate_how_many_and_no_images(run64):
    import evaluate as E
    rows, _ = E.main(run64["args"] + ["--how_many", "3", "--results_dir", "three"])
    # the second batch is truncated, not dropped.  Its one image goes through the generator alone, where a
    # layer may take another kernel than for a batch of two: fp32 reassociation can move a few uint8 values
    # by one, so that row is compared loosely (one step of one pixel in 12288 moves psnr by < 1e-3 dB)
    assert len(rows) == 3 and _same(rows[:2], run64["rows"][:2])
    assert np.allclose(rows[2][:3], run64["rows"][2][:3], rtol=0, atol=1e-2) and np.isnan(rows[2][3])
    dest = os.path.join(run64["out"], "three", "exp", "test_all_3")
    assert sorted(os.listdir(dest)) == ["a_0.png", "a_1.png", "a_2.png", "metrics.csv"]
    rows, _ = E.main(run64["args"] + ["--no_images", "--results_dir", "scores"])
    assert _same(rows, run64["rows"])
    assert os.listdir(os.path.join(run64["out"], "scores", "exp", "test_all_3")) == ["metrics.csv"]


def test_evaluate_single_dataset_writes_input_result_panels(run64, tmp_path):
    """--model test --dataset_mode single: no labels, [input | result] panels, no CSV."""
    import shutil
    from PIL import Image
    import evaluate as E
    d = tmp_path / "single"
    d.mkdir()
    data = os.path.join(os.path.dirname(run64["out"]), "data", "test_all")
    for i in range(4):   # the single dataset serves the first half of the sorted listing
        shutil.copy(os.path.join(data, "a_%d.png" % i), str(d / ("a_%d.png" % i)))
    rows, means = E.main(["--dataroot", str(d), "--out", run64["out"], "--name", "exp", "--which_epoch", "3",
                          "--gpu_ids", "0", "--batchSize", "2", "--nThreads", "0", "--model", "test",
                          "--results_dir", "single"] + _size_args(64))
    assert rows == [] and means is None
    dest = os.path.join(run64["out"], "single", "exp", "test_3")
    assert sorted(os.listdir(dest)) == ["a_0.png", "a_1.png"]
    for n in range(2):
        got = np.asarray(Image.open(os.path.join(dest, "a_%d.png" % n)))
        ref = np.hstack([O.to_u8_hwc(run64[k][n]) for k in ("A", "fake")])
        assert np.array_equal(got, ref), n


def test_evaluate_unet_batchnorm_runs_in_eval_mode(tmp_path, monkeypatch):
    """unet_128 with dropout and BatchNorm: dropout is off (two runs are bitwise equal) and the running
    buffers are read, not updated."""
    import evaluate as E
    import models
    from options.train_options import default_train_opt
    data, out = str(tmp_path / "data"), str(tmp_path / "out")
    _write_pairs(os.path.join(data, "test_all"), 3, 128, 5)
    net = ["--which_model_netG", "unet_128", "--ngf", "8", "--norm", "batch"]
    torch.manual_seed(9)
    m = models.create_model(default_train_opt(net, gpu_ids=[0], isTrain=False, precision="fp32", name="u",
                                              checkpoints_dir=os.path.join(out, "checkpoints")))
    with torch.no_grad():   # running statistics that differ from any batch's
        for k, v in m.netG.state_dict().items():
            if k.endswith("running_mean"):
                v.normal_(0, 0.1)
            elif k.endswith("running_var"):
                v.uniform_(0.5, 1.5)
    m.save_networks("1")
    saved = {k: v.detach().cpu().clone() for k, v in m.netG.state_dict().items()}
    assert any(k.endswith("running_mean") for k in saved)
    made = []
    create = models.create_model
    monkeypatch.setattr(models, "create_model", lambda o: (made.append(create(o)), made[-1])[1])
    args = ["--dataroot", data, "--out", out, "--name", "u", "--which_epoch", "1", "--gpu_ids", "0", "--batchSize", "2",
            "--nThreads", "0", "--no_images"] + net + _size_args(128)
    rows1, _ = E.main(args)
    rows2, _ = E.main(args)
    assert len(rows1) == 3 and _same(rows1, rows2)
    assert all(np.isfinite(r[:3]).all() and np.isnan(r[3]) for r in rows1)
    for model in made:
        assert not model.netG.training
        for k, v in model.netG.state_dict().items():
            assert torch.equal(v.cpu(), saved[k]), k


def test_train_eval_pass_leaves_training_bit_identical(tmp_path):
    import train as T
    data = str(tmp_path / "data")
    _write_pairs(os.path.join(data, "train_all"), 4, 64, 2)
    finals = []
    for tag, extra in (("off", ["--eval_freq", "0"]), ("on", ["--eval_freq", "1", "--eval_phase", "train_all/"])):
        out = str(tmp_path / tag)
        model, hist = T.main(["--dataroot", data, "--out", out, "--gpu_ids", "0", "--batchSize", "2", "--nThreads", "0",
                              "--niter", "2", "--niter_decay", "0", "--lr_policy", "step"] + _size_args(64) + extra,
                             output_freq=1)   # (step policy: the lambda rule's last epoch has lr 0 and would train nothing)
        assert len(hist) == 2 and model.netG.training
        assert all(mod.training for mod in model.netG.modules())
        finals.append((model.flatG.data.clone(), model.flatD.data.clone()))
        with open(os.path.join(out, "each_epoch.csv"), newline="") as f:
            lines = list(csv.reader(f))
        if tag == "off":
            assert [l[:2] for l in lines] == [["1", "train"], ["2", "train"]]
        else:
            assert [l[:2] for l in lines] == [["1", "train"], ["1", "test"], ["2", "train"], ["2", "test"]]
            assert all(np.isfinite(float(l[2])) and np.isfinite(float(l[3])) for l in lines)
    assert torch.equal(finals[0][0], finals[1][0])
    assert torch.equal(finals[0][1], finals[1][1])
