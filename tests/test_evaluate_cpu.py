"""evaluate.py's host side, without a GPU: where the results go, the options it refuses, the CSV it
writes, and that the per-image ssim refuses a gradient before any device call."""
import csv
import types

import pytest
import torch


def _opt(**kw):
    o = types.SimpleNamespace(results_dir="epoch_8_result_original/", name="exp", phase="test_all/", which_epoch="8",
                              aspect_ratio=1.0, how_many=1000)
    for k, v in kw.items():
        setattr(o, k, v)
    return o


def test_results_dir_rule(tmp_path):
    import os
    import evaluate as E
    out = str(tmp_path / "out")
    assert E.results_dir(_opt(), out) == os.path.join(out, "epoch_8_result_original/", "exp", "test_all_8")
    # an absolute --results_dir is taken as it is, a nested phase is flattened
    ab = str(tmp_path / "elsewhere")
    assert E.results_dir(_opt(results_dir=ab, phase="val/night", which_epoch="latest"), out) == \
        os.path.join(ab, "exp", "val_night_latest")


def test_eval_options_force_order_and_no_flip():
    import evaluate as E
    o = _opt(serial_batches=False, no_flip=False)
    e = E.eval_options(o, "train_all/")
    assert (e.serial_batches, e.no_flip, e.phase) == (True, True, "train_all/")
    assert (o.serial_batches, o.no_flip, o.phase) == (False, False, "test_all/")   # a copy: the caller's is untouched
    assert E.eval_options(o).phase == "test_all/"


def test_aspect_ratio_refused(tmp_path):
    import evaluate as E
    with pytest.raises(ValueError, match="aspect_ratio"):
        E.check_options(_opt(aspect_ratio=1.5))
    E.check_options(_opt())
    # through main: refused right after the options are parsed, before a model or a loader exists
    with pytest.raises(ValueError, match="aspect_ratio"):
        E.main(["--dataroot", str(tmp_path / "none"), "--out", str(tmp_path / "out"), "--gpu_ids", "-1",
                "--aspect_ratio", "2.0"])


def test_world_size_refused(tmp_path, monkeypatch):
    import evaluate as E
    monkeypatch.setenv("WORLD_SIZE", "2")
    with pytest.raises(RuntimeError, match="single-process"):
        E.main(["--dataroot", str(tmp_path / "none"), "--out", str(tmp_path / "out"), "--gpu_ids", "-1"])


def test_metrics_csv(tmp_path):
    import evaluate as E
    nan = float("nan")
    cols = ("ssim", "psnr", "ssim_gauss", "ms_ssim")
    rows = [[0.5, 20.25, 0.625, nan], [0.25, 10.0, 0.125, nan]]
    p = str(tmp_path / "metrics.csv")
    E.write_metrics_csv(p, cols, ["a_0", "a_1"], rows, [0.375, 15.125, 0.375, nan])
    with open(p, newline="") as f:
        got = list(csv.reader(f))
    assert got[0] == ["image", "ssim", "psnr", "ssim_gauss", "ms_ssim"]
    assert got[1] == ["a_0", "0.5", "20.25", "0.625", ""]
    assert got[2] == ["a_1", "0.25", "10", "0.125", ""]
    assert got[3] == ["mean", "0.375", "15.125", "0.375", ""]
    assert len(got) == 4


@pytest.mark.parametrize("kw", [{"size_average": False}, {"nonnegative_ssim": True}])
def test_per_image_ssim_refuses_grad_before_any_device_call(kw):
    """CPU tensors: a device call would raise RuntimeError (ptr refuses them), so NotImplementedError
    shows that the refusal comes first."""
    import MS_SSIM as M
    X = torch.rand(1, 3, 16, 16, requires_grad=True)
    Y = torch.rand(1, 3, 16, 16)
    with pytest.raises(NotImplementedError):
        M.ssim(X, Y, data_range=1.0, **kw)
    with pytest.raises(NotImplementedError):
        M.ssim(Y, X, data_range=1.0, **kw)
    with torch.no_grad(), pytest.raises(RuntimeError, match="device tensor"):
        M.ssim(X, Y, data_range=1.0, **kw)   # without a gradient it goes to the device path
