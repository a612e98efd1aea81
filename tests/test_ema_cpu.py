"""--ema_decay / --use_ema on the host, without a GPU: the flag, its default and its range, where
evaluate.py --use_ema writes and which checkpoint it asks for."""
import os
import types

import pytest


def test_ema_decay_default_is_off():
    from options.train_options import TrainOptions, default_train_opt
    assert TrainOptions().gather_options([]).ema_decay == 0.0
    assert default_train_opt().ema_decay == 0.0


def test_ema_decay_parses():
    from options.train_options import TrainOptions, default_train_opt
    opt = TrainOptions().gather_options(["--ema_decay", "0.999"])
    assert isinstance(opt.ema_decay, float) and opt.ema_decay == 0.999
    assert default_train_opt(["--ema_decay", "0.5", "--precision", "bf16"]).ema_decay == 0.5
    with pytest.raises(SystemExit):
        TrainOptions().gather_options(["--ema_decay", "often"])


def test_ema_decay_is_a_training_flag_only():
    from options.test_options import TestOptions
    with pytest.raises(SystemExit):
        TestOptions().gather_options(["--ema_decay", "0.5"])


@pytest.mark.parametrize("bad", [1.0, -0.25, 2.0, float("nan")])
def test_ema_decay_outside_range_refused(bad):
    """Refused by the model's initialize, ahead of anything that needs a device."""
    from models import create_model
    from options.train_options import default_train_opt
    with pytest.raises(ValueError, match="ema_decay"):
        create_model(default_train_opt(gpu_ids=[], ema_decay=bad))


def test_results_dir_with_use_ema(tmp_path):
    import evaluate as E
    opt = types.SimpleNamespace(results_dir="epoch_8_result_original/", name="exp", phase="test_all/", which_epoch="8")
    out = str(tmp_path / "out")
    raw = E.results_dir(opt, out)
    assert raw == os.path.join(out, "epoch_8_result_original/", "exp", "test_all_8")
    assert E.results_dir(opt, out, False) == raw
    assert E.results_dir(opt, out, True) == raw + "_ema"
    opt.results_dir, opt.phase, opt.which_epoch = str(tmp_path / "abs"), "val/night", "latest"
    assert E.results_dir(opt, out, True) == os.path.join(str(tmp_path / "abs"), "exp", "val_night_latest_ema")


def test_ema_checkpoint_lookup(tmp_path):
    import evaluate as E
    d = str(tmp_path)
    with pytest.raises(FileNotFoundError) as ei:
        E.ema_checkpoint(d, "8")
    assert os.path.join(d, "8_net_G_ema.pth") in str(ei.value)
    assert os.path.join(d, "8_useSE_net_G_ema.pth") in str(ei.value)
    open(os.path.join(d, "8_useSE_net_G_ema.pth"), "wb").close()
    assert E.ema_checkpoint(d, "8") == os.path.join(d, "8_useSE_net_G_ema.pth")
    open(os.path.join(d, "8_net_G_ema.pth"), "wb").close()   # the reference's load name comes first
    assert E.ema_checkpoint(d, "8") == os.path.join(d, "8_net_G_ema.pth")


def test_use_ema_without_a_checkpoint_fails_before_any_output(tmp_path):
    import evaluate as E
    out = str(tmp_path / "out")
    with pytest.raises(FileNotFoundError, match="4_net_G_ema.pth"):
        E.main(["--dataroot", str(tmp_path / "none"), "--out", out, "--gpu_ids", "-1", "--name", "exp",
                "--which_epoch", "4", "--use_ema"])
    assert not os.path.exists(os.path.join(out, "epoch_8_result_original"))
