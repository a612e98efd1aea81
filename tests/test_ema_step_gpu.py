"""--ema_decay through the model: the averaged generator beside an unchanged training run, under graph
replay, inside ``ema_scope()``, in the checkpoints, in evaluate.py --use_ema and in train.py's test pass.

Model recipe of tests/test_model_gpu.py (oracle.recipe.make_params, synth_pair) at 64x64, batch <= 2.
The decay is 0.5 throughout (see tests/test_ema_ops_gpu.py); the bar of the average against the float64
recurrence over the recorded weights is the one derived there, K * 2^-22 * max(|p|, |e|).
"""
import csv
import os
import random
import shutil

import numpy as np
import pytest
import torch

from oracle import dsgan_cpu as O
from oracle.recipe import make_params, synth_pair

pytestmark = pytest.mark.gpu
DECAY = 0.5


def _model(precision, ema_decay=DECAY, **kw):
    import dsgan_hip
    from options.train_options import default_train_opt
    from models import create_model
    dsgan_hip.require_gpu()
    random.seed(20)
    torch.manual_seed(20)
    m = create_model(default_train_opt(gpu_ids=[0], pool_size=0, precision=precision, ema_decay=ema_decay, **kw))
    with torch.no_grad():
        for net, pr in ((m.netG, make_params(O.g_param_spec(), "fanin", 1000)),
                        (m.netD, make_params(O.d_param_spec(), "fanin", 5000)),
                        (m.vgg, make_params(O.vgg_param_spec(True), "vgg", 7000))):
            for k, v in net.state_dict().items():
                v.copy_(pr[k])
    if m.ema_on:   # the average starts from the weights just written, as after a checkpoint load
        m.optimizer_G.reset_ema()
    return m


def _step(m, it, b=2):
    A, B = synth_pair(b, 64, seed=700 + it)
    m.set_input({"A": A.cuda(), "B": B.cuda(), "A_paths": ["a"] * b, "B_paths": ["b"] * b})
    m.optimize_parameters()


def _write_pairs(d, n, size, seed):
    from PIL import Image
    rng = np.random.default_rng(seed)
    os.makedirs(d)
    for i in range(n):
        for side in ("a", "b"):
            Image.fromarray(rng.integers(0, 256, (size, size, 3), dtype=np.uint8)).save(os.path.join(d, "%s_%d.png" % (side, i)))


def _size_args(size):
    return ["--loadSize_w", str(size), "--fineSize_w", str(size), "--loadSize_h", str(size), "--fineSize_h", str(size)]


@pytest.mark.parametrize("prec", ["fp32", "bf16"])
def test_training_unchanged_and_average_follows_recurrence(prec):
    K = 3
    on, off = _model(prec), _model(prec, 0.0)
    assert off.optimizer_G.ema is None and not off.ema_on
    assert not hasattr(on.optimizer_D, "ema") or on.optimizer_D.ema is None   # the generator only
    e0 = on.optimizer_G.ema.clone()
    assert torch.equal(e0, on.flatG.data)
    snaps = []
    for it in range(K):
        _step(on, it)
        _step(off, it)
        snaps.append(on.flatG.data.clone())
    torch.cuda.synchronize()
    for a, b in ((on.flatG.data, off.flatG.data), (on.flatD.data, off.flatD.data),
                 (on.optimizer_G.m, off.optimizer_G.m), (on.optimizer_G.v, off.optimizer_G.v),
                 (on.optimizer_D.m, off.optimizer_D.m), (on.optimizer_D.v, off.optimizer_D.v)):
        assert torch.equal(a, b)
    ema = on.optimizer_G.ema
    assert not torch.equal(ema, e0) and not torch.equal(ema, snaps[-1])
    ref, big = e0.double(), float(e0.abs().max())
    for p in snaps:
        ref = ref + (1.0 - DECAY) * (p.double() - ref)
        big = max(big, float(p.abs().max()), float(ref.abs().max()))
    err = float((ema.double() - ref).abs().max())
    print("%s: max|ema - ref64| = %.3g, bar %.3g, moved %.3g" % (prec, err, K * 2.0 ** -22 * big,
                                                                 float((ema - e0).abs().max())))
    assert err <= K * 2.0 ** -22 * big


def test_graph_replay_averages_like_the_eager_step():
    sizes = [2, 2, 2, 1, 1, 2]
    out = []
    for graph in (False, True):
        m = _model("bf16")
        m.cuda_graph = graph
        e0 = m.optimizer_G.ema.clone()
        for it, b in enumerate(sizes):
            _step(m, it, b)
        torch.cuda.synchronize()
        assert bool(m._graphs) == graph
        assert not torch.equal(m.optimizer_G.ema, e0)
        out.append((m.optimizer_G.ema.clone(), m.flatG.data.clone()))
    assert torch.equal(out[0][0], out[1][0]) and torch.equal(out[0][1], out[1][1])


def test_scope_leaves_training_untouched(monkeypatch):
    """bf16 with graph replay: a scope between two replays, with a forward inside it (which rebuilds the
    cached 16-bit and tap-major weight copies from the averaged weights), changes nothing afterwards."""
    A, _ = synth_pair(2, 64, seed=9)
    runs = []
    for enter in (True, False):
        m = _model("bf16")
        assert m.cuda_graph
        for it in range(3):   # warm-up, capture, replay
            _step(m, it)
        if enter:
            g0, e0 = m.flatG.data.clone(), m.optimizer_G.ema.clone()
            with torch.no_grad():
                raw = m.netG(A.cuda()).clone()
                with m.ema_scope() as net:
                    assert net is m.netG
                    assert torch.equal(m.flatG.data, e0) and torch.equal(m.optimizer_G.ema, g0)
                    avg = m.netG(A.cuda()).clone()
                again = m.netG(A.cuda()).clone()
            assert torch.equal(m.flatG.data, g0) and torch.equal(m.optimizer_G.ema, e0)
            assert torch.equal(raw, again) and not torch.equal(raw, avg)
            with monkeypatch.context() as mp:   # no scope while a graph is being captured
                mp.setattr(torch.cuda, "is_current_stream_capturing", lambda: True)
                with pytest.raises(RuntimeError, match="capture"):
                    with m.ema_scope():
                        pass
            assert torch.equal(m.flatG.data, g0) and torch.equal(m.optimizer_G.ema, e0)
        assert len(m._graphs) == 1
        _step(m, 3)
        _step(m, 4)
        torch.cuda.synchronize()
        runs.append((m.flatG.data.clone(), m.optimizer_G.ema.clone(), m.flatD.data.clone(), m.fake_B.detach().clone()))
    for a, b in zip(*runs):
        assert torch.equal(a, b)


def test_scope_needs_the_average():
    m = _model("fp32", 0.0)
    with pytest.raises(RuntimeError, match="ema_decay"):
        with m.ema_scope():
            pass
    from options.train_options import default_train_opt
    from models import create_model
    for bad in (1.0, -0.5, 1.5):
        with pytest.raises(ValueError, match="ema_decay"):
            create_model(default_train_opt(gpu_ids=[0], ema_decay=bad))


@pytest.fixture(scope="module")
def ckpt(tmp_path_factory):
    """A bf16 run with the average on, two steps at a learning rate large enough that the averaged and the
    raw generator give visibly different images, saved as epoch 3."""
    root = tmp_path_factory.mktemp("ema_ckpt")
    out = str(root / "out")
    m = _model("bf16", lr=5e-3, name="exp", checkpoints_dir=os.path.join(out, "checkpoints"))
    init = m.flatG.data.clone()
    for it in range(2):
        _step(m, it)
    m.save_networks("3")
    torch.cuda.synchronize()
    return {"m": m, "out": out, "dir": os.path.join(out, "checkpoints", "exp"), "init": init.cpu(),
            "g": m.flatG.data.cpu().clone(), "ema": m.optimizer_G.ema.cpu().clone()}


def test_checkpoint_files(ckpt, tmp_path):
    assert sorted(os.listdir(ckpt["dir"])) == ["3_useSE_net_D.pth", "3_useSE_net_G.pth", "3_useSE_net_G_ema.pth"]
    g = torch.load(os.path.join(ckpt["dir"], "3_useSE_net_G.pth"), weights_only=True)
    e = torch.load(os.path.join(ckpt["dir"], "3_useSE_net_G_ema.pth"), weights_only=True)
    assert list(g.keys()) == list(e.keys())
    assert all(g[k].shape == e[k].shape and g[k].dtype == e[k].dtype for k in g)
    m = ckpt["m"]
    names = {id(p): k for k, p in m.netG.named_parameters()}
    seen = 0
    for p, view in m.optimizer_G.ema_views(m.netG):
        assert torch.equal(e[names[id(p)]], view.cpu()) and torch.equal(g[names[id(p)]], p.detach().cpu())
        seen += 1
    assert seen == len(names) and any(not torch.equal(g[k], e[k]) for k in g)
    # saving left the run as it was
    assert torch.equal(m.flatG.data.cpu(), ckpt["g"]) and torch.equal(m.optimizer_G.ema.cpu(), ckpt["ema"])
    # with the average off, the files are the two of before
    off = _model("fp32", 0.0, name="off", checkpoints_dir=str(tmp_path))
    off.save_networks("3")
    assert sorted(os.listdir(str(tmp_path / "off"))) == ["3_useSE_net_D.pth", "3_useSE_net_G.pth"]


@pytest.mark.parametrize("ema_file", ["3_useSE_net_G_ema.pth", "3_net_G_ema.pth", None])
def test_continue_train_restores_the_average(ckpt, tmp_path, ema_file):
    from options.train_options import default_train_opt
    from models import create_model
    d = str(tmp_path / "checkpoints" / "exp")
    shutil.copytree(ckpt["dir"], d)
    if ema_file is None:
        os.remove(os.path.join(d, "3_useSE_net_G_ema.pth"))
    elif ema_file != "3_useSE_net_G_ema.pth":   # the reference's load name; ``module.`` prefixes stripped
        sd = torch.load(os.path.join(d, "3_useSE_net_G_ema.pth"), weights_only=True)
        os.remove(os.path.join(d, "3_useSE_net_G_ema.pth"))
        torch.save({"module." + k: v for k, v in sd.items()}, os.path.join(d, ema_file))
    torch.manual_seed(31)
    opt = default_train_opt(gpu_ids=[0], pool_size=0, precision="bf16", ema_decay=DECAY, name="exp",
                            checkpoints_dir=str(tmp_path / "checkpoints"), continue_train=True, which_epoch="3")
    m = create_model(opt)
    fresh = m.flatG.data.cpu().clone()
    assert torch.equal(m.optimizer_G.ema.cpu(), fresh)
    m.setup(opt)
    assert torch.equal(m.flatG.data.cpu(), ckpt["g"]) and not torch.equal(fresh, ckpt["g"])
    if ema_file is None:   # from the loaded weights, never from the random init made before loading
        assert torch.equal(m.optimizer_G.ema.cpu(), ckpt["g"])
        assert not torch.equal(m.optimizer_G.ema.cpu(), fresh)
    else:
        assert torch.equal(m.optimizer_G.ema.cpu(), ckpt["ema"])
        assert not torch.equal(ckpt["ema"], ckpt["g"])


def test_scope_output_is_the_saved_generator(ckpt):
    from dsgan_hip import functional as HF
    from options.train_options import default_train_opt
    from models import create_model
    m = ckpt["m"]
    fresh = create_model(default_train_opt(gpu_ids=[0], isTrain=False, precision="bf16", name="exp",
                                           checkpoints_dir=os.path.join(ckpt["out"], "checkpoints")))
    fresh.load_suffix = "_ema"
    fresh.load_networks("3")
    assert HF.get_precision() == "bf16"
    A, _ = synth_pair(2, 64, seed=11)
    A = A.cuda()
    flags = [(mod, mod.training) for mod in m.netG.modules()]
    m.netG.eval()
    fresh.netG.eval()
    with torch.no_grad():
        raw = m.netG(A).clone()
        with m.ema_scope():
            avg = m.netG(A).clone()
        want = fresh.netG(A)
    for mod, t in flags:
        mod.training = t
    assert torch.equal(avg, want)
    assert not torch.equal(avg, raw)


def test_evaluate_use_ema(ckpt, tmp_path):
    import evaluate as E
    data, out = str(tmp_path / "data"), str(tmp_path / "out")
    _write_pairs(os.path.join(data, "test_all"), 5, 64, 3)
    shutil.copytree(ckpt["dir"], os.path.join(out, "checkpoints", "exp"))
    args = ["--dataroot", data, "--out", out, "--name", "exp", "--which_epoch", "3", "--gpu_ids", "0",
            "--batchSize", "2", "--nThreads", "0", "--no_images", "--precision", "bf16"] + _size_args(64)
    rows, means = E.main(args)
    rows_e, means_e = E.main(args + ["--use_ema"])
    base = os.path.join(out, "epoch_8_result_original/", "exp")
    assert sorted(os.listdir(base)) == ["test_all_3", "test_all_3_ema"]
    assert os.listdir(os.path.join(base, "test_all_3_ema")) == ["metrics.csv"]
    assert len(rows) == len(rows_e) == 5
    print("raw means %s, ema means %s" % (list(means), list(means_e)))
    for r, e in zip(rows, rows_e):
        assert np.isfinite(e[:3]).all() and not np.array_equal(np.asarray(r[:3]), np.asarray(e[:3]))
    # the module.-prefixed reference name is read as well, to the same rows
    d = os.path.join(out, "checkpoints", "exp")
    sd = torch.load(os.path.join(d, "3_useSE_net_G_ema.pth"), weights_only=True)
    os.remove(os.path.join(d, "3_useSE_net_G_ema.pth"))
    torch.save({"module." + k: v for k, v in sd.items()}, os.path.join(d, "3_net_G_ema.pth"))
    rows_m, _ = E.main(args + ["--use_ema", "--results_dir", "again"])
    assert np.array_equal(np.asarray(rows_m)[:, :3], np.asarray(rows_e)[:, :3])
    os.remove(os.path.join(d, "3_net_G_ema.pth"))
    with pytest.raises(FileNotFoundError, match="3_net_G_ema.pth") as ei:
        E.main(args + ["--use_ema", "--results_dir", "missing"])
    assert d in str(ei.value) and "3_useSE_net_G_ema.pth" in str(ei.value)
    assert not os.path.exists(os.path.join(out, "missing"))


def test_train_eval_pass_with_the_average(tmp_path):
    """Two epochs of two bf16 steps (the second epoch replays the graphs captured in the first): with
    --eval_freq 1 each epoch gets its test and test_ema rows, and the run ends on the same bits."""
    import train as T
    data = str(tmp_path / "data")
    _write_pairs(os.path.join(data, "train_all"), 4, 64, 2)
    finals = []
    for tag, extra in (("off", []), ("on", ["--eval_freq", "1", "--eval_phase", "train_all/"])):
        out = str(tmp_path / tag)
        model, hist = T.main(["--dataroot", data, "--out", out, "--gpu_ids", "0", "--batchSize", "2", "--nThreads", "0",
                              "--niter", "2", "--niter_decay", "0", "--lr_policy", "step", "--precision", "bf16",
                              "--ema_decay", str(DECAY)] + _size_args(64) + extra, output_freq=1)
        assert len(hist) == 2 and model.ema_on and all(mod.training for mod in model.netG.modules())
        finals.append((model.flatG.data.clone(), model.optimizer_G.ema.clone(), model.flatD.data.clone()))
        with open(os.path.join(out, "each_epoch.csv"), newline="") as f:
            lines = list(csv.reader(f))
        kinds = ["train"] if tag == "off" else ["train", "test", "test_ema"]
        assert [l[:2] for l in lines] == [[str(e), k] for e in (1, 2) for k in kinds]
        assert all(np.isfinite(float(l[2])) and np.isfinite(float(l[3])) for l in lines)
        if tag == "on":   # the averaged generator is scored, not the raw one twice
            assert any(lines[i][2:] != lines[i + 1][2:] for i in (1, 4))
        saved = sorted(os.listdir(os.path.join(out, "checkpoints", "experiment_name")))
        assert [s for s in saved if s.endswith(".pth")] == sorted(
            "%d_useSE_net_%s.pth" % (e, n) for e in (1, 2) for n in ("D", "G", "G_ema"))
    assert not torch.equal(finals[0][0], finals[0][1])
    for a, b in zip(*finals):
        assert torch.equal(a, b)
