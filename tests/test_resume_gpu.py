"""Resumable training through the model and train.py: a run that is saved (save_networks + save_train_state),
dropped and continued in a fresh process-like state (another seed, a new model, load_networks + load_ema +
load_train_state) ends on the same bits as the run that never stopped.

Model recipe of tests/test_ema_step_gpu.py (oracle.recipe.make_params, synth_pair) at 64x64, batch 2, with
``pool_size=3`` (the ImagePool is full and draws python ``random`` from step 2 on) and ``ema_decay=0.5``.
"""
import csv
import os
import random
import shutil
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from bn_fixture import d_params_bn  # noqa: E402
from unet_fixture import unet_spec, unet_params  # noqa: E402
from oracle import dsgan_cpu as O  # noqa: E402
from oracle.recipe import make_params, synth_pair  # noqa: E402

pytestmark = pytest.mark.gpu
DECAY, POOL = 0.5, 3


def _model(precision, ckpt, seed=20, init=True, **kw):
    """``init``: the recipe's weights (a first start); else whatever the seed drew (a restart, before it
    loads).  The VGG weights are in no checkpoint: both get them."""
    import dsgan_hip
    from options.train_options import default_train_opt
    from models import create_model
    dsgan_hip.require_gpu()
    random.seed(seed)
    np.random.seed(seed)
    torch.manual_seed(seed)
    m = create_model(default_train_opt(gpu_ids=[0], pool_size=POOL, precision=precision, ema_decay=DECAY, name="exp",
                                       checkpoints_dir=str(ckpt), **kw))
    nets = [(m.vgg, make_params(O.vgg_param_spec(True), "vgg", 7000))]
    if init:
        nets += [(m.netG, make_params(O.g_param_spec(), "fanin", 1000)), (m.netD, make_params(O.d_param_spec(), "fanin", 5000))]
    with torch.no_grad():
        for net, pr in nets:
            for k, v in net.state_dict().items():
                v.copy_(pr[k])
    m.optimizer_G.reset_ema()
    return m


def _step(m, it, b=2, size=64):
    A, B = synth_pair(b, size, seed=700 + it)
    m.set_input({"A": A.cuda(), "B": B.cuda(), "A_paths": ["a"] * b, "B_paths": ["b"] * b})
    m.optimize_parameters()


def _snap(m):
    torch.cuda.synchronize()
    out = {"G": m.flatG.data, "D": m.flatD.data, "G.m": m.optimizer_G.m, "G.v": m.optimizer_G.v,
           "D.m": m.optimizer_D.m, "D.v": m.optimizer_D.v, "ema": m.optimizer_G.ema,
           "pool": m.fake_AB_pool.store[:m.fake_AB_pool.num_imgs]}
    for k, sc in (("scaler_G", m.scaler_G), ("scaler_D", m.scaler_D)):
        if sc is not None:
            out[k] = sc.state
    for k, v in list(m.netG.state_dict().items()) + list(m.netD.state_dict().items()):
        if k.endswith(("running_mean", "running_var", "num_batches_tracked")):
            out["buf." + k + str(len(out))] = v
    out = {k: v.detach().clone() for k, v in out.items()}
    out["num_imgs"], out["py"], out["calls"] = m.fake_AB_pool.num_imgs, random.getstate(), dict(m.step_calls)
    return out


def _same(a, b):
    assert sorted(a) == sorted(b)
    return [k for k in a if not (torch.equal(a[k], b[k]) if torch.is_tensor(a[k]) else a[k] == b[k])]


def _ptrs(m):
    out = [m.optimizer_G.m.data_ptr(), m.optimizer_G.v.data_ptr(), m.optimizer_D.m.data_ptr(), m.optimizer_D.v.data_ptr(),
           m.optimizer_G.ema.data_ptr(), m.flatG.data.data_ptr(), m.flatD.data.data_ptr()]
    return out + [sc.state.data_ptr() for sc in (m.scaler_G, m.scaler_D) if sc is not None]


def _resume(m, epoch, state=True):
    m.load_networks(epoch)
    m.load_ema(epoch)
    if state:
        m.load_train_state(epoch)


def _interrupted(precision, ckpt, first, second, before=None, step=_step, **kw):
    """``first`` steps, save, drop the model, reseed, a fresh model, load, ``second`` more steps."""
    m = _model(precision, ckpt, **kw)
    for it in range(first):
        if before is not None:
            before(m, it)
        step(m, it)
    m.save_networks("3")
    path = m.save_train_state("3")
    assert os.path.basename(path) == "3_train_state.pth"
    del m
    m = _model(precision, ckpt, seed=77, init=False, **kw)
    ptrs = _ptrs(m)
    _resume(m, "3")
    assert _ptrs(m) == ptrs   # in place: captured graphs hold these pointers
    for it in range(first, first + second):
        step(m, it)
    return m


@pytest.mark.parametrize("prec", ["fp32", "bf16", "fp16"])
def test_resume_is_bitwise(prec, tmp_path):
    a = _model(prec, tmp_path / "a")
    assert a.cuda_graph == (prec != "fp32") and (a.scaler_G is None) == (prec == "fp32")
    for it in range(6):
        _step(a, it)
    A = _snap(a)
    assert A["num_imgs"] == POOL and A["py"] != random.Random(20).getstate()   # the pool drew from `random`
    assert bool(a._graphs) == (prec != "fp32")
    del a
    b = _interrupted(prec, tmp_path / "b", 3, 3)
    assert bool(b._graphs) == (prec != "fp32")
    B = _snap(b)
    assert _same(A, B) == []
    assert sorted(os.listdir(str(tmp_path / "b" / "exp"))) == ["3_train_state.pth", "3_useSE_net_D.pth",
                                                                "3_useSE_net_G.pth", "3_useSE_net_G_ema.pth"]
    sd = torch.load(str(tmp_path / "b" / "exp" / "3_train_state.pth"), map_location="cpu", weights_only=True)
    assert sd["epoch"] == "3" and sd["world_size"] == 1 and sd["precision"] == prec and sd["step_calls"] == {"G": 3, "D": 3}
    assert float(sd["optimizer_G"]["state"][0]["step"]) == 3.0
    assert sd["optimizer_G"]["param_names"] == [k for k, _ in b.netG.named_parameters()]
    # the control: today's --continue_train (the networks and the average only) does not get there
    del b
    c = _model(prec, tmp_path / "b", seed=77, init=False)
    _resume(c, "3", state=False)
    for it in range(3, 6):
        _step(c, it)
    C = _snap(c)
    assert "G" in _same(A, C) and "G.m" in _same(A, C)


def test_a_skipped_step_survives(tmp_path):
    """fp16: the generator's scale is raised before step 1, which overflows: the skipped-step counts and the
    backed-off scale are the uninterrupted run's after the restart."""
    def overflow(m, it):
        if it == 1:
            m.scaler_G.state[0].fill_(2.0 ** 126)

    a = _model("fp16", tmp_path / "a")
    for it in range(5):
        overflow(a, it)
        _step(a, it)
    A = _snap(a)
    rep, scales = a.nonfinite_report(), (a.scaler_G.get_scale(), a.scaler_D.get_scale())
    print("uninterrupted: skipped %s, scales %s" % (rep, scales))
    assert rep["G"][0] >= 1 and rep["G"][1] == 5 and rep["D"][1] == 5 and scales[0] < 2.0 ** 126
    del a
    b = _interrupted("fp16", tmp_path / "b", 3, 2, before=overflow)
    assert b.nonfinite_report() == rep and (b.scaler_G.get_scale(), b.scaler_D.get_scale()) == scales
    assert _same(A, _snap(b)) == []


def _unet(precision, ckpt, seed=20, init=True):
    import dsgan_hip
    from options.train_options import default_train_opt
    from models import create_model
    dsgan_hip.require_gpu()
    random.seed(seed)
    torch.manual_seed(seed)
    m = create_model(default_train_opt(gpu_ids=[0], pool_size=POOL, precision=precision, ema_decay=DECAY, name="exp",
                                       checkpoints_dir=str(ckpt), batchSize=1, no_lsgan=False, which_model_netD="basic",
                                       norm="batch", which_model_netG="unet_128", ngf=8, no_dropout=False))
    nets = [(m.vgg, make_params(O.vgg_param_spec(True), "vgg", 7000))]
    if init:
        gspec = unet_spec(3, 3, 7, 8, "batch", True)
        dspec = [(k, tuple(v.shape)) for k, v in m.netD.state_dict().items()]
        nets += [(m.netG, unet_params(gspec)), (m.netD, d_params_bn(dspec))]
    with torch.no_grad():
        for net, pr in nets:
            for k, v in net.state_dict().items():
                v.copy_(pr[k])
    m.optimizer_G.reset_ema()
    return m


def test_unet_dropout_and_batchnorm_resume(tmp_path):
    """unet_128 with dropout and --norm batch, 128x128, batch 1, 2 + 2 steps: the dropout layers' counters,
    seed and stream ids come from the state file, the BatchNorm running buffers from the network files."""
    step = lambda m, it: _step(m, it, b=1, size=128)   # noqa: E731
    a = _unet("fp32", tmp_path / "a")
    blocks = a.netG.dropout_blocks()
    assert len(blocks) == 2 and blocks[0].drop_seed == 20
    for it in range(4):
        step(a, it)
    A = _snap(a)
    A["drop"] = [(int(b.drop_counter), b.drop_seed, b.drop_stream) for b in blocks]
    assert [d[0] for d in A["drop"]] == [4, 4] and any(k.startswith("buf.") for k in A)
    del a, blocks
    m = _unet("fp32", tmp_path / "b")
    for it in range(2):
        step(m, it)
    m.save_networks("3")
    m.save_train_state("3")
    del m
    m = _unet("fp32", tmp_path / "b", seed=77, init=False)
    assert m.netG.dropout_blocks()[0].drop_seed == 77
    counters = [b.drop_counter.data_ptr() for b in m.netG.dropout_blocks()]
    _resume(m, "3")
    assert [b.drop_counter.data_ptr() for b in m.netG.dropout_blocks()] == counters
    for it in range(2, 4):
        step(m, it)
    B = _snap(m)
    B["drop"] = [(int(b.drop_counter), b.drop_seed, b.drop_stream) for b in m.netG.dropout_blocks()]
    assert _same(A, B) == []


@pytest.fixture(scope="module")
def saved(tmp_path_factory):
    """An fp32 run of two steps, saved as epoch 3."""
    ckpt = tmp_path_factory.mktemp("resume_ckpt")
    m = _model("fp32", ckpt)
    for it in range(2):
        _step(m, it)
    m.save_networks("3")
    m.save_train_state("3")
    torch.cuda.synchronize()
    return {"m": m, "ckpt": ckpt, "dir": os.path.join(str(ckpt), "exp")}


def test_torch_adam_interop(saved):
    m = saved["m"]
    opt = m.optimizer_D
    sd = opt.state_dict()
    assert float(sd["state"][0]["step"]) == 2.0 and sd["param_groups"][0]["betas"] == [0.5, 0.999]
    clones = [torch.nn.Parameter(p.detach().cpu().clone()) for p in m.flatD.params]
    ref = torch.optim.Adam(clones, lr=2e-4, betas=(0.5, 0.999))
    ref.load_state_dict(sd)
    offs = {id(p): off for p, off, _ in m.flatD.layout}
    for p, q in zip(m.flatD.params, clones):
        st = ref.state[q]
        assert torch.equal(st["exp_avg"], opt.m[offs[id(p)]:offs[id(p)] + p.numel()].view(p.shape).cpu())
        assert float(st["step"]) == 2.0
    g = torch.Generator().manual_seed(5)
    grads = [torch.randn(p.shape, generator=g) * 1e-2 for p in clones]
    opt.zero_grad()
    for p, q, gr in zip(m.flatD.params, clones, grads):
        p.grad.copy_(gr)
        q.grad = gr.clone()
    data0, m0, v0, n0 = m.flatD.data.clone(), opt.m.clone(), opt.v.clone(), opt.step_count
    opt.step()
    ref.step()
    torch.cuda.synchronize()
    err = max(float((p.detach().cpu() - q.detach()).abs().max()) for p, q in zip(m.flatD.params, clones))
    print("one step after the load: max |FlatAdam - torch.optim.Adam| = %.3g" % err)
    for p, q in zip(m.flatD.params, clones):
        assert torch.allclose(p.detach().cpu(), q.detach(), rtol=1e-6, atol=1e-7)
    # the reverse: torch's state dict (now at step 3) into FlatAdam, bit for bit and in place
    ptrs = (opt.m.data_ptr(), opt.v.data_ptr())
    with torch.no_grad():
        opt.m.zero_(), opt.v.zero_()
    opt.load_state_dict(ref.state_dict())
    assert (opt.m.data_ptr(), opt.v.data_ptr()) == ptrs and opt.step_count == 3 == opt.applied_steps()
    for p, q in zip(m.flatD.params, clones):
        o = offs[id(p)]
        assert torch.equal(opt.m[o:o + p.numel()].view(p.shape).cpu(), ref.state[q]["exp_avg"])
        assert torch.equal(opt.v[o:o + p.numel()].view(p.shape).cpu(), ref.state[q]["exp_avg_sq"])
    assert opt.param_groups[0]["lr"] == 2e-4   # lr is the scheduler's, never the file's
    with torch.no_grad():   # leave the fixture's model as it was saved
        m.flatD.data.copy_(data0), opt.m.copy_(m0), opt.v.copy_(v0)
    opt.step_count = n0


def test_verification_bites(saved, tmp_path):
    from dsgan_hip import functional as HF
    d = str(tmp_path / "exp")
    shutil.copytree(saved["dir"], d)
    path = os.path.join(d, "3_train_state.pth")
    sd = torch.load(path, map_location="cpu", weights_only=True)
    assert sorted(sd["fingerprints"]) == ["D.data", "D.exp_avg", "D.exp_avg_sq", "G.data", "G.ema", "G.exp_avg", "G.exp_avg_sq"]
    assert sd["fingerprints"]["D.exp_avg"] == "%016x" % HF.fingerprint(saved["m"].optimizer_D.m)
    m = _model("fp32", tmp_path, seed=5, init=False)
    _resume(m, "3")   # the untouched copy loads
    assert torch.equal(m.optimizer_G.v, saved["m"].optimizer_G.v)
    # one element of a saved moment changed in the file
    t = sd["optimizer_D"]["state"][1]["exp_avg"]
    t.view(-1)[0] = t.view(-1)[0] + 1.0
    torch.save(sd, path)
    with pytest.raises(RuntimeError, match=r"D\.exp_avg has fingerprint"):
        _resume(m, "3")
    # a weight file of another epoch beside the state
    shutil.copy(os.path.join(saved["dir"], "3_train_state.pth"), path)
    with torch.no_grad():
        m.flatG.data[0] += 1.0
    assert m.save_dir == d
    torch.save({k: v.detach().cpu() for k, v in m.netG.state_dict().items()}, os.path.join(d, "3_useSE_net_G.pth"))
    with pytest.raises(RuntimeError, match=r"G\.data has fingerprint"):
        _resume(m, "3")
    # another precision, another world size
    try:
        other = _model("bf16", tmp_path, seed=5, init=False)
        shutil.copy(os.path.join(saved["dir"], "3_useSE_net_G.pth"), os.path.join(d, "3_useSE_net_G.pth"))
        with pytest.raises(RuntimeError, match="--precision fp32, this run uses bf16"):
            _resume(other, "3")
    finally:
        HF.set_precision("fp32")
    sd = torch.load(path, map_location="cpu", weights_only=True)
    sd["world_size"] = 8
    torch.save(sd, path)
    with pytest.raises(RuntimeError, match="saved by 8 rank"):
        m.load_train_state("3")


def _write_pairs(d, n, size, seed):
    from PIL import Image
    rng = np.random.default_rng(seed)
    os.makedirs(d)
    for i in range(n):
        for side in ("a", "b"):
            Image.fromarray(rng.integers(0, 256, (size, size, 3), dtype=np.uint8)).save(os.path.join(d, "%s_%d.png" % (side, i)))


def _lrs(text):
    return [line for line in text.splitlines() if line.startswith("learning rate = ")]


@pytest.mark.parametrize("prec", ["fp32", "bf16"])
def test_train_resume_end_to_end(prec, tmp_path, capsys):
    """4 PNG pairs of 64x64, batch 2, shuffled, no workers, --niter 2 --niter_decay 1: straight through against
    --resume --stop_after_epoch 2 followed by the same command with --resume alone."""
    import train as T
    data = str(tmp_path / "data")
    _write_pairs(os.path.join(data, "train_all"), 4, 64, 2)

    def args(out):
        return ["--dataroot", data, "--out", out, "--gpu_ids", "0", "--batchSize", "2", "--nThreads", "0", "--niter", "2",
                "--niter_decay", "1", "--precision", prec, "--ema_decay", str(DECAY), "--pool_size", str(POOL),
                "--loadSize_w", "64", "--fineSize_w", "64", "--loadSize_h", "64", "--fineSize_h", "64"]

    one, two = str(tmp_path / "one"), str(tmp_path / "two")
    capsys.readouterr()
    _, hist = T.main(args(one), output_freq=1)
    lr_one = _lrs(capsys.readouterr().out)
    assert [h[0] for h in hist] == [1, 2, 3] and len(lr_one) == 3 and len(set(lr_one)) == 3
    ck_one, ck_two = (os.path.join(o, "checkpoints", "experiment_name") for o in (one, two))
    assert not any("train_state" in n for n in os.listdir(ck_one))   # the flags are off: no state file
    _, hist = T.main(args(two) + ["--resume", "--stop_after_epoch", "2"], output_freq=1)
    text = capsys.readouterr().out
    assert [h[0] for h in hist] == [1, 2] and "starting fresh" in text
    lr_two = _lrs(text)
    assert sorted(n for n in os.listdir(ck_two) if "train_state" in n) == ["1_train_state.pth", "2_train_state.pth"]
    model, hist = T.main(args(two) + ["--resume"], output_freq=1)
    text = capsys.readouterr().out
    assert [h[0] for h in hist] == [3] and "continuing after epoch 2" in text
    lr_two += _lrs(text)
    assert lr_two == lr_one
    for name in ("3_useSE_net_G.pth", "3_useSE_net_D.pth", "3_useSE_net_G_ema.pth"):
        x = torch.load(os.path.join(ck_one, name), map_location="cpu", weights_only=True)
        y = torch.load(os.path.join(ck_two, name), map_location="cpu", weights_only=True)
        assert list(x) == list(y) and all(torch.equal(x[k], y[k]) for k in x), name
    rows = []
    for o in (one, two):
        with open(os.path.join(o, "each_epoch.csv"), newline="") as f:
            rows.append(list(csv.reader(f)))
    assert rows[0] == rows[1] and [r[:2] for r in rows[0]] == [[str(e), "train"] for e in (1, 2, 3)]
    # --keep_states 2: the state files of the two newest epochs, and every network file
    assert sorted(n for n in os.listdir(ck_two) if "train_state" in n) == ["2_train_state.pth", "3_train_state.pth"]
    assert sorted(n for n in os.listdir(ck_two) if "_net_" in n) == sorted(n for n in os.listdir(ck_one) if "_net_" in n)
    assert len([n for n in os.listdir(ck_two) if "_net_" in n]) == 9
