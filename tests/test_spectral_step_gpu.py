"""--spectral_norm in the nets and the train step, at 64x64, batch 2, ndf 8:

  * D forward, D input grad and weight_orig / bias grads of basic, pixel and multi against the plain-torch
    float64 model of tests/sn_fixture.py (autograd through W / sigma): the project's fp32 parity
    criterion, 1e-3 relative per tensor;
  * three fp32 optimize_parameters steps against that model stepping torch.optim.Adam: u, v, sigma, the
    losses and the weights after each step, to the same criterion;
  * the stacked batch-2N D pass against the two-pass form; bf16 graph replay against the eager bf16 step,
    bit for bit; an fp16 step the scaler skips (weights and moments untouched, u advanced); --resume bit for
    bit; a 1-rank RCCL exchange bit for bit; a --diffaug step, deterministic.

The model recipe of tests/test_diffaug_step_gpu.py."""
import os
import random
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from sn_fixture import RefSND, gan_loss, sn_params  # noqa: E402
from oracle import dsgan_cpu as O  # noqa: E402
from oracle.recipe import make_params, synth_pair  # noqa: E402

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIZE, BATCH, NDF = 64, 2, 8
PARITY = 1e-3   # README: the fp32 parity criterion
REL_DBATCH = 2e-6   # tests/test_dbatch_gpu.py: stacked vs two-pass weight-grads, fp32 (a reassociation)


def _rel(a, b):
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    return ((a - b).norm() / max(b.norm().item(), 1e-30)).item()


def _load(net, params):
    with torch.no_grad():
        for k, v in net.state_dict().items():
            v.copy_(params[k])
    net.spectral.refresh(iterate=False)


def _model(prec="fp32", seed=20, init=True, pool_size=0, **kw):
    import dsgan_hip
    from options.train_options import default_train_opt
    from models import create_model
    dsgan_hip.require_gpu()
    random.seed(seed)
    np.random.seed(seed)
    torch.manual_seed(seed)
    kw.setdefault("spectral_norm", True)
    m = create_model(default_train_opt(gpu_ids=[0], pool_size=pool_size, precision=prec, batchSize=BATCH, ndf=NDF, **kw))
    nets = [(m.vgg, make_params(O.vgg_param_spec(True), "vgg", 7000))]
    if init:
        nets.append((m.netG, make_params(O.g_param_spec(), "fanin", 1000)))
    with torch.no_grad():
        for net, pr in nets:
            for k, v in net.state_dict().items():
                v.copy_(pr[k])
    if init and m.snD is not None:
        _load(m.netD, sn_params(m.netD))
    return m


def _set(m, seed):
    A, B = synth_pair(BATCH, SIZE, seed=seed)
    m.set_input({"A": A.cuda(), "B": B.cuda(), "A_paths": ["a"] * BATCH, "B_paths": ["b"] * BATCH})
    return A, B


# ---- the nets ----

@pytest.mark.parametrize("kind", ["basic", "pixel", "multi"])
def test_discriminator_forward_and_grads(kind):
    import dsgan_hip
    from dsgan_hip import functional as HF
    from models.networks import define_D
    dsgan_hip.require_gpu()
    HF.set_precision("fp32")
    lsgan = kind == "multi"   # multi needs --no_lsgan: sigmoid + least squares
    net = define_D(6, NDF, kind, 3, "instance", lsgan, "normal", [0], spectral_norm=True)
    assert len(net.spectral.convs) == {"basic": 5, "pixel": 3, "multi": 15}[kind]
    pr = sn_params(net)
    _load(net, pr)
    ref = RefSND(kind, pr, lsgan)
    A, B = synth_pair(BATCH, SIZE, seed=4)
    x = torch.cat((A, B), 1)
    x64 = x.double().requires_grad_(True)
    want = ref(x64)
    gan_loss(want, True, lsgan).backward()
    xd = x.cuda().requires_grad_(True)
    y = net(xd)
    outs = [s[-1] for s in y] if kind == "multi" else [y]
    msg = []
    for i, (o, w) in enumerate(zip(outs, want)):
        assert tuple(o.shape) == tuple(w.shape)
        msg.append("out%d %.1e" % (i, _rel(o, w)))
        assert _rel(o, w) <= PARITY, (kind, i, msg)
    loss = sum(torch.mean((o - 1.0) ** 2) for o in outs) if lsgan else \
        torch.nn.functional.binary_cross_entropy_with_logits(y, torch.ones_like(y))
    loss.backward()
    net.spectral.backward()   # the W_sn leaves' grads onto weight_orig.grad
    torch.cuda.synchronize()
    got = dict((k, p.grad) for k, p in net.named_parameters())
    got["input"] = xd.grad
    wantg = dict((k, p.grad) for k, p in ref.named_parameters())
    wantg["input"] = x64.grad
    assert sorted(got) == sorted(wantg)
    for k, g in got.items():
        assert torch.isfinite(g).all() and g.abs().max() > 0, k
        msg.append("%s %.1e" % (k, _rel(g, wantg[k])))
        assert _rel(g, wantg[k]) <= PARITY, (kind, k, msg)
    assert not net.spectral.scratch.any()
    # sigma is the reference's, and the G step's freeze reaches the W_sn leaves
    assert _rel(net.spectral.sigma, ref.sigmas()) <= 1e-5
    from models.base_model import BaseModel
    BaseModel.set_requires_grad(None, net, False)
    assert not any(w.requires_grad for w in net.spectral.weights)
    net(xd.detach())   # a frozen D still runs
    BaseModel.set_requires_grad(None, net, True)
    assert all(w.requires_grad for w in net.spectral.weights)
    print("\n[%s] %s" % (kind, ", ".join(msg)))


# ---- the step ----

def test_flag_off_leaves_no_trace():
    m = _model(spectral_norm=False)
    assert m.snD is None and getattr(m.netD, "spectral", None) is None
    assert all(k.endswith((".weight", ".bias")) for k in m.netD.state_dict())


def test_three_steps_against_torch_adam():
    m = _model()
    assert m.snD is not None and m.scaler_D is None and not m.cuda_graph
    pr = sn_params(m.netD)
    ref = RefSND("basic", pr, False)
    opt = torch.optim.Adam(ref.parameters(), lr=m.opt.lr, betas=(m.opt.beta1, 0.999))
    names = [k for k, _ in ref.named_parameters()]
    for it in range(3):
        A, B = _set(m, 300 + it)
        m.optimize_parameters()
        torch.cuda.synchronize()
        fake_AB = torch.cat((A, m.fake_B.detach().cpu()), 1).double()
        real_AB = torch.cat((A, B), 1).double()
        lf, lr_ = gan_loss(ref(fake_AB), False, False), gan_loss(ref(real_AB), True, False)
        opt.zero_grad()
        ((lf + lr_) * 0.5).backward()
        opt.step()
        ref.refresh(iterate=True)
        with torch.no_grad():
            lg = gan_loss(ref(fake_AB), True, False)   # the G step reads the updated D
        msg = ["D_fake %.1e" % (abs(m.loss_D_fake.item() - lf.item()) / abs(lf.item())),
               "D_real %.1e" % (abs(m.loss_D_real.item() - lr_.item()) / abs(lr_.item())),
               "G_GAN %.1e" % (abs(m.loss_G_GAN.item() - lg.item()) / abs(lg.item()))]
        assert abs(m.loss_D_fake.item() - lf.item()) <= PARITY * abs(lf.item()), (it, msg)
        assert abs(m.loss_D_real.item() - lr_.item()) <= PARITY * abs(lr_.item()), (it, msg)
        assert abs(m.loss_G_GAN.item() - lg.item()) <= PARITY * abs(lg.item()), (it, msg)
        sd = m.netD.state_dict()
        for k in names:
            msg.append("%s %.1e" % (k, _rel(sd[k], ref.p[k])))
            assert _rel(sd[k], ref.p[k]) <= PARITY, (it, k, msg)
        for pre in ref.layers:
            for s in ("weight_u", "weight_v"):
                e = (sd[pre + s].double().cpu() - ref.p[pre + s]).abs().max().item()
                msg.append("%s %.1e" % (pre + s, e))
                assert e <= PARITY, (it, pre + s, msg)
        e = _rel(m.snD.sigma, ref.sigmas())
        msg.append("sigma %.1e" % e)
        assert e <= PARITY, (it, msg)
        for c, pre in zip(m.snD.convs, ref.layers):
            assert _rel(c.weight, ref.w_sn(pre)[0]) <= PARITY, (it, pre)
        print("\nstep %d: %s" % (it, ", ".join(msg)))
    assert not m.snD.scratch.any()


def test_stacked_d_equals_two_pass():
    """The stacked pass reads the same W_sn buffers: outputs and losses bit for bit; the weight-grads differ by
    the fp32 reassociation of the weight-grad kernels, held to tests/test_dbatch_gpu.py's bar as with the flag off."""
    m = _model()
    assert m.d_batch
    _set(m, 51)
    m.forward()
    res = {}
    for form in (False, True):
        m.d_batch = form
        m.set_requires_grad(m.netD, True)
        m.optimizer_D.zero_grad()
        m.backward_D()
        m.snD.backward()
        torch.cuda.synchronize()
        res[form] = dict(pf=m.pred_fake.detach().clone(), pr=m.pred_real.detach().clone(),
                         L=(m.loss_D_fake.item(), m.loss_D_real.item(), m.loss_D.item()),
                         g={k: p.grad.detach().clone() for k, p in m.netD.named_parameters()})
    two, st = res[False], res[True]
    assert torch.equal(st["pf"], two["pf"]) and torch.equal(st["pr"], two["pr"])
    assert st["L"] == two["L"]
    msg = []
    for k, g2 in two["g"].items():
        assert torch.isfinite(st["g"][k]).all() and g2.abs().max() > 0, k
        msg.append("%s %.2e" % (k, _rel(st["g"][k], g2)))
        assert _rel(st["g"][k], g2) <= REL_DBATCH, (k, msg)
    print("\nstacked vs two-pass under --spectral_norm: %s" % ", ".join(msg))


def _d_state(m):
    torch.cuda.synchronize()
    out = {"G": m.flatG.data, "D": m.flatD.data, "D.m": m.optimizer_D.m, "D.v": m.optimizer_D.v,
           "G.m": m.optimizer_G.m, "G.v": m.optimizer_G.v, "W_sn": m.snD.wsn, "sigma": m.snD.sigma}
    for k, v in m.netD.state_dict().items():
        if k.endswith(("weight_u", "weight_v")):
            out[k] = v
    return {k: v.detach().clone() for k, v in out.items()}


def _diff(a, b):
    assert sorted(a) == sorted(b)
    return [k for k in a if not torch.equal(a[k], b[k])]


def test_graph_steps_equal_eager_steps():
    runs = []
    for graph in (0, 1):
        m = _model("bf16")
        m.cuda_graph = bool(graph)
        rec = []
        for it in range(3):
            _set(m, 300 + it)
            m.optimize_parameters()
            rec.append(dict(_d_state(m), fake_B=m.fake_B.detach().clone()))
        runs.append((rec, bool(m._graphs)))
        assert m.nonfinite_report() == {"G": (0, 3), "D": (0, 3)}
    (eager, cap_e), (graph, cap_g) = runs
    assert not cap_e and cap_g
    for te, tg in zip(eager, graph):
        assert all(torch.isfinite(v).all() for v in te.values())
        assert _diff(te, tg) == []
    assert _diff(eager[1], eager[2]) != [] and not torch.equal(eager[1]["W_sn"], eager[2]["W_sn"])


def test_fp16_skipped_step_leaves_weights_and_advances_u():
    m = _model("fp16")
    m.cuda_graph = False
    _set(m, 300)
    m.optimize_parameters()
    before = _d_state(m)
    assert not m.scaler_D.skipped_last()
    with torch.no_grad():
        m.scaler_D.state[0] = float("inf")   # the scaled D loss, and with it the D gradient, is not finite
    _set(m, 301)
    m.optimize_parameters()
    after = _d_state(m)
    assert m.scaler_D.skipped_last() and m.scaler_D.applied_steps() == 1
    assert not torch.isfinite(m.flatD.grad).all()   # the projection kept it non-finite
    for k in ("D", "D.m", "D.v"):
        assert torch.equal(before[k], after[k]), k
    moved = [k for k in _diff(before, after) if k.endswith("weight_u")]
    assert len(moved) == len(m.snD.convs) - 1, moved   # (the logits conv has R = 1: its u is +-1)
    assert torch.isfinite(after["W_sn"]).all() and torch.isfinite(after["sigma"]).all()
    assert not m.snD.scratch.any()
    assert not torch.equal(before["G"], after["G"])   # the G step went on


def _interrupted(prec, ckpt, first, second, **kw):
    """``first`` steps, save, drop the model, reseed, a fresh model, load, ``second`` more steps."""
    m = _model(prec, checkpoints_dir=str(ckpt), name="exp", **kw)
    for it in range(first):
        _set(m, 700 + it)
        m.optimize_parameters()
    m.save_networks("3")
    m.save_train_state("3")
    keys = set(torch.load(str(ckpt / "exp" / "3_train_state.pth"), map_location="cpu", weights_only=True))
    del m
    m = _model(prec, seed=77, init=False, checkpoints_dir=str(ckpt), name="exp", **kw)
    m.load_networks("3")
    m.load_train_state("3")
    for it in range(first, first + second):
        _set(m, 700 + it)
        m.optimize_parameters()
    return m, keys


def test_resume_is_bitwise(tmp_path):
    kw = dict(pool_size=3)
    a = _model("bf16", checkpoints_dir=str(tmp_path / "a"), name="exp", **kw)
    for it in range(4):
        _set(a, 700 + it)
        a.optimize_parameters()
    A = _d_state(a)
    assert bool(a._graphs)
    del a
    b, keys = _interrupted("bf16", tmp_path / "b", 2, 2, **kw)
    assert _diff(A, _d_state(b)) == []
    # no new field in the state file: u and v travel in the D file
    off = _model("bf16", spectral_norm=False, checkpoints_dir=str(tmp_path / "c"), name="exp", **kw)
    _set(off, 700)
    off.optimize_parameters()
    off.save_train_state("3")
    assert keys == set(torch.load(str(tmp_path / "c" / "exp" / "3_train_state.pth"), map_location="cpu", weights_only=True))
    d_file = torch.load(str(tmp_path / "b" / "exp" / "3_useSE_net_D.pth"), map_location="cpu", weights_only=True)
    assert list(d_file) == list(b.netD.state_dict())
    # the flag-on D file offered to the flag-off run is refused, naming the missing keys
    off.save_dir = b.save_dir
    with pytest.raises(RuntimeError, match="missing keys.*model.0.weight'"):
        off.load_networks("3")


def _nccl_worker(port, out_dir):
    sys.path[:0] = [REPO, os.path.join(REPO, "ds-gan_amd"), os.path.join(REPO, "tests")]
    import torch.distributed as dist
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), HSA_ENABLE_IPC_MODE_LEGACY="0")
    torch.cuda.set_device(0)
    dist.init_process_group("nccl", rank=0, world_size=1, device_id=torch.device("cuda", 0))
    res = {}
    for mode in ("plain", "exchange"):
        m = _model("bf16")
        m.cuda_graph = False
        m.exchange = mode == "exchange"
        for it in range(2):
            _set(m, 40 + it)
            m.optimize_parameters()
        res[mode] = {k: v.cpu() for k, v in _d_state(m).items()}
    torch.save(res, os.path.join(out_dir, "nccl.pt"))
    dist.destroy_process_group()


def test_one_rank_exchange_gives_the_single_process_bits(tmp_path):
    import multiprocessing as mp
    ctx = mp.get_context("spawn")
    p = ctx.Process(target=_nccl_worker, args=(38000 + random.randint(0, 2000), str(tmp_path)))
    p.start()
    p.join(timeout=240)
    assert p.exitcode == 0, p.exitcode
    r = torch.load(tmp_path / "nccl.pt", weights_only=True)
    assert _diff(r["plain"], r["exchange"]) == []


def test_diffaug_step_runs_and_is_deterministic():
    runs = []
    for _ in range(2):
        m = _model(diffaug="translation")
        for it in range(2):
            _set(m, 51 + it)
            m.optimize_parameters()
        assert int(m.diffaug.counter.item()) == 6
        runs.append(_d_state(m))
    assert all(torch.isfinite(v).all() for v in runs[0].values())
    assert _diff(runs[0], runs[1]) == []
