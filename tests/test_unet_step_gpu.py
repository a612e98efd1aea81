"""The train step with ``--which_model_netG unet_128`` (ngf 8, 128x128, batch 2, pool_size 0, the basic
D, BCE; DSGAN/models/pix2pix_model.py:141-217):

  * one fp32 ``optimize_parameters`` with ``--no_dropout``, for ``--norm instance`` and ``--norm batch``,
    against the reference's own step (tests/golden/golden_v7.npz, gen_golden_v7.py) under the bar rules
    of tests/test_batchnorm_step_gpu.py: the nine losses 1e-3 relative against its fp32 and its fp64
    step; fake_B max(1e-3, 3x the reference's own fp32 error, 8x its 1-ulp spread); gradients per tensor
    (the PReLU slopes included) |g - g64| <= max(2 |g32_ref - g64_ref|, 2e-3 |g64|, 8x the 1-ulp spread)
    + 1e-6 on the norm and the probe dot; the G's Adam update per tensor, against the step's own gradient
    (-lr g / (|g| + eps)) and, as a probe dot, against the reference's within the stored margins plus
    2 lr |probe| for every element whose step sign is not determined at fp32 resolution (the rule of
    tests/test_step256_gpu.py); under batch norm the G's running buffers after the step 1e-5
    against the reference's fp64 step and every counter of the G == 1 (the G runs forward once per step);
  * with dropout on (bf16 with the non-finite guard, the mode of the graph step): three steps eagerly and
    three steps of the graph step (an eager warm-up, the capture, a replay), from the same seed and
    counters, are bitwise equal in fake_B and the flat parameter buffers after every step, and each
    dropout counter advances by one per step;
  * a checkpoint round-trips: the saved keys equal the reference's (no dropout state among them) and
    load back bitwise; ``--model test`` builds the same generator and runs it.
"""
import os
import random
import sys
from collections import OrderedDict

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from bn_fixture import d_params_bn  # noqa: E402
from unet_fixture import unet_spec, unet_params  # noqa: E402
from oracle import dsgan_cpu as O  # noqa: E402
from oracle.recipe import make_params, synth_pair, probe  # noqa: E402

pytestmark = pytest.mark.gpu

G7 = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "golden_v7.npz"))
NAMES = ["G_GAN", "G_L1", "D_real", "D_fake", "vgg", "tv", "ssim", "G", "D"]
SIZE, BATCH, NGF = 128, 2, 8


def _model(norm, prec="fp32", dropout=False, **kw):
    import dsgan_hip
    from options.train_options import default_train_opt
    from models import create_model
    dsgan_hip.require_gpu()
    random.seed(20)
    torch.manual_seed(20)
    m = create_model(default_train_opt(gpu_ids=[0], pool_size=0, precision=prec, batchSize=BATCH, no_lsgan=False,
                                       which_model_netD="basic", norm=norm, which_model_netG="unet_128", ngf=NGF,
                                       no_dropout=not dropout, **kw))
    gspec = unet_spec(3, 3, 7, NGF, norm, dropout)
    assert [(k, tuple(v.shape)) for k, v in m.netG.state_dict().items()] == gspec
    dspec = [(k, tuple(v.shape)) for k, v in m.netD.state_dict().items()]
    dp = d_params_bn(dspec) if norm == "batch" else make_params(dspec, "fanin", 5000)
    with torch.no_grad():
        for net, pr in ((m.netG, unet_params(gspec)), (m.netD, dp),
                        (m.vgg, make_params(O.vgg_param_spec(True), "vgg", 7000))):
            for k, v in net.state_dict().items():
                v.copy_(pr[k])
    return m


def _set(m, seed):
    A, B = synth_pair(BATCH, SIZE, seed=seed)
    m.set_input({"A": A.cuda(), "B": B.cuda(), "A_paths": ["a"] * BATCH, "B_paths": ["b"] * BATCH})


def _losses(m):
    return [float(x) for x in (m.loss_G_GAN, m.loss_G_L1, m.loss_D_real, m.loss_D_fake, m.loss_vgg, m.tv_loss,
                               m.loss_ssim, m.loss_G, m.loss_D)]


def _g_buffers(m):
    sd = m.netG.state_dict()
    rm = [v.flatten() for k, v in sd.items() if k.endswith("running_mean")]
    rv = [v.flatten() for k, v in sd.items() if k.endswith("running_var")]
    return (torch.cat(rm) if rm else None, torch.cat(rv) if rv else None,
            [int(v) for k, v in sd.items() if k.endswith("num_batches_tracked")])


def _rel(a, b):
    a, b = a.double().cpu(), b.double().cpu()
    return ((a - b).norm() / max(b.norm().item(), 1e-30)).item()


@pytest.mark.parametrize("norm", ["instance", "batch"])
def test_unet_step_fp32_vs_reference(norm):
    g = G7
    pre, pre64, spr = "S7_%s_f32_" % norm, "S7_%s_f64_" % norm, "S7_%s_spread_" % norm
    m = _model(norm)
    _set(m, int(g["S7_%s_input_seed" % norm]))
    m.optimize_parameters()
    torch.cuda.synchronize()
    report = []
    got = np.array(_losses(m))
    for ref_key in (pre, pre64):
        ref = g[ref_key + "losses"]
        r = np.abs(got - ref) / np.maximum(np.abs(ref), 1e-6)
        report.append("losses vs %s: max rel %.2e" % (ref_key, r.max()))
        assert (r <= 1e-3).all(), (ref_key, dict(zip(NAMES, r)))
    fake = m.fake_B.detach().double().cpu()
    sub = fake[:, :, ::8, ::8].numpy()
    pd = np.array([float(probe(fake.numel(), 70000 + j) @ fake.flatten()) for j in range(4)])

    def fake_err(key):
        s_, nrm = g[key + "fake_sub"].astype(np.float64), float(g[key + "fake_norm"])
        return np.array([np.linalg.norm(sub - s_) / np.linalg.norm(s_), abs(float(fake.norm()) - nrm) / nrm,
                         np.abs(pd - g[key + "fake_pdot"]).max() / nrm])

    own = np.array([np.linalg.norm(g[pre + "fake_sub"].astype(np.float64) - g[pre64 + "fake_sub"])
                    / np.linalg.norm(g[pre64 + "fake_sub"].astype(np.float64)),
                    abs(float(g[pre + "fake_norm"]) - float(g[pre64 + "fake_norm"])) / float(g[pre64 + "fake_norm"]),
                    np.abs(g[pre + "fake_pdot"] - g[pre64 + "fake_pdot"]).max() / float(g[pre64 + "fake_norm"])])
    fbar = np.maximum(np.maximum(1e-3, 3 * own), 8 * float(g[spr + "fake"]))
    for ref_key in (pre, pre64):
        e = fake_err(ref_key)
        report.append("fake_B vs %s: sample %.2e norm %.2e probe %.2e (bar %.1e)" % ((ref_key,) + tuple(e) + (fbar.max(),)))
        assert (e <= fbar).all(), (ref_key, e, fbar)
    worst = {}
    for net, nm in ((m.netG, "G"), (m.netD, "D")):
        d32, d64, n32, n64 = (g[pre + nm + "_gdot"], g[pre64 + nm + "_gdot"], g[pre + nm + "_gnorm"],
                              g[pre64 + nm + "_gnorm"])
        sv, sd = g[spr + nm + "_gvec"], g[spr + nm + "_gdot"]
        assert len(list(net.parameters())) == len(d64)
        for i, (k, p) in enumerate(net.named_parameters()):
            gr = p.grad.detach().double().cpu().flatten()
            pr = probe(gr.numel(), 90000 + i)
            bar = max(2 * abs(d32[i] - d64[i]), 2 * abs(n32[i] - n64[i]), 2e-3 * n64[i], 8 * sv[i], 8 * sd[i]) + 1e-6
            e = max(abs(float(gr @ pr) - d64[i]), abs(float(gr.norm()) - n64[i]))
            worst[nm] = max(worst.get(nm, 0.0), e / bar)
            assert e <= bar, (nm, k, e, bar, d64[i], n64[i])
    report.append("worst grad error / bar: " + ", ".join("%s %.2f" % kv for kv in sorted(worst.items())))
    # the Adam update of every G tensor (the PReLU slopes are parameters of the flat buffer like any other)
    gspec = unet_spec(3, 3, 7, NGF, norm)
    p0 = unet_params(gspec)
    # (a) against the step's own gradient: a first Adam step is -lr g / (|g| + eps), for every tensor;
    # (b) its probe dot against the reference's, within the stored margins (the rule tests/test_step256_gpu.py
    # reports: 3x the reference's own fp32 error, 8x its 1-ulp spread, 1e-3 relative) plus what the elements
    # whose step is not determined may add: lr * sign(g) steps either way where |g| is ~0 at fp32 resolution,
    # i.e. |g| <= 1e-6 or <= 16x the tensor's RMS gradient error (test_step256_gpu.py's rule, the error taken
    # from the reference's 1-ulp spread of the gradient vector); such an element moves the dot by <= 2 lr |probe|.
    u32, u64, su, sv = g[pre + "G_upd"], g[pre64 + "G_upd"], g[spr + "G_upd"], g[spr + "G_gvec"]
    lr, eps = float(m.opt.lr), 1e-8
    worst_u = 0.0
    for i, (k, p) in enumerate(m.netG.named_parameters()):
        d = (p.detach().double().cpu() - p0[k].double()).flatten()
        gr = p.grad.detach().double().cpu().flatten()
        assert (d + lr * gr / (gr.abs() + eps)).abs().max() <= 1e-3 * lr + 2.0 ** -23 * float(p0[k].abs().max()), ("adam", k)
        pr = probe(d.numel(), 90000 + i)
        loose = gr.abs() <= max(1e-6, 16 * sv[i] / np.sqrt(d.numel()))
        bar = max(3 * abs(u32[i] - u64[i]), 8 * su[i], 1e-3 * abs(u64[i])) + 1e-7 + 2 * lr * float(pr[loose].abs().sum())
        e = abs(float(d @ pr) - u64[i])
        worst_u = max(worst_u, e / bar)
        assert e <= bar, ("upd", k, e, bar, int(loose.sum()), d.numel())
    report.append("worst G update error / bar %.2f" % worst_u)
    rm, rv, nbt = _g_buffers(m)
    if norm == "batch":
        e_rm, e_rv = _rel(rm, torch.from_numpy(g[pre64 + "G_rm"])), _rel(rv, torch.from_numpy(g[pre64 + "G_rv"]))
        report.append("G running_mean %.2e running_var %.2e counters %s" % (e_rm, e_rv, sorted(set(nbt))))
        assert e_rm <= 1e-5 and e_rv <= 1e-5
        assert nbt == [1] * len(nbt) == list(g[pre64 + "G_nbt"]) and len(nbt) == 11
    else:
        assert nbt == []
    print("\n[unet_128 --norm %s 128^2 fp32 step] " % norm + "; ".join(report))


def test_dropout_graph_steps_equal_eager_steps():
    runs = []
    for graph in (0, 1):
        m = _model("batch", "bf16", dropout=True)
        m.cuda_graph = bool(graph)
        blocks = m.netG.dropout_blocks()
        assert len(blocks) == 2 and [b.drop_seed for b in blocks] == [20, 20]
        rec = []
        for it in range(3):
            _set(m, 300 + it)
            m.optimize_parameters()
            torch.cuda.synchronize()
            assert [int(b.drop_counter) for b in blocks] == [it + 1] * 2
            rec.append((m.fake_B.detach().clone(), m.flatG.data.clone(), m.flatD.data.clone()))
        runs.append((rec, bool(m._graphs)))
        assert m.nonfinite_report() == {"G": (0, 3), "D": (0, 3)}
    (eager, cap_e), (graph, cap_g) = runs
    assert not cap_e and cap_g
    for te, tg in zip(eager, graph):
        for a, b in zip(te, tg):
            assert torch.isfinite(a).all() and torch.equal(a, b)
    assert not torch.equal(eager[0][0], eager[1][0])


def test_checkpoint_round_trip_and_test_model(tmp_path):
    m = _model("batch", dropout=True, checkpoints_dir=str(tmp_path), name="ck")
    _set(m, 51)
    m.optimize_parameters()
    torch.cuda.synchronize()
    want = OrderedDict((k, v.detach().cpu().clone()) for k, v in m.netG.state_dict().items())
    assert [k for k, _ in unet_spec(3, 3, 7, NGF, "batch", True)] == list(want) == list(G7["K7_batch_1_keys"])
    m.save_networks("7")
    path = os.path.join(str(tmp_path), "ck", "7_useSE_net_G.pth")
    assert list(torch.load(path, map_location="cpu", weights_only=True).keys()) == list(want)
    with torch.no_grad():
        for v in m.netG.state_dict().values():
            v.zero_()
    m.load_networks("7")
    for k, v in m.netG.state_dict().items():
        assert v.dtype == want[k].dtype and torch.equal(v.cpu(), want[k]), k
    # --model test: the same generator from the saved file, eval mode (dropout the identity, running statistics)
    from options.test_options import default_test_opt
    from models import create_model
    topt = default_test_opt(gpu_ids=[0], precision="fp32", checkpoints_dir=str(tmp_path), name="ck", which_epoch="7",
                            norm="batch", which_model_netG="unet_128", ngf=NGF, no_dropout=False)
    t = create_model(topt)
    assert type(t).__name__ == "TestModel"
    t.setup(topt)
    t.eval()
    A, _ = synth_pair(BATCH, SIZE, seed=51)
    m.netG.eval()
    with torch.no_grad():
        ref = m.netG(A.cuda()).clone()
    t.set_input({"A": A, "A_paths": ["a"] * BATCH})
    t.test()
    torch.cuda.synchronize()
    out = t.fake_B.detach().clone()
    assert tuple(out.shape) == (BATCH, 3, SIZE, SIZE) and torch.isfinite(out).all() and float(out.abs().max()) <= 1.0
    assert torch.equal(out, ref)
    t.test()
    assert torch.equal(out, t.fake_B)      # eval mode: no mask drawn, the running statistics left alone
    assert all(int(b.drop_counter) == 0 for b in t.netG.dropout_blocks())
    assert all(int(v) == 1 for k, v in t.netG.state_dict().items() if k.endswith("num_batches_tracked"))
