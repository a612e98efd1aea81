"""The train step with ``--norm batch`` (the ``basic`` D on BatchNorm2d), at 64x64, batch 2, pool_size 0
(DSGAN/models/pix2pix_model.py:141-217):

  * one fp32 ``optimize_parameters``, with BCE and with ``--no_lsgan``, against the reference's own
    step (tests/golden/golden_v6.npz, gen_golden_v6.py) under the bar rules of
    tests/test_step256_gpu.py: the nine losses 1e-3 relative against its fp32 and its fp64 step;
    fake_B max(1e-3, 3x the reference's own fp32 error, 8x its 1-ulp spread); gradients per tensor
    |g - g64| <= max(2 |g32_ref - g64_ref|, 2e-3 |g64|, 8x the 1-ulp spread) + 1e-6 on the norm and
    the probe dot; the D's running buffers after the step 1e-5 against the reference's fp64 step,
    every counter == 3 (fake pass, real pass, the G step's pass).  The fixture's input seed is one
    for which the reference's own fp64 step has no BatchNorm pre-activation within 1e-5 of zero
    (gen_golden_v6.py Z_MIN, ``S6_*_f64_zmin``): such an element's LeakyReLU sign lies inside the fp32
    rounding of the conv in front of it, and one flipped sign moves a BatchNorm bias gradient by
    ~1e-2 of its norm (seed 43, with two such elements in the fake pass: model.3.bias 1.1e-2 off,
    every BatchNorm launch itself <= 1.3e-7 against fp64 on its own inputs);
  * ``d_batch`` True and False: the same bits for predictions, losses, D gradients and buffers --
    the stacked batch-2N pass is never taken under batch statistics;
  * the two-graph step against the eager step over three steps, and two identical eager runs: the
    same bits for losses, flat gradients, flat parameters and the running buffers; counters == 9;
  * bf16 / fp16: three finite steps with no skipped optimizer step, and the D's 16-bit-mode output
    error against its fp32-mode output at most 4x the error the unchanged instance-norm ``basic`` D
    shows in the same comparison at the same shape (the unchanged D is the yardstick; 4 is the factor
    tests/test_lsgan_step_gpu.py uses for the same comparison);
  * a checkpoint round-trips running_mean / running_var / num_batches_tracked bitwise through
    save_networks / load_networks, also from a ``module.``-prefixed file.
"""
import os
import random
import sys
from collections import OrderedDict

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from bn_fixture import d_params_bn, bn_indices  # noqa: E402
from oracle import dsgan_cpu as O  # noqa: E402
from oracle.recipe import make_params, synth_pair, probe  # noqa: E402

pytestmark = pytest.mark.gpu

G6 = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "golden_v6.npz"))
NAMES = ["G_GAN", "G_L1", "D_real", "D_fake", "vgg", "tv", "ssim", "G", "D"]
SIZE, BATCH = 64, 2


def _model(prec="fp32", lsgan=False, norm="batch", **kw):
    import dsgan_hip
    from options.train_options import default_train_opt
    from models import create_model
    dsgan_hip.require_gpu()
    random.seed(20)
    torch.manual_seed(20)
    m = create_model(default_train_opt(gpu_ids=[0], pool_size=0, precision=prec, batchSize=BATCH, no_lsgan=lsgan,
                                       which_model_netD="basic", norm=norm, **kw))
    dspec = [(k, tuple(v.shape)) for k, v in m.netD.state_dict().items()]
    dp = d_params_bn(dspec) if norm == "batch" else make_params(dspec, "fanin", 5000)
    with torch.no_grad():
        for net, pr in ((m.netG, make_params(O.g_param_spec(), "fanin", 1000)), (m.netD, dp),
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


def _bns(m):
    return [mod for mod in m.netD.modules() if isinstance(mod, torch.nn.BatchNorm2d)]


def _buffers(m):
    bns = _bns(m)
    return (torch.cat([b.running_mean for b in bns]).clone(), torch.cat([b.running_var for b in bns]).clone(),
            [int(b.num_batches_tracked) for b in bns])


def _rel(a, b):
    a, b = a.double().cpu(), b.double().cpu()
    return ((a - b).norm() / max(b.norm().item(), 1e-30)).item()


@pytest.mark.parametrize("name,lsgan", [("bce", False), ("ls", True)])
def test_batchnorm_step_fp32_vs_reference(name, lsgan):
    g = G6
    pre, pre64, spr = "S6_%s_f32_" % name, "S6_%s_f64_" % name, "S6_%s_spread_" % name
    m = _model(lsgan=lsgan)
    assert m.d_batch_stats and len(_bns(m)) == 3
    _set(m, int(g["S6_%s_input_seed" % name]))
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
    rm, rv, nbt = _buffers(m)
    e_rm, e_rv = _rel(rm, torch.from_numpy(g[pre64 + "D_rm"])), _rel(rv, torch.from_numpy(g[pre64 + "D_rv"]))
    report.append("running_mean %.2e running_var %.2e counters %s" % (e_rm, e_rv, nbt))
    print("\n[--norm batch %s 64^2 fp32 step] " % name + "; ".join(report))
    assert e_rm <= 1e-5 and e_rv <= 1e-5
    assert nbt == [3, 3, 3] == list(g[pre64 + "D_nbt"])


@pytest.mark.parametrize("prec", ["fp32", "bf16"])
def test_stacked_flag_changes_nothing(prec):
    m = _model(prec)
    _set(m, 51)
    m.forward()
    state0 = OrderedDict((k, v.clone()) for k, v in m.netD.state_dict().items())
    s0 = m.scaler_D.state.clone() if m.scaler_D is not None else None
    calls = []
    fwd = m.netD.forward
    m.netD.forward = lambda x: (calls.append(int(x.shape[0])), fwd(x))[1]
    res = {}
    for form in (False, True):
        with torch.no_grad():
            for k, v in m.netD.state_dict().items():
                v.copy_(state0[k])
        m.d_batch = form
        m.set_requires_grad(m.netD, True)
        m.optimizer_D.zero_grad()
        m.backward_D()
        if m.scaler_D is not None:
            m.scaler_D.check(m.flatD.grad)
            assert m.scaler_D.state[1].item() == 0.0
            m.scaler_D.state.copy_(s0)
        torch.cuda.synchronize()
        res[form] = [m.pred_fake.detach().clone(), m.pred_real.detach().clone(),
                     torch.stack([m.loss_D_fake.detach(), m.loss_D_real.detach(), m.loss_D.detach()]).clone(),
                     m.flatD.grad.clone()] + list(_buffers(m)[:2])
        assert _buffers(m)[2] == [2, 2, 2]
    assert calls == [BATCH] * 4   # two passes of the plain batch each time, never the stacked 2N
    for a, b in zip(res[False], res[True]):
        assert torch.isfinite(a).all() and torch.equal(a, b)


def test_graph_step_equals_eager_and_steps_repeat():
    """bf16 with the non-finite guard (device-side step counts), the mode of
    tests/test_model_gpu.py::test_graph_step_equals_eager: the step replayed from its two captured
    graphs (captured in step 2) gives the eager step's bits after two steps and after a third (a replay
    of the kept pair), running buffers and counters included; two eager runs agree too."""
    runs = []
    for graph in (0, 1, 0):
        m = _model("bf16")
        m.cuda_graph = bool(graph)
        rec = []
        for it in range(3):
            _set(m, 300 + it)
            m.optimize_parameters()
            if it >= 1:
                torch.cuda.synchronize()
                rm, rv, nbt = _buffers(m)
                assert nbt == [3 * (it + 1)] * 3
                rec.append((_losses(m), m.flatG.grad.clone(), m.flatD.grad.clone(), m.flatG.data.clone(),
                            m.flatD.data.clone(), rm, rv))
        runs.append((rec, bool(m._graphs)))
        assert m.nonfinite_report() == {"G": (0, 3), "D": (0, 3)}
        assert _buffers(m)[2] == [9, 9, 9]
    (eager, cap_e), (graph, cap_g), (again, _) = runs
    assert not cap_e and cap_g
    for other in (graph, again):
        for (le, *te), (lo, *to) in zip(eager, other):
            assert le == lo and all(np.isfinite(le))
            for a, b in zip(te, to):
                assert torch.equal(a, b)


@pytest.mark.parametrize("prec", ["bf16", "fp16"])
def test_16bit_steps_finite_and_output_error(prec):
    """Measured ratio (batch-norm D error / instance-norm D error) is printed; the bar is 4."""
    m = _model(prec)
    for it in range(3):
        _set(m, 400 + it)
        m.optimize_parameters()
        assert all(np.isfinite(_losses(m))), (it, _losses(m))
    torch.cuda.synchronize()
    assert m.nonfinite_report() == {"G": (0, 3), "D": (0, 3)}
    assert _buffers(m)[2] == [9, 9, 9]
    del m
    torch.cuda.empty_cache()
    from dsgan_hip import functional as HF
    A, B = synth_pair(BATCH, SIZE, seed=51)
    x = torch.cat((A, B), 1).cuda()
    errs = {}
    for norm in ("batch", "instance"):
        outs = {}
        for p in ("fp32", prec):
            md = _model(p, norm=norm)
            with torch.no_grad(), HF.precision(p):
                outs[p] = md.netD(x).clone()
            del md
        errs[norm] = _rel(outs[prec], outs["fp32"])
    print("\n[%s] D output vs fp32 mode: batch norm %.3e, unchanged instance norm %.3e, ratio %.2f"
          % (prec, errs["batch"], errs["instance"], errs["batch"] / errs["instance"]))
    assert errs["batch"] <= 4 * errs["instance"], errs


def test_checkpoint_round_trip(tmp_path):
    m = _model(checkpoints_dir=str(tmp_path), name="ck")
    _set(m, 51)
    m.optimize_parameters()   # counters 3, buffers away from the recipe's
    torch.cuda.synchronize()
    want = OrderedDict((k, v.detach().cpu().clone()) for k, v in m.netD.state_dict().items())
    assert sum(k.endswith("num_batches_tracked") for k in want) == 3
    assert all(int(want["model.%d.num_batches_tracked" % i]) == 3 for i in (3, 6, 9))
    m.save_networks("7")
    path = os.path.join(str(tmp_path), "ck", "7_useSE_net_D.pth")
    assert list(torch.load(path, map_location="cpu", weights_only=True).keys()) == list(want)
    for prefixed in (False, True):
        if prefixed:   # a reference-style DataParallel checkpoint
            for n in ("G", "D"):
                f = os.path.join(str(tmp_path), "ck", "7_useSE_net_%s.pth" % n)
                sd = torch.load(f, map_location="cpu", weights_only=True)
                torch.save(OrderedDict(("module." + k, v) for k, v in sd.items()), f)
        with torch.no_grad():
            for v in m.netD.state_dict().values():
                v.zero_()
        m.load_networks("7")
        for k, v in m.netD.state_dict().items():
            assert v.dtype == want[k].dtype and torch.equal(v.cpu(), want[k]), (prefixed, k)
