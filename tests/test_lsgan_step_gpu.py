"""The train step with ``--no_lsgan`` (sigmoid + least squares, quirk q3) on the ``basic`` and the
``multi`` discriminator, at 64x64, batch 2, pool_size 0 (DSGAN/models/pix2pix_model.py:141-217):

  * one fp32 ``optimize_parameters`` against the reference's own step (tests/golden/golden_v5.npz,
    gen_golden_v5.py) under the bar rules of tests/test_step256_gpu.py: the nine losses 1e-3
    relative against its fp32 and its fp64 step; fake_B max(1e-3, 3x the reference's own fp32 error,
    8x its 1-ulp spread); gradients per tensor |g - g64| <= max(2 |g32_ref - g64_ref|, 2e-3 |g64|,
    8x the 1-ulp spread) + 1e-6 on the norm and the probe dot;
  * backward_D's stacked batch-2N pass against two passes: every scale's predictions and the three D
    losses the same bits, the D gradients within tests/test_dbatch_gpu.py's REL of the mode.  On the
    fan-in recipe, like every test here (oracle/recipe.py: the regime where fp32 gradients are
    meaningful).  On the N(0, 0.02) recipe every prediction is 0.5 +- 0.01, so the fake and the real
    half of a last conv's one-element bias gradient cancel to ~1/30 of either half, and the relative
    error of that element measures the cancellation: 2.08e-6 for layer1.11.bias in fp32 there, all
    other tensors <= 5.1e-7;
  * the two-graph step against the eager step, and two identical steps: the same bits;
  * bf16 / fp16: three finite steps with no skipped optimizer step, and the multi D's 16-bit output
    error against its fp32-mode output at most 4x the error the unchanged ``basic`` D (BCE, no
    sigmoid) shows in the same comparison at the same shape (the unchanged D is the yardstick; the 4
    allows for the sigmoid's slope and the three pad-2 scales);
  * a ``multi`` checkpoint round-trips through save_networks / load_networks, also ``module.``-prefixed.
"""
import os
import random
from collections import OrderedDict

import numpy as np
import pytest
import torch

from oracle import dsgan_cpu as O
from oracle.recipe import make_params, synth_pair, probe

pytestmark = pytest.mark.gpu

G5 = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "golden_v5.npz"))
NAMES = ["G_GAN", "G_L1", "D_real", "D_fake", "vgg", "tv", "ssim", "G", "D"]
REL = {"fp32": 2e-6, "bf16": 5e-4, "fp16": 5e-4}   # tests/test_dbatch_gpu.py
SIZE, BATCH = 64, 2


def _in_bias(k):   # conv biases ahead of an InstanceNorm: analytic gradient 0
    return k.endswith((".2.bias", ".5.bias", ".8.bias"))


def _model(kind, prec="fp32", lsgan=True, recipe="fanin", **kw):
    import dsgan_hip
    from options.train_options import default_train_opt
    from models import create_model
    dsgan_hip.require_gpu()
    random.seed(20)
    torch.manual_seed(20)
    m = create_model(default_train_opt(gpu_ids=[0], pool_size=0, precision=prec, batchSize=BATCH, no_lsgan=lsgan,
                                       which_model_netD=kind, **kw))
    dspec = [(k, tuple(v.shape)) for k, v in m.netD.state_dict().items()]
    with torch.no_grad():
        for net, pr in ((m.netG, make_params(O.g_param_spec(), recipe, 1000)),
                        (m.netD, make_params(dspec, recipe, 5000)),
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


def _flat_preds(p):
    return [t for s in p for t in s] if isinstance(p, list) else [p]


def _rel(a, b):
    a, b = a.double(), b.double()
    return ((a - b).norm() / max(b.norm().item(), 1e-30)).item()


@pytest.mark.parametrize("kind", ["basic", "multi"])
def test_lsgan_step_fp32_vs_reference(kind):
    g = G5
    pre, pre64, spr = "S5_%s_f32_" % kind, "S5_%s_f64_" % kind, "S5_%s_spread_" % kind
    m = _model(kind)
    _set(m, int(g["S5_input_seed"]))
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
    print("\n[--no_lsgan %s 64^2 fp32 step] " % kind + "; ".join(report))


@pytest.mark.parametrize("prec", ["fp32", "bf16", "fp16"])
@pytest.mark.parametrize("kind", ["basic", "multi"])
def test_stacked_d_equals_two_pass(kind, prec):
    m = _model(kind, prec)
    _set(m, 51)
    m.forward()
    s0 = m.scaler_D.state.clone() if m.scaler_D is not None else None
    res = {}
    for form in (False, True):
        m.d_batch = form
        m.set_requires_grad(m.netD, True)
        m.optimizer_D.zero_grad()
        m.backward_D()
        if m.scaler_D is not None:
            m.scaler_D.check(m.flatD.grad)
        torch.cuda.synchronize()
        assert isinstance(m.pred_fake, list) == (kind == "multi") and isinstance(m.pred_real, list) == (kind == "multi")
        res[form] = dict(pf=[t.detach().clone() for t in _flat_preds(m.pred_fake)],
                         pr=[t.detach().clone() for t in _flat_preds(m.pred_real)],
                         L=(m.loss_D_fake.item(), m.loss_D_real.item(), m.loss_D.item()),
                         g={k: p.grad.detach().clone() for k, p in m.netD.named_parameters()})
        if s0 is not None:
            assert m.scaler_D.state[1].item() == 0.0   # no skipped step
            m.scaler_D.state.copy_(s0)
    two, st = res[False], res[True]
    assert len(st["pf"]) == (3 if kind == "multi" else 1)
    for a, b in zip(st["pf"] + st["pr"], two["pf"] + two["pr"]):
        assert a.shape[0] == BATCH and torch.equal(a, b)
    assert st["L"] == two["L"]
    print("\n[%s %s stacked vs two-pass] %s" % (kind, prec, ", ".join(
        "%s %.2e" % (k, _rel(st["g"][k], g2)) for k, g2 in two["g"].items())))
    for k, g2 in two["g"].items():
        gs = st["g"][k]
        assert torch.isfinite(gs).all(), k
        if _in_bias(k):
            gw = two["g"][k.replace("bias", "weight")].double().norm().item()
            assert (gs.double() - g2.double()).norm().item() <= 2e-6 * gw, k
        else:
            assert _rel(gs, g2) <= REL[prec], (k, _rel(gs, g2))


@pytest.mark.parametrize("kind", ["basic", "multi"])
def test_graph_step_equals_eager_and_steps_repeat(kind):
    """bf16 with the non-finite guard (device-side step counts), the mode of
    tests/test_model_gpu.py::test_graph_step_equals_eager: the step replayed from its two captured
    graphs (captured in step 2) gives the eager step's bits -- losses, flat gradients and flat parameters
    of both networks after two steps and after a third (a replay of the kept pair); two eager runs of
    the same steps give the same bits too."""
    runs = []
    for graph in (0, 1, 0):
        m = _model(kind, "bf16")
        m.cuda_graph = bool(graph)
        rec = []
        for it in range(3):
            _set(m, 300 + it)
            m.optimize_parameters()
            if it >= 1:
                torch.cuda.synchronize()
                rec.append((_losses(m), m.flatG.grad.clone(), m.flatD.grad.clone(), m.flatG.data.clone(),
                            m.flatD.data.clone()))
        runs.append((rec, bool(m._graphs)))
        assert m.nonfinite_report() == {"G": (0, 3), "D": (0, 3)}
    (eager, cap_e), (graph, cap_g), (again, _) = runs
    assert not cap_e and cap_g
    for other in (graph, again):
        for (le, *te), (lo, *to) in zip(eager, other):
            assert le == lo and all(np.isfinite(le))
            for a, b in zip(te, to):
                assert torch.equal(a, b)


@pytest.mark.parametrize("prec", ["bf16", "fp16"])
def test_multi_16bit_steps_finite_and_output_error(prec):
    m = _model("multi", prec)
    for it in range(3):
        _set(m, 400 + it)
        m.optimize_parameters()
        assert all(np.isfinite(_losses(m))), (it, _losses(m))
    torch.cuda.synchronize()
    assert m.nonfinite_report() == {"G": (0, 3), "D": (0, 3)}
    del m
    torch.cuda.empty_cache()
    # the D's output in this mode against its fp32-mode output on the same weights and input
    from dsgan_hip import functional as HF
    A, B = synth_pair(BATCH, SIZE, seed=51)
    x = torch.cat((A, B), 1).cuda()
    errs = {}
    for kind, lsgan in (("multi", True), ("basic", False)):
        outs = {}
        for p in ("fp32", prec):
            md = _model(kind, p, lsgan=lsgan)
            with torch.no_grad(), HF.precision(p):
                outs[p] = [t.clone() for t in _flat_preds(md.netD(x))]
            del md
        errs[kind] = max(_rel(a, b) for a, b in zip(outs[prec], outs["fp32"]))
    print("\n[%s] D output vs fp32 mode: multi (sigmoid, 3 scales) %.3e, unchanged basic (logits) %.3e"
          % (prec, errs["multi"], errs["basic"]))
    assert errs["multi"] <= 4 * errs["basic"], errs


def test_multi_checkpoint_round_trip(tmp_path):
    m = _model("multi", checkpoints_dir=str(tmp_path), name="ck")
    want = OrderedDict((k, v.detach().cpu().clone()) for k, v in m.netD.state_dict().items())
    assert list(want) == ["layer%d.%d.%s" % (s, i, p) for s in range(3) for i in (0, 2, 5, 8, 11)
                          for p in ("weight", "bias")]
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
            assert torch.equal(v.cpu(), want[k]), (prefixed, k)
