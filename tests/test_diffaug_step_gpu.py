"""--diffaug in the train step: off it is absent; on, the three D passes of one optimize_parameters draw calls
k, k+1, k+2 of one counter-based stream -- the stacked backward_D equals the two-pass form, a replayed graph
equals the eager step, the G step's gradient flows back through the transform, a resumed run continues bit
for bit, and every discriminator / objective / conditioning variant takes it.

The 64x64, batch-2 model recipe of tests/test_resume_gpu.py."""
import os
import random
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from bn_fixture import d_params_bn  # noqa: E402
from oracle import dsgan_cpu as O  # noqa: E402
from oracle.recipe import make_params, synth_pair  # noqa: E402
from dsgan_hip import diffaug as DA  # noqa: E402

pytestmark = pytest.mark.gpu

FULL = "color,translation,cutout"
SIZE, BATCH = 64, 2
# per-tensor relative bars of the D weight-grads, stacked vs two-pass: tests/test_dbatch_gpu.py's
REL = {"fp32": 2e-6, "bf16": 5e-4, "fp16": 5e-4}
IN_BIAS = ("model.2.bias", "model.5.bias", "model.8.bias")   # conv biases ahead of an InstanceNorm
PARITY = 1e-3   # README: the fp32 parity criterion


def _model(prec="fp32", seed=20, init=True, pool_size=0, **kw):
    import dsgan_hip
    from options.train_options import default_train_opt
    from models import create_model
    dsgan_hip.require_gpu()
    random.seed(seed)
    np.random.seed(seed)
    torch.manual_seed(seed)
    m = create_model(default_train_opt(gpu_ids=[0], pool_size=pool_size, precision=prec, batchSize=BATCH, **kw))
    nets = [(m.vgg, make_params(O.vgg_param_spec(True), "vgg", 7000))]
    if init:
        dspec = [(k, tuple(v.shape)) for k, v in m.netD.state_dict().items()]
        dp = d_params_bn(dspec) if kw.get("norm") == "batch" else make_params(dspec, "fanin", 5000)
        nets += [(m.netG, make_params(O.g_param_spec(), "fanin", 1000)), (m.netD, dp)]
    with torch.no_grad():
        for net, pr in nets:
            for k, v in net.state_dict().items():
                v.copy_(pr[k])
    return m


def _set(m, seed):
    A, B = synth_pair(BATCH, SIZE, seed=seed)
    m.set_input({"A": A.cuda(), "B": B.cuda(), "A_paths": ["a"] * BATCH, "B_paths": ["b"] * BATCH})


def _rel(a, b):
    a, b = a.double(), b.double()
    return ((a - b).norm() / max(b.norm().item(), 1e-30)).item()


def test_flag_off_leaves_no_trace():
    m = _model()
    assert m.diffaug is None and m.diffaug_policy == ()
    _set(m, 51)
    m.optimize_parameters()
    assert "diffaug" not in m.train_state_dict()


def test_stacked_d_equals_two_pass():
    m = _model(diffaug=FULL)
    assert m.diffaug is not None and m.diffaug.seed == 20 and m.diffaug.stream == 0xFFFF and m.d_batch
    _set(m, 51)
    m.forward()
    res = {}
    for form in (False, True):
        m.d_batch = form
        m.diffaug.counter.zero_()
        m.set_requires_grad(m.netD, True)
        m.optimizer_D.zero_grad()
        m.backward_D()
        torch.cuda.synchronize()
        assert int(m.diffaug.counter.item()) == 2
        res[form] = dict(pf=m.pred_fake.detach().clone(), pr=m.pred_real.detach().clone(),
                         L=(m.loss_D_fake.item(), m.loss_D_real.item(), m.loss_D.item()),
                         g={k: p.grad.detach().clone() for k, p in m.netD.named_parameters()})
    two, st = res[False], res[True]
    assert torch.equal(st["pf"], two["pf"]) and torch.equal(st["pr"], two["pr"])
    assert st["L"] == two["L"]
    msg = []
    for k, g2 in two["g"].items():
        gs = st["g"][k]
        assert torch.isfinite(gs).all(), k
        if k in IN_BIAS:
            gw = two["g"][k.replace("bias", "weight")].double().norm().item()
            ok = (gs.double() - g2.double()).norm().item() <= 2e-6 * gw
        else:
            ok = _rel(gs, g2) <= REL["fp32"]
        msg.append("%s %.2e" % (k, _rel(gs, g2)))
        assert ok, (k, msg)
    print("stacked vs two-pass under --diffaug: %s" % ", ".join(msg))
    # the D really saw another input: the un-augmented logits differ
    m.diffaug, keep = None, m.diffaug
    m.backward_D()
    assert not torch.equal(m.pred_real, two["pr"])
    m.diffaug = keep


def test_graph_steps_equal_eager_steps():
    runs = []
    for graph in (0, 1):
        m = _model("bf16", diffaug=FULL)
        m.cuda_graph = bool(graph)
        rec = []
        for it in range(3):
            _set(m, 300 + it)
            m.optimize_parameters()
            torch.cuda.synchronize()
            assert int(m.diffaug.counter.item()) == 3 * (it + 1)
            rec.append((m.fake_B.detach().clone(), m.flatG.data.clone(), m.flatD.data.clone()))
        runs.append((rec, bool(m._graphs)))
        assert m.nonfinite_report() == {"G": (0, 3), "D": (0, 3)}
    (eager, cap_e), (graph, cap_g) = runs
    assert not cap_e and cap_g
    for te, tg in zip(eager, graph):
        for a, b in zip(te, tg):
            assert torch.isfinite(a).all() and torch.equal(a, b)
    assert not torch.equal(eager[0][0], eager[1][0]) and not torch.equal(eager[1][2], eager[2][2])


def test_g_step_differentiates_through_the_op():
    """One backward_G, fp32, full policy: the gradient the op hands to fake_B equals torch autograd through
    augment_reference (float64) chained on the D-input gradient the HIP path produced."""
    from dsgan_hip import functional as HF
    m = _model(diffaug=FULL)
    _set(m, 51)
    m._launch_real_features()
    m.forward()
    m.set_requires_grad(m.netD, False)
    m.optimizer_G.zero_grad()
    m.diffaug.counter.fill_(11)
    rec, orig = {}, HF.diffaug_cat

    def spy(a, b, policy, state, group=None, out=None):
        rec["k"], rec["a"], rec["b"] = int(state.counter.item()), a.detach().clone(), b.detach().clone()
        b2 = b.view_as(b)   # what reaches b2 is this op's gradient alone (fake_B's own sums the image losses')
        b2.register_hook(lambda g: rec.__setitem__("gb", g.detach().clone()))
        y = orig(a, b2, policy, state, group, out)
        y.register_hook(lambda g: rec.__setitem__("gy", g.detach().clone()))
        return y

    HF.diffaug_cat = spy
    try:
        m.backward_G()
    finally:
        HF.diffaug_cat = orig
    torch.cuda.synchronize()
    assert rec["k"] == 11 and int(m.diffaug.counter.item()) == 12
    assert torch.equal(rec["b"], m.fake_B.detach()) and torch.equal(rec["a"], m.real_A)
    gy, gb = rec["gy"].cpu().double(), rec["gb"].cpu().double()
    assert gy.abs().max() > 0 and gy.shape[1] == 6 and gb.shape[1] == 3
    p = DA.draw_params(m.diffaug.seed, m.diffaug.stream, 11, BATCH, SIZE, SIZE)
    xb = rec["b"].cpu().double().requires_grad_(True)
    y = DA.augment_reference(torch.cat([rec["a"].cpu().double(), xb], 1), 3, FULL, p)
    (want,) = torch.autograd.grad(y, xb, gy)
    err = ((gb - want).abs().max() / want.abs().max()).item()
    print("G step through diffaug: max rel err of the fake_B gradient %.3g" % err)
    assert err <= PARITY
    # and it arrived: the generator's gradient with the op differs from the one without it
    g_on = m.flatG.grad.clone()
    m.optimizer_G.zero_grad()
    m.diffaug, keep = None, m.diffaug
    m._launch_real_features()
    m.forward()   # (the first backward freed the generator's graph)
    m.backward_G()
    m.diffaug = keep
    assert torch.isfinite(g_on).all() and not torch.equal(g_on, m.flatG.grad)


def _snap(m):
    torch.cuda.synchronize()
    out = {"G": m.flatG.data, "D": m.flatD.data, "G.m": m.optimizer_G.m, "G.v": m.optimizer_G.v,
           "D.m": m.optimizer_D.m, "D.v": m.optimizer_D.v, "pool": m.fake_AB_pool.store[:m.fake_AB_pool.num_imgs],
           "fake_B": m.fake_B, "aug": m.diffaug.counter}
    for k, sc in (("scaler_G", m.scaler_G), ("scaler_D", m.scaler_D)):
        if sc is not None:
            out[k] = sc.state
    out = {k: v.detach().clone() for k, v in out.items()}
    out["py"], out["calls"] = random.getstate(), dict(m.step_calls)
    return out


def _same(a, b):
    assert sorted(a) == sorted(b)
    return [k for k in a if not (torch.equal(a[k], b[k]) if torch.is_tensor(a[k]) else a[k] == b[k])]


def _interrupted(prec, ckpt, first, second, **kw):
    """``first`` steps, save, drop the model, reseed, a fresh model, load, ``second`` more steps."""
    m = _model(prec, checkpoints_dir=str(ckpt), name="exp", **kw)
    for it in range(first):
        _set(m, 700 + it)
        m.optimize_parameters()
    m.save_networks("3")
    m.save_train_state("3")
    del m
    m = _model(prec, seed=77, init=False, checkpoints_dir=str(ckpt), name="exp", **kw)
    ctr = m.diffaug.counter.data_ptr()
    m.load_networks("3")
    m.load_train_state("3")
    assert m.diffaug.counter.data_ptr() == ctr and int(m.diffaug.counter.item()) == 3 * first   # restored in place
    for it in range(first, first + second):
        _set(m, 700 + it)
        m.optimize_parameters()
    return m


def test_resume_is_bitwise(tmp_path):
    kw = dict(pool_size=3, diffaug=FULL)
    a = _model("bf16", checkpoints_dir=str(tmp_path / "a"), name="exp", **kw)
    for it in range(4):
        _set(a, 700 + it)
        a.optimize_parameters()
    A = _snap(a)
    assert int(A["aug"].item()) == 12 and bool(a._graphs)
    del a
    b = _interrupted("bf16", tmp_path / "b", 2, 2, **kw)
    assert _same(A, _snap(b)) == []
    sd = torch.load(str(tmp_path / "b" / "exp" / "3_train_state.pth"), map_location="cpu", weights_only=True)
    assert sd["diffaug"] == {"counter": 6, "seed": 20, "stream": 0xFFFF, "policy": FULL}
    # a state saved with another policy -- or with none, or loaded into a run with none -- is refused by name
    for other, pat in (("cutout", "color,translation,cutout.*'cutout'"), ("", "color,translation,cutout.*''")):
        c = _model("bf16", seed=77, init=False, checkpoints_dir=str(tmp_path / "b"), name="exp", pool_size=3, diffaug=other)
        c.load_networks("3")
        with pytest.raises(RuntimeError, match=pat):
            c.load_train_state("3")
    c.save_train_state("4")   # the flag-off state ...
    with pytest.raises(RuntimeError, match="''.*color,translation,cutout"):
        b.load_train_state("4")   # ... into the flag-on run


@pytest.mark.parametrize("kw", [dict(which_model_netD="pixel", no_lsgan=True), dict(which_model_netD="multi", no_lsgan=True),
                                dict(which_model_netD="basic", norm="batch"), dict(use_condition=0),
                                dict(precision="fp16")],
                         ids=["pixel", "multi", "batchnorm", "uncond", "fp16"])
def test_variants_take_it(kw):
    kw = dict(kw)
    m = _model(kw.pop("precision", "fp32"), diffaug=FULL, **kw)
    _set(m, 51)
    m.optimize_parameters()
    torch.cuda.synchronize()
    assert int(m.diffaug.counter.item()) == 3
    for v in (m.loss_D_fake, m.loss_D_real, m.loss_G_GAN, m.loss_G):
        assert np.isfinite(float(v.detach()))
    assert torch.isfinite(m.flatG.data).all() and torch.isfinite(m.flatD.data).all()
    assert torch.isfinite(m.flatG.grad).all() and m.flatD.grad.abs().max() > 0
