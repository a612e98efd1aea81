"""--spectral_norm without a GPU: dsgan_hip.spectral's reference against torch.nn.utils.spectral_norm and
autograd, the power iteration's convergence, the conv holder's state dict against a torch-wrapped twin, the
refusal of a checkpoint of the other kind, and flag off leaving define_D as it was."""
import numpy as np
import pytest
import torch
import torch.nn as nn

from dsgan_hip import spectral as SN

SHAPES = [(32, 6, 4), (1, 8, 4), (3, 5, 1), (64, 32, 4)]   # (Cout, Cin, k)


def _case(cout, cin, k, seed=0):
    g = torch.Generator().manual_seed(100 + seed)
    W = 0.02 * torch.randn(cout, cin, k, k, generator=g, dtype=torch.float64)
    u = torch.randn(cout, generator=g, dtype=torch.float64)
    return W, u / u.norm()


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_reference_is_torch_spectral_norm(shape):
    """One training forward of torch's wrapper from the same (W, u): u, v and the weight to 1e-12."""
    cout, cin, k = shape
    W, u0 = _case(*shape)
    conv = nn.Conv2d(cin, cout, k).double()
    with torch.no_grad():
        conv.weight.copy_(W)
    conv = nn.utils.spectral_norm(conv, n_power_iterations=1, eps=SN.EPS)
    with torch.no_grad():
        conv.weight_u.copy_(u0)
    conv.train()
    conv(torch.zeros(1, cin, 8, 8, dtype=torch.float64))
    w_np, u_np, v_np, s_np = SN.refresh(W.numpy(), u0.numpy())
    w_t, u_t, v_t, s_t = SN.refresh_torch(W, u0)
    for got_u, got_v, got_w in ((torch.from_numpy(u_np), torch.from_numpy(v_np), torch.from_numpy(w_np)), (u_t, v_t, w_t)):
        assert (got_u - conv.weight_u).abs().max() <= 1e-12
        assert (got_v - conv.weight_v).abs().max() <= 1e-12
        assert (got_w - conv.weight.detach()).abs().max() <= 1e-12 * conv.weight.abs().max()
    assert abs(float(s_np) - float(s_t)) <= 1e-12 * abs(float(s_t))
    # iterate=False keeps (u, v) and gives the sigma and W_sn of the call that left them
    w2, u2, v2, s2 = SN.refresh(W.numpy(), u_np, v_np, iterate=False)
    assert np.array_equal(u2, u_np) and np.array_equal(v2, v_np)
    assert np.array_equal(w2, w_np) and s2 == s_np


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_backward_is_autograd(shape):
    W, u0 = _case(*shape, seed=1)
    g = torch.Generator().manual_seed(7)
    G = torch.randn(W.shape, generator=g, dtype=torch.float64)
    Wr = W.clone().requires_grad_(True)
    w_sn, u, v, sigma = SN.refresh_torch(Wr, u0)
    (want,) = torch.autograd.grad((w_sn * G).sum(), Wr)
    got = SN.backward(G.numpy(), w_sn.detach().numpy(), u.numpy(), v.numpy(), float(sigma.detach()))
    assert np.abs(got - want.numpy()).max() <= 1e-12 * want.abs().max().item()


def test_power_iteration_converges_on_a_planted_matrix():
    rng = np.random.default_rng(3)
    a, b = rng.standard_normal(64), rng.standard_normal(512)
    a, b = a / np.linalg.norm(a), b / np.linalg.norm(b)
    M = 4.0 * np.outer(a, b) + 0.02 * rng.standard_normal((64, 512))
    top = np.linalg.svd(M, compute_uv=False)[0]
    u = SN.initial_u(0, 64).double().numpy()
    v, err = None, []
    for _ in range(4):
        _, u, v, sigma = SN.refresh(M, u, v)
        err.append(abs(sigma - top) / top)
    print("planted 64x512: relative error of sigma after 1..4 iterations %s" % ["%.1e" % e for e in err])
    assert err[3] <= 1e-6


def test_initial_u_is_private_and_reproducible():
    torch.manual_seed(5)
    before = torch.get_rng_state().clone()
    a, b, c = SN.initial_u(3, 32), SN.initial_u(3, 32), SN.initial_u(4, 32)
    assert torch.equal(torch.get_rng_state(), before)
    assert torch.equal(a, b) and not torch.equal(a, c)
    assert abs(a.norm().item() - 1.0) <= 1e-6 and a.dtype == torch.float32


def _twin(kind, ndf=8):
    """The architecture define_D(6, ndf, kind, spectral_norm=True) builds, from nn.Conv2d wrapped by torch."""
    sn = lambda *a, **k: nn.utils.spectral_norm(nn.Conv2d(*a, **k), eps=SN.EPS)  # noqa: E731
    if kind == "pixel":
        class T(nn.Module):
            def __init__(self):
                super().__init__()
                self.net = nn.Sequential(sn(6, ndf, 1), nn.LeakyReLU(0.2), sn(ndf, 2 * ndf, 1), nn.Identity(),
                                         nn.LeakyReLU(0.2), sn(2 * ndf, 1, 1))
        return T()

    class T(nn.Module):
        def __init__(self):
            super().__init__()
            self.model = nn.Sequential(
                sn(6, ndf, 4, 2, 1), nn.LeakyReLU(0.2),
                sn(ndf, 2 * ndf, 4, 2, 1), nn.Identity(), nn.LeakyReLU(0.2),
                sn(2 * ndf, 4 * ndf, 4, 2, 1), nn.Identity(), nn.LeakyReLU(0.2),
                sn(4 * ndf, 8 * ndf, 4, 1, 1), nn.Identity(), nn.LeakyReLU(0.2),
                sn(8 * ndf, 1, 4, 1, 1))
    return T()


@pytest.mark.parametrize("kind", ["basic", "pixel"])
def test_state_dict_interop_with_a_torch_wrapped_twin(kind):
    from models.networks import define_D, SNConv2d
    torch.manual_seed(11)
    ours = define_D(6, 8, kind, 3, "instance", False, "normal", [], spectral_norm=True)
    twin = _twin(kind)
    seq_o, seq_t = (ours.net, twin.net) if kind == "pixel" else (ours.model, twin.model)
    assert list(ours.state_dict().keys()) == list(twin.state_dict().keys())
    assert [k for k, _ in ours.named_parameters()] == [k for k, _ in twin.named_parameters()]
    # ours -> torch: strict load; in eval mode torch's wrapper computes W / sigma from the loaded (W, u, v)
    twin.load_state_dict(ours.state_dict(), strict=True)
    twin.eval()
    x = torch.randn(2, 6, 32, 32)
    with torch.no_grad():
        for mo, mt in zip(seq_o, seq_t):
            if isinstance(mo, SNConv2d):
                mt(torch.zeros(1, mo.in_channels, 8, 8))   # the wrapper's pre-forward hook sets .weight
                assert (mo.weight - mt.weight).abs().max() <= 1e-6 * mt.weight.abs().max()
        assert (seq_o(x) - seq_t(x)).abs().max() <= 1e-5
    # torch -> ours: a twin trained elsewhere (other weights, one more power iteration)
    twin.train()
    with torch.no_grad():
        for p in twin.parameters():
            p.add_(0.01 * torch.randn_like(p))
        seq_t(x)
    twin.eval()
    ours.load_state_dict(twin.state_dict(), strict=True)   # (the post-hook recomputes W_sn, iterate=False)
    with torch.no_grad():
        for (k, a), (_, b) in zip(ours.state_dict().items(), twin.state_dict().items()):
            assert torch.equal(a, b), k
        assert (seq_o(x) - seq_t(x)).abs().max() <= 1e-5


def test_checkpoint_of_the_other_kind_is_refused_by_name():
    from models.networks import define_D
    on = define_D(6, 8, "basic", 3, "instance", False, "normal", [], spectral_norm=True).state_dict()
    off = define_D(6, 8, "basic", 3, "instance", False, "normal", []).state_dict()
    SN.check_state_keys(on.keys(), on.keys())
    SN.check_state_keys(off.keys(), off.keys())
    with pytest.raises(RuntimeError, match=r"missing keys \[.*'model\.0\.weight_orig'.*'model\.11\.weight_v'"):
        SN.check_state_keys(on.keys(), off.keys(), "netD")
    with pytest.raises(RuntimeError, match=r"missing keys \['model\.0\.weight', .*'model\.11\.weight'"):
        SN.check_state_keys(off.keys(), on.keys(), "netD")


def test_load_networks_refuses_the_other_kind(tmp_path):
    """BaseModel.load_networks on the CPU, both directions."""
    from models.base_model import BaseModel
    from models.networks import define_D
    for flag in (True, False):
        kw = {"spectral_norm": True} if flag else {}
        src = define_D(6, 8, "basic", 3, "instance", False, "normal", [], **kw)
        d = tmp_path / ("on" if flag else "off")
        d.mkdir()
        torch.save(src.state_dict(), str(d / "3_net_D.pth"))
        m = BaseModel()
        m.save_dir, m.model_names = str(d), ["D"]
        m.netD = define_D(6, 8, "basic", 3, "instance", False, "normal", [], **kw)
        m.load_networks("3")   # its own kind loads
        for k, v in m.netD.state_dict().items():
            assert torch.equal(v, src.state_dict()[k]), k
        if flag:
            for a, b in zip(m.netD.spectral.convs, src.spectral.convs):
                assert torch.equal(a.weight, b.weight)
        m.netD = define_D(6, 8, "basic", 3, "instance", False, "normal", [], **({} if flag else {"spectral_norm": True}))
        with pytest.raises(RuntimeError, match="missing keys.*model.0.weight" + ("'" if flag else "_orig")):
            m.load_networks("3")


@pytest.mark.parametrize("kind,sig", [("basic", False), ("n_layers", False), ("pixel", True), ("multi", True)])
def test_flag_off_leaves_define_D_unchanged(kind, sig):
    from models.networks import define_D, spectral_weights
    torch.manual_seed(20)
    a = define_D(6, 16, kind, 3, "instance", sig, "normal", [])
    torch.manual_seed(20)
    b = define_D(6, 16, kind, 3, "instance", sig, "normal", [], spectral_norm=False)
    assert list(a.state_dict().keys()) == list(b.state_dict().keys())
    assert [k for k, _ in a.named_parameters()] == [k for k, _ in b.named_parameters()]
    assert all(k.endswith((".weight", ".bias")) for k in a.state_dict())
    for (k, x), (_, y) in zip(a.state_dict().items(), b.state_dict().items()):
        assert torch.equal(x, y), k
    assert getattr(a, "spectral", None) is None and spectral_weights(a) == []
    # flag on: the same Sequential indices, torch's names, every conv with a bias, no norm layer
    c = define_D(6, 16, kind, 3, "instance", sig, "normal", [], spectral_norm=True)
    convs = sorted({k.rsplit(".", 1)[0] for k in a.state_dict()})
    assert sorted({k.rsplit(".", 1)[0] for k in c.state_dict()}) == convs
    for pre in convs:
        assert all(pre + "." + s in c.state_dict() for s in ("bias", "weight_orig", "weight_u", "weight_v"))
    assert not any(isinstance(m, (nn.InstanceNorm2d, nn.BatchNorm2d)) for m in c.modules())
    assert len(spectral_weights(c)) == len(convs) == len(c.spectral.convs)


def test_train_option():
    from options.train_options import default_train_opt, TrainOptions
    assert default_train_opt().spectral_norm is False
    assert default_train_opt(spectral_norm=True).spectral_norm is True
    import argparse
    p = TrainOptions().initialize(argparse.ArgumentParser())
    act = next(a for a in p._actions if "--spectral_norm" in a.option_strings)
    assert act.default is False and "generator" in act.help
