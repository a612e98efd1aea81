"""The U-Net generator's host side, without a GPU: construction through ``define_G``, the state_dict
and the init draw against the reference (tests/golden/golden_v7.npz), the fixture's restatement and mask
twin (tests/unet_fixture.py), and the kernel families its layers take.
"""
import inspect
import json
import os
import random
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from unet_fixture import (unet_spec, unet_params, unet_levels, torch_unet, philox_mask, philox_words,  # noqa: E402
                          unet_conv_calls, prelu_keys, out_view)
from oracle.recipe import synth_pair  # noqa: E402

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
G7 = np.load(os.path.join(GOLD, "golden_v7.npz"))
NETS = [(5, 8, 32), (6, 8, 64), (5, 32, 32)]


@pytest.mark.parametrize("drop", [False, True])
@pytest.mark.parametrize("norm", ["instance", "batch"])
def test_define_g_builds_unet_128_with_the_reference_state_dict(norm, drop):
    from models.networks import define_G
    from models.unet import UnetGenerator
    net = define_G(3, 3, 64, "unet_128", norm, drop, "normal", [])
    assert isinstance(net, UnetGenerator)
    sd = net.state_dict()
    pre = "K7_%s_%d_" % (norm, int(drop))
    assert list(sd.keys()) == list(G7[pre + "keys"])
    assert [json.dumps(list(v.shape)) for v in sd.values()] == list(G7[pre + "shapes"])
    assert sum(p.numel() for p in net.parameters()) == int(G7[pre + "nparams"])
    assert [(k, tuple(v.shape)) for k, v in sd.items()] == unet_spec(3, 3, 7, 64, norm, drop)
    if norm == "batch":
        assert len(sd) == 77 and int(G7[pre + "nparams"]) == 41829002
    # every PReLU is a learnable (1,) parameter at 0.25 that init_weights leaves alone
    pk = prelu_keys(unet_spec(3, 3, 7, 64, norm, drop))
    assert len(pk) == 7 and all(sd[k].item() == 0.25 for k in pk)
    assert all(dict(net.named_parameters())[k].requires_grad for k in pk)
    # dropout state: two blocks (num_downs - 5), stream ids 0 and 1, counters outside the state_dict
    blocks = net.dropout_blocks()
    assert len(blocks) == (2 if drop else 0)
    assert [b.drop_stream for b in blocks] == list(range(len(blocks)))
    assert all(b.drop_counter.dtype == torch.int64 and int(b.drop_counter) == 0 for b in blocks)
    assert not any("drop" in k for k in sd)
    net.load_state_dict(sd, strict=True)


def test_init_draw_equals_the_reference():
    from models.networks import define_G
    torch.manual_seed(20)
    np.random.seed(20)
    random.seed(20)
    net = define_G(3, 3, 64, "unet_128", "batch", True, "normal", [])
    vals = [v.detach().double().flatten() for v in net.state_dict().values()]
    assert len(vals) == len(G7["I7_sum"])
    for i, v in enumerate(vals):   # the sums to fp64 summation order (it differs between hosts), the heads exactly
        assert abs(float(v.sum()) - G7["I7_sum"][i]) <= 1e-9 * max(1.0, abs(G7["I7_sum"][i])), i
        assert abs(float(v.abs().sum()) - G7["I7_abs"][i]) <= 1e-9 * max(1.0, G7["I7_abs"][i]), i
        n = min(8, v.numel())
        assert np.array_equal(v[:n].numpy(), G7["I7_head"][i][:n]), i
    assert np.array_equal(torch.rand(4, dtype=torch.float64).numpy(), G7["I7_rng_after"])
    assert [b.drop_seed for b in net.dropout_blocks()] == [20, 20]   # torch's seed at construction


def test_names_that_raise():
    from models.networks import define_G
    with pytest.raises(NotImplementedError, match="num_downs=8"):
        define_G(3, 3, 64, "unet_256", "instance")
    with pytest.raises(NotImplementedError, match="norm"):
        define_G(3, 3, 64, "unet_128", "none")
    for name in ("unet_64", "resnet_9blocks", "gll", "cascaded"):
        with pytest.raises(NotImplementedError, match="not recognized"):
            define_G(3, 3, 64, name, "instance")


def test_unet_generator_builds_at_any_depth():
    from models.networks import get_norm_layer
    from models.unet import UnetGenerator
    for nd in (5, 6, 8):
        net = UnetGenerator(3, 3, nd, 8, norm_layer=get_norm_layer("batch"), use_dropout=True)
        assert [(k, tuple(v.shape)) for k, v in net.state_dict().items()] == unet_spec(3, 3, nd, 8, "batch", True)
        assert len(net.dropout_blocks()) == nd - 5


@pytest.mark.parametrize("nd,ngf,size", NETS)
@pytest.mark.parametrize("norm", ["instance", "batch"])
def test_fixture_restatement_reproduces_the_reference(norm, nd, ngf, size):
    pre = "N7_%s_%d_%d_%d_" % (norm, nd, ngf, size)
    A, _ = synth_pair(2, size, seed=int(G7[pre + "input_seed"]))
    for drop in ((False, True) if nd > 5 else (False,)):
        params = unet_params(unet_spec(3, 3, nd, ngf, norm, drop))
        lv = unet_levels(3, 3, nd, ngf, drop)
        masks = [torch.from_numpy(philox_mask((2, ngf * 8, size >> 4, size >> 4), int(G7["N7_drop_seed"]), 0, 0))] if drop else None
        key = "_dout" if drop else "_out"
        g64, g32 = G7[pre + "f64" + key], G7[pre + "f32" + key]
        outs = {}
        for dt in (torch.float64, torch.float32):
            p = {k: (v.clone().to(dt) if v.is_floating_point() else v.clone()) for k, v in params.items()}
            x = A.clone().to(dt)
            with torch.no_grad():
                full = torch_unet(x, p, lv, norm, masks).double()
                outs[dt] = out_view(full).numpy()
            if dt == torch.float64:
                assert abs(float(full.norm()) - float(G7[pre + "f64" + key + "_norm"])) <= 1e-12 * float(full.norm())
            assert torch.equal(x, A.to(dt))   # the restatement leaves its input alone
            if norm == "batch" and not drop and dt == torch.float64:
                rm = np.concatenate([v.numpy() for k, v in p.items() if k.endswith("running_mean")])
                rv = np.concatenate([v.numpy() for k, v in p.items() if k.endswith("running_var")])
                assert np.abs(rm - G7[pre + "f64_rm"]).max() <= 1e-12 and np.abs(rv - G7[pre + "f64_rv"]).max() <= 1e-12
                assert all(int(v) == 1 for k, v in p.items() if k.endswith("num_batches_tracked"))
        nrm = np.linalg.norm(g64)
        assert np.linalg.norm(outs[torch.float64] - g64) / nrm <= 1e-12
        own = np.linalg.norm(g32.astype(np.float64) - g64) / nrm     # the reference's own fp32-vs-fp64 distance
        assert 0 < own < 1e-5
        assert np.linalg.norm(outs[torch.float32] - g32.astype(np.float64)) / nrm <= own
        assert np.abs(g64).max() <= 1.0 and g64.shape == (2, 3, min(size, 32), min(size, 32))


def test_in_place_skip_quirk_is_what_the_fixture_computes():
    """One inner block by hand: the skip half of the concatenation is lrelu(x), not x."""
    lv = unet_levels(3, 3, 5, 8)
    p = {k: v.double() if v.is_floating_point() else v for k, v in unet_params(unet_spec(3, 3, 5, 8, "instance")).items()}
    A, _ = synth_pair(2, 32, seed=43)
    import torch.nn.functional as F
    z = F.conv2d(A.double(), p["model.model.0.weight"], p["model.model.0.bias"], stride=2, padding=1)
    seen = []
    orig = F.prelu

    def spy(t, w):
        seen.append(t.clone())
        return orig(t, w)
    F.prelu = spy
    try:
        torch_unet(A.double(), p, lv, "instance")
    finally:
        F.prelu = orig
    outer_in = seen[-1]            # the outermost PReLU's input: cat(lrelu(z), up)
    assert torch.equal(outer_in[:, :8], F.leaky_relu(z, 0.2)) and not torch.equal(outer_in[:, :8], z)


def test_mask_twin():
    # Random123's known answers for philox4x32-10
    assert [int(w) for w in philox_words([0], 0, 0, 0)[0]] == [0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8]
    w = philox_words(np.array([0x85a308d3243f6a88], dtype=np.uint64), (0x299f31d0 << 32) | 0xa4093822, 0x03707344, 0x13198a2e)[0]
    assert [int(x) for x in w] == [0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1]
    shape, n = (2, 64, 16, 16), 32768
    for seed, stream in ((20, 3), (int(G7["N7_drop_seed"]), 0), (20, 0), (20, 1)):   # the seeds / streams the GPU tests use
        m0, m1 = philox_mask(shape, seed, stream, 0), philox_mask(shape, seed, stream, 1)
        assert np.array_equal(m0, philox_mask(shape, seed, stream, 0))
        assert not np.array_equal(m0, m1)
        for m in (m0, m1):
            assert set(np.unique(m)) == {0.0, 1.0}
            assert abs(m.sum() / n - 0.5) <= 2.5 / np.sqrt(n)
    assert not np.array_equal(philox_mask(shape, 20, 3, 0), philox_mask(shape, 21, 3, 0))
    assert not np.array_equal(philox_mask(shape, 20, 3, 0), philox_mask(shape, 20, 4, 0))
    # a shape that is no multiple of four elements uses the head of the same stream
    assert np.array_equal(philox_mask((2, 5, 3, 3), 20, 3, 7).reshape(-1), philox_mask((90,), 20, 3, 7))
    assert np.array_equal(philox_mask((90,), 20, 3, 7), philox_mask((92,), 20, 3, 7)[:90])


def test_conv_families_of_unet_128():
    """Every conv question unet_128 asks at (16, 3, 256, 256), ngf 64, in fp32 and bf16, pinned in
    tests/golden/unet_dispatch_v1.json; in bf16 no layer with both channel counts a multiple of 32 may
    fall to igemm_kernel.  The stem (3 -> 64 with its LeakyReLU) takes the pgstem kernels."""
    from dsgan_hip import _lib
    if not os.path.exists(_lib.LIB_PATH):
        pytest.skip("libdsgan_hip.so not built (run __graft_entry__.build())")
    from dsgan_hip import functional as HF
    with open(os.path.join(GOLD, "unet_dispatch_v1.json")) as f:
        rows = json.load(f)
    calls = unet_conv_calls(16, 256, 3, 3, 7, 64)
    assert len(rows) == 2 * len(calls)
    choosers = {"fwd": HF.conv_fwd_family, "dgrad": HF.conv_dgrad_family, "wgrad": HF.conv_wgrad_family}
    old = HF._state["prec"]
    base = 1 << 32
    try:
        for i, r in enumerate(rows):
            c = calls[i % len(calls)]
            assert all(r[k] == v for k, v in c.items()), (r, c)
            HF._state["prec"] = r["prec"]
            if r["layer"] == "L0.down":
                assert r["fam"] == "pgstem_kernel" and _lib.load().dsgan_pgstem_supported(3, 64, 256, 256) == 1
                continue
            fn = choosers[r["op"]]
            got = fn(**{k: (base + r[k] if k.endswith("_ptr") and r[k] is not None else r[k])
                        for k in inspect.signature(fn).parameters})
            assert got == (r["fam"], r["form"]), (r["layer"], r["op"], r["prec"], got)
            if r["prec"] == "bf16" and r["Cin"] % 32 == 0 and r["Cout"] % 32 == 0:
                assert r["fam"] != "igemm_kernel", r
    finally:
        HF._state["prec"] = old
    assert {r["prec"] for r in rows} == {"fp32", "bf16"}
