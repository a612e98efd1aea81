"""``--norm batch`` (the BatchNorm2d PatchGAN), the parts that need no GPU: the state_dict surface and
the seed-20 init draw against the reference's (tests/golden/golden_v6.npz, written by
tests/golden/gen_golden_v6.py from DSGAN/models/networks.py:21-30, 49-70, 115-131, 533-579), the
pairings that keep raising, and the scratch contract / launch planner of batchnorm.hip in plan-only
mode (dsgan_set_plan_only: validation and planning run on the host, no HIP call is made)."""
import json
import os
import random

import numpy as np
import pytest
import torch

G6 = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "golden_v6.npz"))

# (N, C, H, W) of tests/test_batchnorm_ops_gpu.py: its SHAPES, the strided case's view and the offset cases
OP_SHAPES = [(2, 64, 3, 3), (3, 5, 31, 31), (2, 4, 128, 128), (16, 256, 7, 7), (2, 5, 31, 31), (4, 6, 32, 32),
             (2, 6, 48, 48), (2, 3, 129, 129), (3, 5, 3, 3)]
SWEEP = OP_SHAPES + [(16, 64, 64, 64), (16, 128, 32, 32), (16, 256, 31, 31), (32, 64, 64, 64), (1, 512, 1, 2),
                     (2, 128, 16, 16), (1, 1, 4097, 1), (64, 3, 256, 256), (1, 130, 128, 128), (2, 1, 1, 1)]


@pytest.mark.parametrize("kind,n_layers", [("basic", 3), ("n_layers", 2)])
@pytest.mark.parametrize("sig", [0, 1])
def test_discriminator_keys_and_shapes(kind, n_layers, sig):
    from models.networks import define_D, has_batch_stats
    d = define_D(6, 32, kind, n_layers, "batch", bool(sig), "normal", [])
    sd = d.state_dict()
    assert list(sd.keys()) == list(G6["D6_%s_%d_keys" % (kind, sig)])
    assert [json.dumps(list(v.shape)) for v in sd.values()] == list(G6["D6_%s_%d_shapes" % (kind, sig)])
    assert has_batch_stats(d) and d.norm == "batch"
    plain = define_D(6, 32, kind, n_layers, "instance", bool(sig), "normal", [])
    assert not has_batch_stats(plain) and plain.norm == "instance"


def test_basic_key_list():
    """The keys the issue lists: bias-free convs in front of a BatchNorm."""
    from models.networks import define_D
    keys = list(define_D(6, 32, "basic", 3, "batch", False, "normal", []).state_dict().keys())
    want = ["model.0.weight", "model.0.bias"]
    for c in (2, 5, 8):
        want += ["model.%d.weight" % c] + ["model.%d.%s" % (c + 1, s) for s in
                                           ("weight", "bias", "running_mean", "running_var", "num_batches_tracked")]
    assert keys == want + ["model.11.weight", "model.11.bias"]


def test_init_draw_matches_reference():
    """setup_seed(20), then define_D(6, 32, 'basic', 3, 'batch', False): conv weights N(0, 0.02) and
    BatchNorm weights N(1, 0.02) in the reference's post-order, from the CPU generator."""
    from models.networks import define_D
    torch.manual_seed(20)
    np.random.seed(20)
    random.seed(20)
    d = define_D(6, 32, "basic", 3, "batch", False, "normal", [])
    vals = [v.detach().double().flatten() for v in d.state_dict().values()]
    assert len(vals) == len(G6["I6_sum"])
    for i, v in enumerate(vals):
        assert abs(float(v.sum()) - G6["I6_sum"][i]) <= 1e-9 * max(1.0, abs(G6["I6_sum"][i])), i
        assert abs(float(v.abs().sum()) - G6["I6_abs"][i]) <= 1e-9 * max(1.0, G6["I6_abs"][i]), i
        n = min(8, v.numel())
        assert np.array_equal(v[:n].numpy(), G6["I6_head"][i][:n]), i
    assert np.array_equal(torch.rand(4, dtype=torch.float64).numpy(), G6["I6_rng_after"])
    bn = d.model[3]
    assert abs(float(bn.weight.detach().mean()) - 1.0) < 0.02 and float(bn.bias.detach().abs().max()) == 0.0


def test_unsupported_pairings_still_raise():
    from models.networks import define_D
    for kind in ("pixel", "multi"):
        with pytest.raises(NotImplementedError, match="norm"):
            define_D(6, 32, kind, 3, "batch", True, "normal", [])
    for kind in ("basic", "n_layers", "pixel", "multi"):
        with pytest.raises(NotImplementedError, match="norm"):
            define_D(6, 32, kind, 3, "none", True, "normal", [])


def test_load_networks_keeps_a_batchnorms_buffers(tmp_path):
    """BaseModel.load_networks drops running_mean / running_var keys only where the model has none
    (the reference's InstanceNorm patch, DSGAN/models/base_model.py:108-109)."""
    from models.base_model import BaseModel
    from models.networks import define_D

    class M(BaseModel):
        pass

    for norm in ("batch", "instance"):
        m = M()
        m.model_names, m.save_dir = ["D"], str(tmp_path)
        m.netD = define_D(6, 8, "basic", 3, norm, False, "normal", [])
        src = define_D(6, 8, "basic", 3, norm, False, "normal", [])
        sd = {("module." + k): v.clone() for k, v in src.state_dict().items()}
        for k, v in sd.items():
            if "running" in k or "tracked" in k:
                v.fill_(3)
        if norm == "instance":   # a pre-0.4 InstanceNorm checkpoint: buffers the model does not have
            sd["module.model.3.running_mean"] = torch.zeros(16)
            sd["module.model.3.running_var"] = torch.ones(16)
        torch.save(sd, os.path.join(str(tmp_path), "4_net_D.pth"))
        m.load_networks("4")
        got = m.netD.state_dict()
        assert list(got) == list(src.state_dict())
        for k, v in got.items():
            assert torch.equal(v, sd["module." + k]), k
        if norm == "batch":
            assert float(got["model.3.running_mean"][0]) == 3.0 and float(got["model.9.running_var"][-1]) == 3.0
            assert int(got["model.6.num_batches_tracked"]) == 3


# ---- batchnorm.hip in plan-only mode --------------------------------------------------------------

@pytest.fixture(scope="module")
def lib():
    from dsgan_hip import _lib
    if not os.path.exists(_lib.LIB_PATH):
        pytest.skip("libdsgan_hip.so not built (run __graft_entry__.build())")
    lib = _lib.load()
    old = lib.dsgan_set_plan_only(1)
    assert old == 0
    yield lib
    lib.dsgan_set_plan_only(0)
    lib.dsgan_batchnorm_tune(0, 0)


# a host buffer standing in for every device operand: plan-only launchers never dereference it
_BUF = np.zeros(1 << 12, dtype=np.uint8)
A = (_BUF.ctypes.data + 255) // 256 * 256
WS = A + 1024


def _fwd(lib, N, C, HW, ws, n, training=1):
    return lib.dsgan_batchnorm_fwd(A, C * HW, A, A, A, C * HW, A, A, A + 512, A + 512, A, N, C, HW, 3, 0.2, 1e-5, 0.1,
                                   training, ws, n, None)


def _bwd(lib, N, C, HW, ws, n, training=1):
    return lib.dsgan_batchnorm_bwd(A, C * HW, A, C * HW, A, A, A, A, A, C * HW, A, A, N, C, HW, 3, 0.2, training, ws, n,
                                   None)


@pytest.mark.parametrize("form", [0, 1, 2])
def test_scratch_contract(lib, form):
    """Each call passes with the queried scratch and is refused one element short (whenever the plan
    needs scratch), in training and in eval mode, under the planner's choice and both forced forms."""
    lib.dsgan_batchnorm_tune(0, form)
    assert lib.dsgan_batchnorm_tune(0, -1) == form
    n_ws = 0
    for N, C, H, W in SWEEP:
        HW = H * W
        q = lib.dsgan_batchnorm_workspace(N, C, HW)
        plan = lib.dsgan_batchnorm_plan(N, C, HW)
        assert plan in (0, 1) and (q > 0) == (plan == 1), (N, C, HW, plan, q)
        for training in ((1, 0) if N * HW > 1 else (0,)):
            for fn in (_fwd, _bwd):
                assert fn(lib, N, C, HW, WS if q else None, q, training) == 0, (fn.__name__, N, C, HW,
                                                                                  lib.dsgan_last_error_string())
                assert lib.dsgan_last_ws_need() == q
                if q > 0:
                    n_ws += 1
                    assert fn(lib, N, C, HW, WS, q - 1, training) == -1
                    assert b"scratch" in lib.dsgan_last_error_string()
                    assert fn(lib, N, C, HW, None, q, training) == -1
    assert n_ws > 0
    lib.dsgan_batchnorm_tune(0, 0)


def test_planner_rules_and_refusals(lib):
    lib.dsgan_batchnorm_tune(0, 0)
    # one workgroup per channel: the channel fits one slice, or it fits the register cache and the
    # channels fill the machine; split otherwise
    assert lib.dsgan_batchnorm_plan(16, 256, 961) == 0      # 15 376 values, 256 channels
    assert lib.dsgan_batchnorm_plan(16, 128, 1024) == 0     # 16 384 values, 128 channels
    assert lib.dsgan_batchnorm_plan(16, 127, 1024) == 1
    assert lib.dsgan_batchnorm_plan(16, 64, 4096) == 1      # 65 536 values: beyond the cache
    assert lib.dsgan_batchnorm_plan(17, 256, 1024) == 1
    assert lib.dsgan_batchnorm_plan(4, 1, 1024) == 0 and lib.dsgan_batchnorm_plan(4, 1, 1025) == 1
    assert lib.dsgan_batchnorm_workspace(16, 64, 4096) == 64 * 16 * 3
    assert lib.dsgan_batchnorm_workspace(64, 3, 65536) == 3 * 64 * 3   # at most 64 slices
    # the op-test shapes reach every id the planner returns
    assert {lib.dsgan_batchnorm_plan(N, C, H * W) for N, C, H, W in OP_SHAPES} == {0, 1}
    # refused on the host: one value per channel in training mode, no channels, bad strides / pairs
    assert _fwd(lib, 1, 4, 1, None, 0, training=1) == -1
    assert b"more than 1 value per channel" in lib.dsgan_last_error_string()
    assert _fwd(lib, 1, 4, 1, None, 0, training=0) == 0
    assert _bwd(lib, 1, 4, 1, None, 0, training=1) == -1
    for C in (0, -3):
        assert _fwd(lib, 2, C, 16, None, 0) == -1 and _bwd(lib, 2, C, 16, None, 0) == -1
        assert lib.dsgan_batchnorm_plan(2, C, 16) == -1 and lib.dsgan_batchnorm_workspace(2, C, 16) == 0
    assert lib.dsgan_batchnorm_fwd(A, 15, A, A, A, 64, A, A, A + 512, A + 512, A, 2, 4, 16, 3, 0.2, 1e-5, 0.1, 1, None, 0,
                                   None) == -1
    assert lib.dsgan_batchnorm_bwd(A, 64, A, 64, A, A, A, A, A, 64, A, None, 2, 4, 16, 3, 0.2, 1, None, 0, None) == -1
    # eval mode may not write mean / rstd over the buffers it reads
    assert lib.dsgan_batchnorm_fwd(A, 64, A, A, A, 64, A, A, A, A + 512, None, 2, 4, 16, 3, 0.2, 1e-5, 0.1, 0, None, 0,
                                   None) == -1


def test_functional_refuses_on_the_host():
    """m == 1 in training mode and momentum=None raise before any device work (CPU tensors would be
    refused by ptr() otherwise: the errors here come first)."""
    from dsgan_hip import functional as HF
    bn = torch.nn.BatchNorm2d(4)
    with pytest.raises(ValueError, match="Expected more than 1 value per channel when training"):
        HF.batch_norm(torch.zeros(1, 4, 1, 1), bn, act="lrelu")
    with pytest.raises(NotImplementedError, match="momentum"):
        HF.batch_norm(torch.zeros(2, 4, 3, 3), torch.nn.BatchNorm2d(4, momentum=None))
    with pytest.raises(NotImplementedError, match="affine"):
        HF.batch_norm(torch.zeros(2, 4, 3, 3), torch.nn.BatchNorm2d(4, affine=False))
