"""Resumable training, the host side on CPU tensors: Adam's moments in torch.optim.Adam's format, the
LossScaler and ImagePool state dicts, the RNG states as a weights_only file, the resume-epoch search and
the pruning over a directory listing, and the ranks' fingerprint agreement (gloo, world_size 2)."""
import os
import random

import numpy as np
import pytest
import torch

BETAS, EPS, LR = (0.5, 0.999), 1e-8, 2e-4


def _params(seed=0):
    g = torch.Generator().manual_seed(seed)
    return [torch.nn.Parameter(torch.randn(s, generator=g)) for s in ((4, 3, 2, 2), (4,), (7, 5), (1,))]


def _slots(params):
    """the flat layout of dsgan_hip.flat.FlatParams: every tensor on a 64-element boundary"""
    slots, n = [], 0
    for p in params:
        slots.append((n, tuple(p.shape)))
        n += (p.numel() + 63) // 64 * 64
    return slots, n


def _stepped_adam(params, steps, seed=1):
    opt = torch.optim.Adam(params, lr=LR, betas=BETAS, eps=EPS)
    g = torch.Generator().manual_seed(seed)
    for _ in range(steps):
        for p in params:
            p.grad = torch.randn(p.shape, generator=g)
        opt.step()
    return opt


def test_adam_state_round_trips_through_torch_format():
    from dsgan_hip.flat import adam_state_to_torch, adam_state_from_torch
    params = _params()
    slots, numel = _slots(params)
    group = {"lr": LR, "betas": BETAS, "eps": EPS, "params": params}
    g = torch.Generator().manual_seed(3)
    m, v = torch.zeros(numel), torch.zeros(numel)
    for off, shape in slots:
        k = int(np.prod(shape))
        m[off:off + k] = torch.randn(k, generator=g)
        v[off:off + k] = torch.rand(k, generator=g)
    sd = adam_state_to_torch(m, v, slots, 7, group)
    assert sorted(sd) == ["param_groups", "state"] and sorted(sd["state"]) == [0, 1, 2, 3]
    assert sd["param_groups"][0]["params"] == [0, 1, 2, 3] and sd["param_groups"][0]["lr"] == LR
    for i, p in enumerate(params):
        st = sd["state"][i]
        assert sorted(st) == ["exp_avg", "exp_avg_sq", "step"] and float(st["step"]) == 7.0
        assert st["exp_avg"].shape == p.shape and st["exp_avg_sq"].shape == p.shape and not st["exp_avg"].is_cuda
    m2, v2, step = adam_state_from_torch(sd, slots, numel, group)
    assert step == 7 and torch.equal(m2, m) and torch.equal(v2, v)
    # by name: a file whose entries come in another order pairs up through param_names
    names = ["a.weight", "a.bias", "b.weight", "b.bias"]
    perm = [2, 0, 3, 1]
    shuffled = {"state": {j: sd["state"][i] for j, i in enumerate(perm)},
                "param_groups": sd["param_groups"], "param_names": [names[i] for i in perm]}
    m3, v3, _ = adam_state_from_torch(shuffled, slots, numel, group, names=names)
    assert torch.equal(m3, m) and torch.equal(v3, v)
    # torch.optim.Adam takes it with its own load_state_dict and steps like the optimizer it came from
    a, b = _params(), _params()
    ref = _stepped_adam(a, 3)
    ma, va, step = adam_state_from_torch(ref.state_dict(), slots, numel, group)
    assert step == 3
    for i, (off, shape) in enumerate(slots):
        k = int(np.prod(shape))
        assert torch.equal(ma[off:off + k].view(shape), ref.state[a[i]]["exp_avg"])
        assert torch.equal(va[off:off + k].view(shape), ref.state[a[i]]["exp_avg_sq"])
    with torch.no_grad():
        for p, q in zip(a, b):
            q.copy_(p)
    other = torch.optim.Adam(b, lr=LR, betas=BETAS, eps=EPS)
    other.load_state_dict(adam_state_to_torch(ma, va, slots, step, group))
    for p, q in zip(a, b):
        p.grad = torch.full(p.shape, 0.25)
        q.grad = torch.full(q.shape, 0.25)
    ref.step()
    other.step()
    for p, q in zip(a, b):
        assert torch.equal(p, q)


def test_adam_state_refuses_mismatches():
    from dsgan_hip.flat import adam_state_to_torch, adam_state_from_torch
    params = _params()
    slots, numel = _slots(params)
    group = {"lr": LR, "betas": BETAS, "eps": EPS}
    names = ["a.weight", "a.bias", "b.weight", "b.bias"]
    sd = _stepped_adam(params, 2).state_dict()
    m, v, step = adam_state_from_torch(sd, slots, numel, group, names)
    assert step == 2 and float(m.abs().sum()) > 0
    assert adam_state_from_torch(torch.optim.Adam(_params(), lr=LR, betas=BETAS, eps=EPS).state_dict(), slots, numel,
                                 group)[2] == 0   # never stepped
    with pytest.raises(ValueError, match="betas"):
        adam_state_from_torch(sd, slots, numel, dict(group, betas=(0.9, 0.999)), names)
    with pytest.raises(ValueError, match="eps"):
        adam_state_from_torch(sd, slots, numel, dict(group, eps=1e-6), names)
    bad = adam_state_to_torch(m, v, slots, 2, group)
    bad["state"][2]["exp_avg"] = torch.zeros(5, 7)
    with pytest.raises(ValueError, match=r"b\.weight: exp_avg \(5, 7\)"):
        adam_state_from_torch(bad, slots, numel, group, names)
    bad = adam_state_to_torch(m, v, slots, 2, group)
    bad["state"][1]["step"] = torch.tensor(3.0)
    with pytest.raises(ValueError, match="step counts differ"):
        adam_state_from_torch(bad, slots, numel, group, names)
    bad = adam_state_to_torch(m, v, slots, 2, group)
    del bad["state"][3]
    with pytest.raises(ValueError, match=r"no entry for \['b\.bias'\]"):
        adam_state_from_torch(bad, slots, numel, group, names)
    bad = dict(adam_state_to_torch(m, v, slots, 2, group), param_names=["a.weight", "a.bias", "b.weight", "c.bias"])
    with pytest.raises(ValueError, match=r"c\.bias"):
        adam_state_from_torch(bad, slots, numel, group, names)


def test_loss_scaler_state_dict_on_cpu():
    from dsgan_hip.amp import LossScaler
    a = LossScaler("cpu")
    a.state.copy_(torch.tensor([2.0 ** 12, 1.0, 17.0, 2.0 ** -13, 41.0]))
    sd = a.state_dict()
    assert sorted(sd) == ["backoff", "growth", "interval", "state", "unit"] and sd["unit"] is False
    a.state[0] = 1.0   # the dict holds a copy
    b = LossScaler("cpu")
    ptr = b.state.data_ptr()
    b.load_state_dict(sd)
    assert b.state.tolist() == [2.0 ** 12, 1.0, 17.0, 2.0 ** -13, 41.0] and b.state.data_ptr() == ptr
    g = LossScaler.guard("cpu")
    assert g.state_dict()["unit"] is True
    with pytest.raises(ValueError, match="unit-scale"):
        g.load_state_dict(sd)
    with pytest.raises(ValueError, match="unit-scale"):
        b.load_state_dict(g.state_dict())
    g2 = LossScaler.guard("cpu")
    g.state[4] = 9.0
    g2.load_state_dict(g.state_dict())
    assert g2.state.tolist() == g.state.tolist()
    with pytest.raises(ValueError, match="interval"):
        LossScaler("cpu", growth_interval=10).load_state_dict(sd)


def test_image_pool_state_dict_on_cpu():
    from util.image_pool import ImagePool
    a = ImagePool(3, rng=random.Random(5))
    a.store = torch.randn(3, 2, 4, 4)
    a.num_imgs = 2
    a.rng.random()
    sd = a.state_dict()
    assert sd["pool_size"] == 3 and sd["num_imgs"] == 2 and tuple(sd["images"].shape) == (2, 2, 4, 4)
    assert isinstance(sd["rng"], list) and isinstance(sd["rng"][1], list)
    b = ImagePool(3, rng=random.Random(99))
    b.load_state_dict(sd, device="cpu")
    assert b.num_imgs == 2 and torch.equal(b.store[:2], a.store[:2]) and tuple(b.store.shape) == (3, 2, 4, 4)
    assert [b.rng.random() for _ in range(3)] == [a.rng.random() for _ in range(3)]
    # a resident pool keeps its tensor
    c = ImagePool(3, rng=random.Random(1))
    c.store = torch.zeros(3, 2, 4, 4)
    ptr = c.store.data_ptr()
    c.load_state_dict(sd)
    assert c.store.data_ptr() == ptr and torch.equal(c.store[:2], a.store[:2]) and c.num_imgs == 2
    with pytest.raises(ValueError, match="pool_size"):
        ImagePool(4, rng=random.Random(1)).load_state_dict(sd)
    d = ImagePool(3, rng=random.Random(1))
    d.store = torch.zeros(3, 2, 8, 8)
    with pytest.raises(ValueError, match="shape"):
        d.load_state_dict(sd)
    # the global `random`: no private state in the dict, and the two kinds do not mix
    e = ImagePool(3)
    assert e.state_dict()["rng"] is None and e.state_dict()["images"] is None
    with pytest.raises(ValueError, match="private RNG"):
        e.load_state_dict(sd)
    assert ImagePool(0).state_dict()["num_imgs"] == 0
    ImagePool(0).load_state_dict(ImagePool(0).state_dict())


def test_state_file_loads_weights_only(tmp_path):
    from dsgan_hip.amp import LossScaler
    from dsgan_hip.flat import adam_state_to_torch
    from models.base_model import atomic_save, rng_state_dict, load_rng_state_dict, train_state_filename
    from util.image_pool import ImagePool
    params = _params()
    slots, numel = _slots(params)
    pool = ImagePool(2, rng=random.Random(3))
    pool.store, pool.num_imgs = torch.randn(2, 6, 4, 4), 1
    random.seed(11), np.random.seed(12), torch.manual_seed(13)
    np.random.standard_normal()   # a cached gaussian in the legacy generator's state
    sd = {"version": 1, "epoch": 4, "world_size": 1, "precision": "bf16", "step_calls": {"G": 6, "D": 6},
          "optimizer_D": dict(adam_state_to_torch(torch.rand(numel), torch.rand(numel), slots, 6,
                                                  {"lr": LR, "betas": BETAS, "eps": EPS}), param_names=list("abcd")),
          "scaler_D": LossScaler.guard("cpu").state_dict(), "scaler_G": None, "pool": pool.state_dict(),
          "dropout": {"model.model.1": {"counter": 3, "seed": 2 ** 63 + 5, "stream": 65537}},
          "rng": rng_state_dict(), "layout": {"D": [["a", 0, 48]]}, "fingerprints": {"D.data": "%016x" % (2 ** 64 - 3)}}
    assert train_state_filename(4) == "4_train_state.pth" and train_state_filename(4, 2) == "4_train_state_rank2.pth"
    path = str(tmp_path / train_state_filename(4))
    atomic_save(sd, path)
    assert os.listdir(str(tmp_path)) == ["4_train_state.pth"]   # no temporary file left
    back = torch.load(path, map_location="cpu", weights_only=True)
    assert back["dropout"] == sd["dropout"] and back["fingerprints"] == sd["fingerprints"]
    assert back["layout"] == sd["layout"] and back["step_calls"] == sd["step_calls"]
    assert torch.equal(back["optimizer_D"]["state"][2]["exp_avg"], sd["optimizer_D"]["state"][2]["exp_avg"])
    want = (random.random(), np.random.standard_normal(), np.random.randint(1 << 30), torch.rand(3))
    random.seed(0), np.random.seed(0), torch.manual_seed(0)
    load_rng_state_dict(back["rng"])
    got = (random.random(), np.random.standard_normal(), np.random.randint(1 << 30), torch.rand(3))
    assert got[:3] == want[:3] and torch.equal(got[3], want[3])


def test_find_resume_epoch():
    import train as T
    nets = lambda e, ema=False: ["%d_useSE_net_G.pth" % e, "%d_useSE_net_D.pth" % e] + (["%d_useSE_net_G_ema.pth" % e] if ema else [])  # noqa: E731
    assert T.find_resume_epoch([]) is None
    assert T.find_resume_epoch(nets(1) + nets(2) + ["opt.txt"]) is None   # weights alone: today's --continue_train
    base = nets(1) + nets(2) + nets(3) + ["1_train_state.pth", "2_train_state.pth", "opt.txt"]
    assert T.find_resume_epoch(base) == 2
    # temporary and partial files of a save that was killed
    assert T.find_resume_epoch(base + ["3_train_state.pth.tmp4242", "3_train_state.pth.part", "tmp_3_train_state.pth"]) == 2
    # the newest state without its network files does not count
    assert T.find_resume_epoch(base + ["4_train_state.pth", "4_useSE_net_G.pth"]) == 2
    assert T.find_resume_epoch(base + ["4_train_state.pth", "4_useSE_net_G.pth", "4_net_D.pth"]) == 4
    assert T.find_resume_epoch(base + ["10_train_state.pth"] + nets(10)) == 10   # by number, not by name
    # the averaged generator's file when the run keeps one
    assert T.find_resume_epoch(base, ema=True) is None
    assert T.find_resume_epoch(base + ["1_useSE_net_G_ema.pth"], ema=True) == 1
    # every rank's file under torchrun
    assert T.find_resume_epoch(base, world=2) is None
    assert T.find_resume_epoch(base + ["1_train_state_rank1.pth", "2_train_state_rank2.pth"], world=2) == 1
    assert T.find_resume_epoch(["2_train_state_rank1.pth"] + nets(2), world=2) is None   # rank 0's is missing


def test_states_to_prune_keeps_n():
    import train as T
    names = ["%d_useSE_net_%s.pth" % (e, n) for e in (1, 2, 3, 10) for n in ("G", "D")]
    names += ["%d_train_state.pth" % e for e in (1, 2, 3, 10)] + ["%d_train_state_rank1.pth" % e for e in (2, 3, 10)]
    names += ["opt.txt", "3_train_state.pth.tmp77"]
    assert T.states_to_prune(names, 2) == ["1_train_state.pth", "2_train_state.pth", "2_train_state_rank1.pth"]
    assert T.states_to_prune(names, 4) == [] and T.states_to_prune(names, 9) == []
    assert T.states_to_prune(names, 1) == sorted(["1_train_state.pth", "2_train_state.pth", "2_train_state_rank1.pth",
                                                  "3_train_state.pth", "3_train_state_rank1.pth"])
    assert all("train_state" in n and n.endswith(".pth") for n in T.states_to_prune(names, 0))
    assert len(T.states_to_prune(names, 0)) == 7


def test_fingerprint_mismatches_is_pure():
    from dsgan_hip.dist import fingerprint_mismatches
    rows = torch.tensor([[1, -2, 3], [1, -2, 3], [1, 5, 3]], dtype=torch.int64)
    assert fingerprint_mismatches(rows[:2], ["a", "b", "c"]) == []
    assert fingerprint_mismatches(rows, ["a", "b", "c"]) == [(2, "b")]


def _agree_worker(rank, world, port, q):
    import torch.distributed as dist
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    from dsgan_hip import dist as hdist
    names = ["G.data", "D.data", "G.exp_avg"]
    same = torch.tensor([5, -(1 << 63), (1 << 63) - 1], dtype=torch.int64)
    out = []
    try:
        hdist.require_same_fingerprints(same.clone(), names)
        out.append("ok")
    except RuntimeError as e:
        out.append(str(e))
    mine = same.clone()
    if rank == 1:
        mine[1] += 1
    try:
        hdist.require_same_fingerprints(mine, names)
        out.append("ok")
    except RuntimeError as e:
        out.append(str(e))
    q.put((rank, out))
    dist.destroy_process_group()


def test_rank_agreement_gloo_world2():
    import multiprocessing as mp
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = 33500 + random.Random().randint(0, 2000)
    ps = [ctx.Process(target=_agree_worker, args=(r, 2, port, q)) for r in range(2)]
    for p in ps:
        p.start()
    out = dict(q.get(timeout=120) for _ in ps)
    for p in ps:
        p.join(timeout=60)
    for r in (0, 1):
        assert out[r][0] == "ok"
        assert "D.data on rank 1" in out[r][1] and "G.data" not in out[r][1] and "exp_avg" not in out[r][1]
    # one process: nothing to compare, no process group needed
    from dsgan_hip import dist as hdist
    hdist.require_same_fingerprints(torch.tensor([1], dtype=torch.int64), ["x"])
    with pytest.raises(ValueError):
        hdist.require_same_fingerprints(torch.tensor([1.0]), ["x"])
