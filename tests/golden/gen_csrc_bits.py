"""Record tests/golden/csrc_bits_v1.json: sha1 digests of the output bytes of the InstanceNorm entry
points (every rung of the float4 and scalar plane-size ladders, both sides of each threshold; the
16-bit forms under both half types; the split `_ws` forms) and of dsgan_mlp_bwd's two LDS-DMA
kernels.  tests/test_csrc_bits_gpu.py recomputes them with the in-tree library and compares for
equality, so a change of host dispatch or of shared helper text that moves one output bit fails.

    DSGAN_HIP_LIB=<the library to pin> python tests/golden/gen_csrc_bits.py [out.json]

Inputs come from CPU torch.Generators with fixed seeds; outputs start zeroed, so an element a
kernel does not write is part of the digest too.
"""
import contextlib
import hashlib
import json
import math
import os
import sys
import zlib

import torch

HERE = os.path.dirname(os.path.abspath(__file__))
FIXTURE = os.path.join(HERE, "csrc_bits_v1.json")

ACT = {"none": 0, "gelu": 1, "relu": 2, "lrelu": 3, "gelu_fast": 5}
ALIGNED = [16, 1024, 1028, 4096, 4100, 16384, 16388, 65536, 65540]   # both sides of every float4 threshold
SCALAR = [1023, 1025, 4095, 4097, 16383, 16385]                      # ... of every scalar threshold (HW % 4 != 0)
HALVES = {"bf16": torch.bfloat16, "fp16": torch.float16}
SLOPE, EPS = 0.2, 1e-5


def planes_of(HW):
    """5 planes where four share a workgroup (a ragged last workgroup), fewer as planes grow."""
    return 5 if HW <= 1024 else 3 if HW <= 16388 else 2


def _api():
    import dsgan_hip
    from dsgan_hip import _lib
    dsgan_hip.require_gpu()
    return _lib


def digest(*ts):
    h = hashlib.sha1()
    for t in ts:
        if t is None:
            continue
        t = t.detach().cpu().contiguous()
        h.update((t.view(torch.int16) if t.dtype in (torch.bfloat16, torch.float16) else t).numpy().tobytes())
    return h.hexdigest()


class Rand:
    """Device tensors drawn on the CPU from a generator seeded by the case id."""

    def __init__(self, case_id):
        self.g = torch.Generator().manual_seed(zlib.crc32(case_id.encode()))

    def __call__(self, *shape, scale=1.0, shift=0.0, off=0):
        t = torch.randn(math.prod(shape) + off, generator=self.g) * scale + shift
        return t.cuda()[off:].view(*shape)

    def stats(self, planes):
        """a plausible (mean, rstd) pair: the backward kernels take them as inputs"""
        return self(planes, scale=0.1), self(planes, scale=0.05, shift=1.0).abs()


def zeros(*shape, dtype=torch.float32):
    return torch.zeros(*shape, device="cuda", dtype=dtype)


@contextlib.contextmanager
def half(name):
    from dsgan_hip import functional as HF
    with HF.precision(name):
        yield HALVES[name]


def in_fwd(L, cid, N, C, HW, act, res=False, scale=False, off=0, ws=False):
    r = Rand(cid)
    x = r(N, C, HW, scale=2.0, shift=0.3, off=off)
    rs = r(N, C, HW) if res else None
    sc = r(N * C, scale=0.2, shift=1.0) if scale else None
    y, mean, rstd = zeros(N, C, HW), zeros(N * C), zeros(N * C)
    args = [L.ptr(x), C * HW, L.ptr(sc), L.ptr(rs), C * HW, L.ptr(y), C * HW, L.ptr(mean), L.ptr(rstd), N, C, HW,
            ACT[act], SLOPE, EPS]
    if ws:
        w = zeros(max(1, L.load().dsgan_instnorm_workspace(N, C, HW)))
        L.call("dsgan_instnorm_fwd_ws", *args, L.ptr(w), w.numel(), L.stream())
    else:
        L.call("dsgan_instnorm_fwd", *args, L.stream())
    return digest(y, mean, rstd)


def in_fwd_h(L, cid, N, C, HW, dt):
    r = Rand(cid)
    x = r(N, C, HW, scale=2.0, shift=0.3)
    y, mean, rstd = zeros(N, C, HW, dtype=dt), zeros(N * C), zeros(N * C)
    L.call("dsgan_instnorm_fwd_bf16", L.ptr(x), C * HW, L.ptr(y), C * HW, L.ptr(mean), L.ptr(rstd), N, C, HW, EPS,
           L.stream())
    return digest(y, mean, rstd)


def in_bwd(L, cid, N, C, HW, act, extras=False, ws=False):
    """extras: scale, res, dres and dscale present"""
    r = Rand(cid)
    x, dy = r(N, C, HW, scale=2.0, shift=0.3), r(N, C, HW)
    mean, rstd = r.stats(N * C)
    rs = r(N, C, HW) if extras else None
    sc = r(N * C, scale=0.2, shift=1.0) if extras else None
    dx = zeros(N, C, HW)
    dres = zeros(N, C, HW) if extras else None
    dscale = zeros(N * C) if extras else None
    args = [L.ptr(dy), C * HW, L.ptr(x), C * HW, L.ptr(sc), L.ptr(rs), C * HW, L.ptr(mean), L.ptr(rstd), L.ptr(dx),
            C * HW, L.ptr(dres), C * HW, L.ptr(dscale), N, C, HW, ACT[act], SLOPE, EPS]
    if ws:
        w = zeros(max(1, L.load().dsgan_instnorm_workspace(N, C, HW)))
        L.call("dsgan_instnorm_bwd_ws", *args, L.ptr(w), w.numel(), L.stream())
    else:
        L.call("dsgan_instnorm_bwd", *args, L.stream())
    return digest(dx, dres, dscale)


def in_bwd_h(L, cid, N, C, HW, act, dt, extras=False):
    """extras: res, dres and dxsum present"""
    r = Rand(cid)
    x, dy = r(N, C, HW, scale=2.0, shift=0.3), r(N, C, HW)
    mean, rstd = r.stats(N * C)
    rs = r(N, C, HW) if extras else None
    dxh = zeros(N, C, HW, dtype=dt)
    dres = zeros(N, C, HW) if extras else None
    dxsum = zeros(N * C) if extras else None
    L.call("dsgan_instnorm_bwd_h", L.ptr(dy), C * HW, L.ptr(x), C * HW, L.ptr(rs), C * HW, L.ptr(mean), L.ptr(rstd),
           L.ptr(dxh), C * HW, L.ptr(dxsum), L.ptr(dres), C * HW, N, C, HW, ACT[act], SLOPE, EPS, L.stream())
    return digest(dxh, dres, dxsum)


def mlp_bwd(L, cid, dt, C=256, P=128, nb=1, HW=128):
    r = Rand(cid)
    C4 = 4 * C
    h = r(nb, C, HW).to(dt)
    dy = r(nb, P, HW)
    w1 = r(C4, C, scale=C ** -0.5).to(dt)
    w2 = r(P, C4, scale=C4 ** -0.5).to(dt)
    b1 = r(C4, scale=0.1)
    dh = zeros(nb, C, HW)
    g, dz = zeros(nb, C4, HW, dtype=dt), zeros(nb, C4, HW, dtype=dt)
    bsum = zeros(nb * HW // L.load().dsgan_mlp_supported(C, P, HW), C4)
    L.call("dsgan_mlp_bwd", L.ptr(h), C * HW, 1, L.ptr(dy), P * HW, L.ptr(w1), L.ptr(b1), L.ptr(w2), L.ptr(dh), C * HW,
           L.ptr(g), L.ptr(dz), L.ptr(bsum), nb, C, P, HW, L.stream())
    return digest(dh, g, dz, bsum)


def compute(group):
    """{case id: sha1} of one group of cases, run on the library dsgan_hip._lib loads."""
    L = _api()
    out = {}

    def put(fn, cid, *a, **k):
        out[cid] = fn(L, cid, *a, **k)

    if group == "fwd_aligned":
        for HW in ALIGNED:
            for act in ("none", "gelu", "lrelu", "gelu_fast"):
                put(in_fwd, "fwd/%d/%s" % (HW, act), 1, planes_of(HW), HW, act)
        put(in_fwd, "fwd/4100/gelu/res", 1, 3, 4100, "gelu", res=True)
        put(in_fwd, "fwd/16384/none/scale", 1, 3, 16384, "none", scale=True)
    elif group == "fwd_scalar":
        for HW in SCALAR:
            put(in_fwd, "fwd/%d/gelu" % HW, 1, 3, HW, "gelu")
        put(in_fwd, "fwd/4097/lrelu/res+scale", 1, 3, 4097, "lrelu", res=True, scale=True)
        put(in_fwd, "fwd/4096/gelu/x+1", 1, 3, 4096, "gelu", off=1)   # HW % 4 == 0, x not 16-byte aligned
    elif group == "fwd_bf16":
        for name in HALVES:
            with half(name) as dt:
                for HW in ALIGNED:
                    put(in_fwd_h, "fwd_h/%s/%d" % (name, HW), 1, planes_of(HW), HW, dt)
    elif group == "bwd":
        for HW in ALIGNED:
            for act in ("none", "gelu", "lrelu", "gelu_fast", "relu"):   # relu: in_bwd_launch's default branch
                put(in_bwd, "bwd/%d/%s" % (HW, act), 1, planes_of(HW), HW, act)
        for HW in SCALAR:
            put(in_bwd, "bwd/%d/gelu" % HW, 1, 3, HW, "gelu")
        for HW in (4100, 65536, 4097):
            put(in_bwd, "bwd/%d/gelu/extras" % HW, 1, planes_of(HW), HW, "gelu", extras=True)
    elif group == "bwd_h":
        for name in HALVES:
            with half(name) as dt:
                for HW in ALIGNED:
                    put(in_bwd_h, "bwd_h/%s/%d" % (name, HW), 1, planes_of(HW), HW, "gelu_fast", dt)
                put(in_bwd_h, "bwd_h/%s/4096/extras" % name, 1, 3, 4096, "gelu_fast", dt, extras=True)
    elif group == "ws":
        for N, C, HW in ((1, 2, 16384), (1, 1, 65540), (1, 128, 16384)):   # split, split, one workgroup per plane
            put(in_fwd, "fwd_ws/%d/%d/%d" % (N, C, HW), N, C, HW, "gelu", res=True, scale=True, ws=True)
            put(in_bwd, "bwd_ws/%d/%d/%d" % (N, C, HW), N, C, HW, "gelu", extras=True, ws=True)
    elif group == "mlp_bwd":
        lib = L.load()
        try:
            for mode in (2, 0):   # 2: mlp_bwd_dma_kernel (the default), 0: mlp_bwd_kernel<..., DMA = true>
                lib.dsgan_mlp_tune(0, mode)
                for name in HALVES:
                    with half(name) as dt:
                        put(mlp_bwd, "mlp_bwd/tune%d/%s" % (mode, name), dt)
        finally:
            lib.dsgan_mlp_tune(0, 2)
    else:
        raise ValueError(group)
    torch.cuda.synchronize()
    return out


GROUPS = ("fwd_aligned", "fwd_scalar", "fwd_bf16", "bwd", "bwd_h", "ws", "mlp_bwd")

if __name__ == "__main__":
    sys.path[:0] = [os.path.join(os.path.dirname(os.path.dirname(HERE)), "ds-gan_amd")]
    rec = {g: compute(g) for g in GROUPS}
    path = sys.argv[1] if len(sys.argv) > 1 else FIXTURE
    with open(path, "w") as f:
        json.dump(rec, f, indent=1, sort_keys=True)
        f.write("\n")
    print("wrote %s: %d digests" % (path, sum(len(v) for v in rec.values())))
