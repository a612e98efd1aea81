"""Torch-CPU reference of the tile blend (dsgan_tiles_blend's defined arithmetic) for the tiling tests.

Per pixel and channel: num = sum fl(w * v) and den = sum w over the covering tiles, iy ascending then ix
ascending, out = num / den, all in ``dtype``; a pixel that exactly one tile covers takes that tile's value,
copied.  w = wy(i) * wx(j) with the integer ramp ``tiling.w1``.  torch's CPU multiply and add are separate
roundings (no FMA), which is the order the kernel is defined in."""
import torch

from dsgan_hip import tiling

# (H, W, th, tw, overlap): up to 9 tiles on a pixel, odd sizes, a non-square tile, one clamped row, the
# frame that is the tile, and overlap 0 on a frame the tile divides
SHAPES = [(97, 131, 64, 64, 32), (100, 170, 64, 64, 16), (101, 77, 64, 32, 5), (65, 64, 64, 64, 16),
          (64, 64, 64, 64, 16), (128, 128, 64, 64, 0)]


def weight2d(plan, dtype=torch.float32):
    wy = torch.tensor(tiling.w1(plan.th, plan.overlap), dtype=dtype)
    wx = torch.tensor(tiling.w1(plan.tw, plan.overlap), dtype=dtype)
    return wy[:, None] * wx[None, :]


def cover_count(plan):
    cnt = torch.zeros(plan.H, plan.W, dtype=torch.int32)
    for y0 in plan.oy:
        for x0 in plan.ox:
            cnt[y0:y0 + plan.th, x0:x0 + plan.tw] += 1
    return cnt


def blend_ref(tiles, plan, dtype=torch.float32):
    """tiles: CPU [T, C, th, tw] -> [C, H, W] in ``dtype``."""
    tiles = tiles.to(dtype)
    C = tiles.shape[1]
    w = weight2d(plan, dtype)
    num = torch.zeros(C, plan.H, plan.W, dtype=dtype)
    one = torch.zeros(C, plan.H, plan.W, dtype=dtype)
    den = torch.zeros(plan.H, plan.W, dtype=dtype)
    for iy, y0 in enumerate(plan.oy):
        for ix, x0 in enumerate(plan.ox):
            v = tiles[iy * plan.nx + ix]
            ys, xs = slice(y0, y0 + plan.th), slice(x0, x0 + plan.tw)
            num[:, ys, xs] += w * v     # fl(w * v) first, then the add
            den[ys, xs] += w
            one[:, ys, xs] = v
    out = num / den
    single = (cover_count(plan) == 1).expand(C, -1, -1)
    out[single] = one[single]
    return out


def random_tiles(plan, C, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.rand(plan.T, C, plan.th, plan.tw, generator=g) * 2 - 1


def crops(frame_u8, plan):
    """The plan's windows of a uint8 [H, W, 3] numpy frame, stacked in tile order."""
    import numpy as np
    return np.stack([frame_u8[y0:y0 + plan.th, x0:x0 + plan.tw] for y0 in plan.oy for x0 in plan.ox])
