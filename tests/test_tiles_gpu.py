"""dsgan_u8_tiles and dsgan_tiles_blend against ``data.to_images`` of host crops and the torch-CPU reference
blend of tests/tiling_fixture.py: bit-exact in fp32, within 2e-6 of the fp64 reference (9 products, 8 sums
and one division at 2^-24 each on magnitudes <= 1 stay under 1.2e-6)."""
import numpy as np
import pytest
import torch

from tiling_fixture import SHAPES, blend_ref, cover_count, crops, random_tiles

pytestmark = pytest.mark.gpu
DEV = "cuda"
# W, tw and every x origin (0, 48, 96, 104) multiples of 4 with up to three tiles on a column: the float4 /
# dword paths of both kernels on more than one tile per axis
ALIGNED = (100, 168, 64, 64, 16)


def _plan(shape):
    from dsgan_hip.tiling import TilePlan
    return TilePlan(*shape)


def _frame(H, W, seed):
    """A uint8 frame that holds all 256 byte values in every channel."""
    rng = np.random.default_rng(seed)
    f = rng.integers(0, 256, (H, W, 3), dtype=np.uint8)
    f.reshape(-1, 3)[:256] = np.arange(256, dtype=np.uint8)[:, None]
    f.reshape(-1, 3)[:256, 1] = np.arange(255, -1, -1, dtype=np.uint8)
    return f


def _bits(a, b):
    return a.shape == b.shape and torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


@pytest.fixture(scope="module")
def refs():
    """Per (shape, C): random tiles in [-1, 1] with their fp32 and fp64 CPU blends, computed once."""
    out = {}
    for shape in SHAPES:
        plan = _plan(shape)
        for C in (1, 3):
            tiles = random_tiles(plan, C, seed=5 + C)
            out[shape, C] = (tiles, blend_ref(tiles, plan), blend_ref(tiles, plan, torch.float64))
    return out


@pytest.mark.parametrize("shape", SHAPES + [ALIGNED])
@pytest.mark.parametrize("gray", [False, True])
def test_u8_tiles_bit_exact_with_to_images_of_crops(shape, gray):
    from data import to_images
    from dsgan_hip import tiling
    plan = _plan(shape)
    frame = _frame(plan.H, plan.W, seed=1)
    assert all(len(np.unique(frame[..., c])) == 256 for c in range(3))
    dev = torch.from_numpy(frame).to(DEV)
    got = tiling.frame_tiles(dev, plan, gray=gray)
    want = to_images(torch.from_numpy(crops(frame, plan)), [0] * plan.T, gray)
    assert got.shape == (plan.T, 1 if gray else 3, plan.th, plan.tw) and _bits(got, want)
    # a range of tiles is the same slice of the whole
    for t0, T in ((0, 1), (plan.T - 1, 1), (plan.T // 2, plan.T - plan.T // 2)):
        assert _bits(tiling.frame_tiles(dev, plan, t0, T, gray), want[t0:t0 + T]), (t0, T)


@pytest.mark.parametrize("shape", SHAPES)
@pytest.mark.parametrize("C", [1, 3])
def test_tiles_blend_vs_reference(refs, shape, C):
    from dsgan_hip import tiling
    plan = _plan(shape)
    tiles, r32, r64 = refs[shape, C]
    got = tiling.blend(tiles.to(DEV), plan).cpu()
    assert got.shape == (C, plan.H, plan.W)
    err = float((got.double() - r64).abs().max())
    print("shape %s C %d: max |kernel - fp64 reference| %.3g, bit mismatches vs fp32 reference %d"
          % (shape, C, err, int((got.view(torch.int32) != r32.view(torch.int32)).sum())))
    assert _bits(got, r32)
    assert err <= 2e-6
    # pixels that one tile covers are that tile's bits
    cnt = cover_count(plan)
    for t in range(plan.T):
        y0, x0 = plan.corner(t)
        m = (cnt[y0:y0 + plan.th, x0:x0 + plan.tw] == 1).expand(C, -1, -1)
        assert _bits(got[:, y0:y0 + plan.th, x0:x0 + plan.tw][m], tiles[t][m]), t
    # identical calls give identical bits
    assert _bits(tiling.blend(tiles.to(DEV), plan).cpu(), got)


def test_tiles_blend_overlap_zero_is_the_concatenation(refs):
    from dsgan_hip import tiling
    plan = _plan((128, 128, 64, 64, 0))
    tiles = refs[(128, 128, 64, 64, 0), 3][0]
    want = torch.cat([torch.cat([tiles[0], tiles[1]], 2), torch.cat([tiles[2], tiles[3]], 2)], 1)
    assert _bits(tiling.blend(tiles.to(DEV), plan).cpu(), want)


def test_tiles_blend_of_one_tile_is_the_tile(refs):
    from dsgan_hip import tiling
    plan = _plan((64, 64, 64, 64, 16))
    for C in (1, 3):
        tiles = refs[(64, 64, 64, 64, 16), C][0]
        assert _bits(tiling.blend(tiles.to(DEV), plan).cpu(), tiles[0])


@pytest.mark.parametrize("shape", SHAPES)
def test_blend_of_a_frames_own_tiles_is_the_frame(shape):
    from data import to_images
    from dsgan_hip import tiling
    plan = _plan(shape)
    frame = torch.from_numpy(_frame(plan.H, plan.W, seed=2)).to(DEV)
    for gray in (False, True):
        got = tiling.blend(tiling.frame_tiles(frame, plan, gray=gray), plan)
        want = to_images(frame[None], [0], gray)[0]
        err = float((got - want).abs().max())
        print("shape %s gray %d: identity error %.3g" % (shape, gray, err))
        assert err <= 2e-6


def test_tiles_blend_vector_and_scalar_paths_give_the_same_bits():
    """Tiles at a 4-byte (not 16-byte) aligned address go pixel by pixel, aligned ones four at a time: both
    are the reference's bits, on a plan whose columns carry up to three tiles."""
    from dsgan_hip import functional as HF
    plan = _plan(ALIGNED)
    tiles = random_tiles(plan, 3, seed=9)
    want = blend_ref(tiles, plan)
    buf = torch.empty(tiles.numel() + 1, device=DEV)
    off = buf[1:].view(tiles.shape)
    off.copy_(tiles)
    assert off.data_ptr() % 16 == 4 and off.is_contiguous()
    oy, ox = plan.device_origins(DEV)
    assert _bits(HF.tiles_blend(off, oy, ox, plan.overlap, plan.H, plan.W).cpu(), want)
    assert _bits(HF.tiles_blend(tiles.to(DEV), oy, ox, plan.overlap, plan.H, plan.W).cpu(), want)


def test_bad_arguments_raise_without_a_launch():
    from dsgan_hip import functional as HF
    frame = torch.zeros(70, 70, 3, dtype=torch.uint8, device=DEV)
    tiles = torch.zeros(4, 3, 64, 64, device=DEV)
    o = [0, 6]
    with pytest.raises(RuntimeError, match="dsgan_u8_tiles: bad args"):
        HF.u8_tiles(frame, o, o, 64, 64, 3, 2)             # the range runs past the plan's 4 tiles
    with pytest.raises(RuntimeError, match="dsgan_u8_tiles: bad args"):
        HF.u8_tiles(frame, o, o, 64, 64, 0, 0)             # no tiles
    with pytest.raises(RuntimeError, match="dsgan_u8_tiles: bad args"):
        HF.u8_tiles(frame, o, o, 71, 64)                   # a tile larger than the frame
    with pytest.raises(ValueError, match="uint8"):
        HF.u8_tiles(frame.float(), o, o, 64, 64)
    with pytest.raises(RuntimeError, match="dsgan_tiles_blend: bad args"):
        HF.tiles_blend(tiles, o, o, 33, 70, 70)            # overlap above half a tile
    with pytest.raises(RuntimeError, match="dsgan_tiles_blend: bad args"):
        HF.tiles_blend(tiles, o, o, 16, 63, 70)            # a frame smaller than the tile
    with pytest.raises(RuntimeError, match="dsgan_tiles_blend: bad args"):
        HF.tiles_blend(tiles, o, o, 16, 0, 70)             # zero-size frame
    with pytest.raises(RuntimeError, match="dsgan_tiles_blend: bad args"):
        HF.tiles_blend(torch.zeros(4, 2, 64, 64, device=DEV), o, o, 16, 70, 70)   # two channels
    with pytest.raises(ValueError, match="3 tiles"):
        HF.tiles_blend(tiles[:3], o, o, 16, 70, 70)        # tiles that are not the plan's
    torch.cuda.synchronize()
