"""The tile plan of whole-frame colourisation without a GPU: origins, refusals, coverage, the blend window,
evaluate.py's refusal of a bad --tile_overlap, and the CPU reference blend against its own fp64 version."""
import os
import types

import pytest
import torch

from tiling_fixture import SHAPES, blend_ref, cover_count, random_tiles, weight2d


def _opt(**kw):
    o = types.SimpleNamespace(results_dir="epoch_8_result_original/", name="exp", phase="test_all/", which_epoch="8",
                              aspect_ratio=1.0, how_many=1000, fineSize_h=256, fineSize_w=256)
    for k, v in kw.items():
        setattr(o, k, v)
    return o


ORIGINS = [((64, 64, 16), [0]), ((100, 64, 16), [0, 36]), ((170, 64, 16), [0, 48, 96, 106]),
           ((97, 64, 32), [0, 32, 33]), ((128, 64, 0), [0, 64]), ((77, 32, 5), [0, 27, 45])]


@pytest.mark.parametrize("args,want", ORIGINS)
def test_tile_origins(args, want):
    from dsgan_hip.tiling import tile_origins
    got = tile_origins(*args)
    assert got == want and all(type(o) is int for o in got)


@pytest.mark.parametrize("args,names", [((63, 64, 16), ("63", "64")), ((100, 64, -1), ("-1",)), ((100, 64, 33), ("33", "32"))])
def test_tile_origins_refusals_name_the_values(args, names):
    from dsgan_hip.tiling import tile_origins
    with pytest.raises(ValueError) as e:
        tile_origins(*args)
    assert all(n in str(e.value) for n in names), str(e.value)


@pytest.mark.parametrize("args,want", ORIGINS)
def test_every_pixel_is_covered_by_one_to_three_tiles_per_axis(args, want):
    size, tile, _ = args
    cover = [sum(o <= p < o + tile for o in want) for p in range(size)]
    assert min(cover) >= 1 and max(cover) <= 3
    assert all(0 <= o and o + tile <= size for o in want) and want == sorted(set(want))


def test_nine_tiles_cover_a_pixel_at_97_64_32():
    from dsgan_hip.tiling import TilePlan
    plan = TilePlan(97, 97, 64, 64, 32)
    assert (plan.ny, plan.nx, plan.T) == (3, 3, 9) and plan.corner(5) == (32, 33)
    assert int(cover_count(plan).max()) == 9 and int(cover_count(plan).min()) == 1


def test_w1_window():
    from dsgan_hip.tiling import w1
    w = w1(64, 16)
    assert len(w) == 64 and w[0] == 1 and w[63] == 1 and w[:16] == list(range(1, 17)) and w[48:] == list(range(16, 0, -1))
    assert set(w[15:49]) == {16}
    assert w1(64, 0) == [1] * 64
    assert w1(5, 2) == [1, 2, 2, 2, 1]
    assert all(type(v) is int for v in w)


def test_tile_plan_refusals():
    from dsgan_hip.tiling import TilePlan
    with pytest.raises(ValueError, match="smaller than the 64x64 tile"):
        TilePlan(100, 63, 64, 64, 16)
    with pytest.raises(ValueError, match="overlap 17"):
        TilePlan(100, 100, 64, 32, 17)   # half of the smaller side bounds it
    p = TilePlan(101, 77, 64, 32, 5)
    assert (p.oy, p.ox, p.T) == ([0, 37], [0, 27, 45], 6)


def test_bad_tile_overlap_is_refused_before_any_directory_is_created(tmp_path):
    import evaluate as E
    with pytest.raises(ValueError, match="tile_overlap"):
        E.check_options(_opt(fineSize_h=64, fineSize_w=64), tile_overlap=33)
    with pytest.raises(ValueError, match="tile_overlap"):
        E.check_options(_opt(fineSize_h=64, fineSize_w=32), tile_overlap=-1)
    E.check_options(_opt(fineSize_h=64, fineSize_w=64), tile_overlap=32)
    E.check_options(_opt())   # without --full_frame the tile is not looked at
    out = tmp_path / "out"
    for bad in ("129", "-1"):   # the default tile is 256 x 256
        with pytest.raises(ValueError, match="tile_overlap"):
            E.main(["--dataroot", str(tmp_path / "none"), "--out", str(out), "--gpu_ids", "-1", "--full_frame",
                    "--tile_overlap", bad])
        assert not out.exists()
    # without --full_frame the flag is not read
    with pytest.raises(ValueError, match="aspect_ratio"):
        E.main(["--dataroot", str(tmp_path / "none"), "--out", str(out), "--gpu_ids", "-1", "--tile_overlap", "999",
                "--aspect_ratio", "2.0"])


def test_full_frame_results_dir():
    import evaluate as E
    base = E.results_dir(_opt(), "o")
    assert E.results_dir(_opt(), "o", full_frame=True) == base + "_full"
    assert E.results_dir(_opt(), "o", use_ema=True, full_frame=True) == base + "_full_ema"


@pytest.mark.parametrize("shape", SHAPES)
@pytest.mark.parametrize("C", [1, 3])
def test_reference_blend_fp32_agrees_with_fp64(shape, C):
    """9 products, 8 sums and one division at 2^-24 each on magnitudes <= 1: under 1.2e-6; bar 2e-6."""
    from dsgan_hip.tiling import TilePlan
    plan = TilePlan(*shape)
    tiles = random_tiles(plan, C, seed=11)
    r32, r64 = blend_ref(tiles, plan), blend_ref(tiles, plan, torch.float64)
    assert r32.dtype == torch.float32 and r32.shape == (C, plan.H, plan.W)
    err = float((r32.double() - r64).abs().max())
    print("shape %s C %d: fp32 reference vs fp64 %.3g" % (shape, C, err))
    assert err <= 2e-6
    assert float(r64.abs().max()) <= 1.0   # a weighted mean of values in [-1, 1]
    # weights and their sums are exact integers in fp32
    assert float(weight2d(plan).max()) == max(plan.overlap, 1) ** 2
    # a pixel that one tile covers is that tile's bits
    assert int(cover_count(plan)[0, 0]) == 1 and torch.equal(r32[:, 0, 0], tiles[0, :, 0, 0])


def test_reference_blend_special_cases():
    from dsgan_hip.tiling import TilePlan
    plan = TilePlan(64, 64, 64, 64, 16)
    tiles = random_tiles(plan, 3, seed=2)
    assert torch.equal(blend_ref(tiles, plan), tiles[0])
    plan = TilePlan(128, 128, 64, 64, 0)
    tiles = random_tiles(plan, 3, seed=3)
    want = torch.cat([torch.cat([tiles[0], tiles[1]], 2), torch.cat([tiles[2], tiles[3]], 2)], 1)
    assert torch.equal(blend_ref(tiles, plan), want)
    # a constant frame stays constant to rounding whatever the cover
    plan = TilePlan(97, 131, 64, 64, 32)
    out = blend_ref(torch.full((plan.T, 1, 64, 64), 0.3), plan)
    assert float((out - 0.3).abs().max()) <= 2e-6


def test_frame_dataset_serves_whole_frames_and_refuses_small_ones(tmp_path):
    import numpy as np
    from PIL import Image
    from data.frame_dataset import FrameDataset
    d = tmp_path / "data" / "test_all"
    os.makedirs(str(d))
    rng = np.random.default_rng(0)
    imgs = {}
    for name, (h, w) in (("a_0", (96, 80)), ("a_1", (64, 70)), ("b_0", (96, 80)), ("b_1", (64, 70))):
        imgs[name] = rng.integers(0, 256, (h, w, 3), dtype=np.uint8)
        Image.fromarray(imgs[name]).save(str(d / (name + ".png")))
    opt = types.SimpleNamespace(dataroot=str(tmp_path / "data"), phase="test_all/", dataset_mode="aligned", fineSize_h=64,
                                fineSize_w=64)
    ds = FrameDataset()
    ds.initialize(opt)
    assert len(ds) == 2
    for i in range(2):
        it = ds[i]
        assert it["A_paths"].endswith("a_%d.png" % i) and it["B_paths"].endswith("b_%d.png" % i)
        assert np.array_equal(it["A_u8"].numpy(), imgs["a_%d" % i]) and np.array_equal(it["B_u8"].numpy(), imgs["b_%d" % i])
    opt.dataset_mode, opt.dataroot = "single", str(d)
    ds = FrameDataset()
    ds.initialize(opt)
    assert len(ds) == 2 and set(ds[1]) == {"A_u8", "A_paths"} and ds[1]["A_u8"].shape == (64, 70, 3)
    opt.fineSize_w = 72
    with pytest.raises(ValueError, match=r"a_1\.png is 64x70"):
        ds[1]


def test_tile_entry_points_validate_on_the_host():
    """NULL pointers and inconsistent sizes are refused before any HIP call (no GPU here)."""
    from dsgan_hip import _lib
    if not os.path.exists(_lib.LIB_PATH):
        pytest.skip("libdsgan_hip.so not built (run __graft_entry__.build())")
    with pytest.raises(RuntimeError, match="dsgan_u8_tiles: bad args"):
        _lib.call("dsgan_u8_tiles", None, 64, 64, None, 1, None, 1, 64, 64, 0, 1, 0, None, None)
    with pytest.raises(RuntimeError, match=r"dsgan_u8_tiles: bad args \(frame 60x64, tile 64x64"):
        _lib.call("dsgan_u8_tiles", 16, 60, 64, 16, 1, 16, 1, 64, 64, 0, 1, 0, 16, None)
    with pytest.raises(RuntimeError, match=r"dsgan_tiles_blend: bad args .*overlap 33"):
        _lib.call("dsgan_tiles_blend", 16, 3, 64, 64, 16, 2, 16, 2, 33, 100, 100, 16, None)
    with pytest.raises(RuntimeError, match="dsgan_tiles_blend: bad args"):
        _lib.call("dsgan_tiles_blend", 16, 3, 64, 64, 16, 2000, 16, 2, 16, 100, 100, 16, None)
