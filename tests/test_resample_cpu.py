"""--load_resize on the CPU: the numpy integer model of Pillow's 8-bit resampler (dsgan_hip/resample.py)
against PIL.Image.resize byte for byte, the coefficient tables, the datasets' whole-frame items and the
host-side argument checks of dsgan_u8_resize_crop_to_image (no launch)."""
import math
import os
import random
from types import SimpleNamespace

import numpy as np
import pytest
import torch
from PIL import Image

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

PIL_FILTER = {"bicubic": Image.BICUBIC, "bilinear": Image.BILINEAR}
SHAPES = [((64, 80), (36, 44)), ((37, 53), (40, 48)), ((20, 20), (57, 63)), ((33, 47), (33, 20)),
          ((48, 48), (48, 48)), ((19, 23), (7, 5)), ((8, 8), (40, 48)), ((480, 640), (143, 191))]


def _image(kind, shape, seed):
    rng = np.random.default_rng(seed)
    if kind == "bytes":
        return rng.integers(0, 256, shape + (3,), dtype=np.uint8)
    return (rng.integers(0, 2, shape + (3,), dtype=np.uint8) * 255).astype(np.uint8)   # overshoot into both clamps


@pytest.mark.parametrize("kind", ["bytes", "0_255"])
@pytest.mark.parametrize("filt", ["bicubic", "bilinear"])
@pytest.mark.parametrize("src,out", SHAPES)
def test_model_equals_pillow(src, out, filt, kind):
    from dsgan_hip.resample import resize_u8_reference
    img = _image(kind, src, src[0] * 1000 + out[1])
    ref = np.asarray(Image.fromarray(img).resize((out[1], out[0]), PIL_FILTER[filt]))
    got = resize_u8_reference(img, out[0], out[1], filt)
    assert got.dtype == np.uint8 and got.shape == ref.shape
    assert np.array_equal(got, ref), int((got != ref).sum())


@pytest.mark.parametrize("filt,support", [("bicubic", 2.0), ("bilinear", 1.0)])
@pytest.mark.parametrize("n_in,n_out", [(80, 44), (53, 48), (20, 63), (23, 5), (640, 191), (640, 40), (8, 48)])
def test_pil_coeffs_tables(n_in, n_out, filt, support):
    from dsgan_hip.resample import pil_coeffs
    bounds, coef = pil_coeffs(n_in, n_out, filt)
    ksize = int(math.ceil(support * max(n_in / n_out, 1.0))) * 2 + 1
    assert bounds.dtype == np.int32 and coef.dtype == np.int32
    assert bounds.shape == (n_out, 2) and coef.shape == (n_out, ksize)
    for (lo, n), k in zip(bounds, coef):
        assert 0 <= lo and 1 <= n <= ksize and lo + n <= n_in
        assert not k[n:].any()                        # the tail is zero-filled
        assert abs(int(k.sum()) - (1 << 22)) <= n      # normalised weights, each rounded by at most 1/2
    assert (np.diff(bounds[:, 0]) >= 0).all()          # windows ascend with the output index


def test_pil_coeffs_refuses_more_than_16x():
    from dsgan_hip.resample import pil_coeffs
    assert pil_coeffs(640, 40, "bicubic")[1].shape[1] == 65      # 16x exactly: the 65-tap window
    with pytest.raises(ValueError, match=r"641 .*16x .*40 .*65 taps"):
        pil_coeffs(641, 40, "bicubic")
    with pytest.raises(ValueError, match="filter"):
        pil_coeffs(64, 40, "lanczos")


def _write_pairs(d, n, shape_a, shape_b, seed=0):
    rng = np.random.default_rng(seed)
    os.makedirs(d, exist_ok=True)
    imgs = {}
    for i in range(n):
        for side, (H, W) in (("a", shape_a), ("b", shape_b)):
            arr = rng.integers(0, 256, (H, W, 3), dtype=np.uint8)
            p = os.path.join(d, "%s_%03d.png" % (side, i))
            Image.fromarray(arr).save(p)
            imgs[p] = arr
    return imgs


def _opt(root, **kw):
    o = dict(dataroot=str(root), phase="train_all", resize_or_crop="resize_and_crop", loadSize_w=48, fineSize_w=32,
             loadSize_h=40, fineSize_h=24, no_flip=False)
    o.update(kw)
    return SimpleNamespace(**o)


def test_aligned_dataset_whole_frames_same_draws(tmp_path):
    """Flag on: whole frames, and the (w_off, h_off, flip) sequence of the flag-off dataset under one seed.
    Flag none (or absent): today's items."""
    from data.aligned_dataset import AlignedDataset
    from data.image_folder import make_dataset
    imgs = _write_pairs(str(tmp_path / "train_all"), 3, (50, 64), (44, 60))
    A, B = make_dataset(str(tmp_path / "train_all"))
    on, off, absent = AlignedDataset(), AlignedDataset(), AlignedDataset()
    on.initialize(_opt(tmp_path, load_resize="bicubic"))
    off.initialize(_opt(tmp_path, load_resize="none"))
    absent.initialize(_opt(tmp_path))
    random.seed(11)
    items_on = [on[i] for i in (0, 1, 2, 1)]
    random.seed(11)
    items_off = [off[i] for i in (0, 1, 2, 1)]
    random.seed(11)
    items_absent = [absent[i] for i in (0, 1, 2, 1)]
    random.seed(11)
    for i, a, b, c in zip((0, 1, 2, 1), items_on, items_off, items_absent):
        wo, ho = random.randint(0, 48 - 32 - 1), random.randint(0, 40 - 24 - 1)
        fl = int(random.random() < 0.5)
        assert (a["w_off"], a["h_off"], a["flip"]) == (wo, ho, fl)
        assert sorted(a) == ["A_frame", "A_paths", "B_frame", "B_paths", "flip", "h_off", "w_off"]
        assert a["A_frame"].dtype == torch.uint8
        assert np.array_equal(a["A_frame"].numpy(), imgs[A[i]]) and np.array_equal(a["B_frame"].numpy(), imgs[B[i]])
        for it in (b, c):   # today's items: host crops of the decoded files
            assert sorted(it) == ["A_paths", "A_u8", "B_paths", "B_u8", "flip"]
            assert it["flip"] == fl and (it["A_paths"], it["B_paths"]) == (A[i], B[i])
            assert np.array_equal(it["A_u8"].numpy(), imgs[A[i]][ho:ho + 24, wo:wo + 32])
            assert np.array_equal(it["B_u8"].numpy(), imgs[B[i]][ho:ho + 24, wo:wo + 32])


def test_single_dataset_whole_frames(tmp_path):
    from data.single_dataset import SingleDataset
    imgs = _write_pairs(str(tmp_path), 2, (50, 64), (50, 64))
    on, off = SingleDataset(), SingleDataset()
    on.initialize(_opt(tmp_path, load_resize="bilinear"))
    off.initialize(_opt(tmp_path, load_resize="none"))
    random.seed(3)
    a = on[1]
    random.seed(3)
    wo, ho = random.randint(0, 48 - 32), random.randint(0, 40 - 24)
    assert (a["w_off"], a["h_off"], a["flip"]) == (wo, ho, 0)
    assert np.array_equal(a["A_frame"].numpy(), imgs[a["A_paths"]])
    random.seed(3)
    b = off[1]
    random.seed(3)
    wo, ho = random.randint(0, 64 - 32), random.randint(0, 50 - 24)
    assert sorted(b) == ["A_paths", "A_u8", "flip"]
    assert np.array_equal(b["A_u8"].numpy(), imgs[b["A_paths"]][ho:ho + 24, wo:wo + 32])


def test_collate_names_two_files_of_different_size(tmp_path):
    from data import collate_frames
    from data.aligned_dataset import AlignedDataset
    _write_pairs(str(tmp_path / "train_all"), 2, (50, 64), (44, 60))
    odd = str(tmp_path / "train_all" / "b_001.png")
    Image.fromarray(np.zeros((44, 62, 3), dtype=np.uint8)).save(odd)
    ds = AlignedDataset()
    ds.initialize(_opt(tmp_path, load_resize="bicubic"))
    items = [ds[0], ds[1]]
    with pytest.raises(ValueError) as e:
        collate_frames(items)
    assert "b_000.png" in str(e.value) and "b_001.png" in str(e.value) and "44x60" in str(e.value) and "44x62" in str(e.value)
    batch = collate_frames([ds[0], ds[0]])
    assert batch["A_frame"].shape == (2, 50, 64, 3) and batch["B_frame"].shape == (2, 44, 60, 3)
    assert batch["h_off"].shape == (2,) and len(batch["A_paths"]) == 2


@pytest.mark.parametrize("kw", [dict(loadSize_w=31), dict(loadSize_h=23)])
def test_load_smaller_than_fine_is_refused(tmp_path, kw):
    from data.aligned_dataset import AlignedDataset
    from data.single_dataset import SingleDataset
    _write_pairs(str(tmp_path / "train_all"), 1, (50, 64), (50, 64))
    o = _opt(tmp_path, load_resize="bicubic", **kw)
    for cls in (AlignedDataset, SingleDataset):
        with pytest.raises(ValueError, match=r"loadSize %dx%d .*fineSize 24x32" % (o.loadSize_h, o.loadSize_w)):
            cls().initialize(o)


def test_flag_is_a_build_flag_of_both_option_sets():
    from options.test_options import TestOptions
    from options.train_options import TrainOptions
    assert TrainOptions().gather_options([]).load_resize == "none"
    assert TestOptions().gather_options(["--load_resize", "bilinear"]).load_resize == "bilinear"
    with pytest.raises(SystemExit):
        TrainOptions().gather_options(["--load_resize", "lanczos"])


def test_full_frame_refuses_load_resize():
    import evaluate as E
    from options.test_options import TestOptions
    opt = TestOptions().gather_options(["--load_resize", "bicubic"])
    with pytest.raises(ValueError, match=r"--full_frame.*--load_resize bicubic"):
        E.check_options(opt, tile_overlap=32)
    E.check_options(opt)   # the crop pass takes the flag


def test_wrapper_validates_on_the_host():
    """Every refusal comes before the first device call, so it shows on a machine without a GPU."""
    from dsgan_hip.resample import resize_crop_to_image, tmp_bytes
    u8 = torch.zeros(2, 40, 52, 3, dtype=torch.uint8)
    for offs in ([(0, 0), (17, 0)], [(0, 0), (0, 17)], [(-1, 0), (0, 0)], [(0, 0), (0, -1)]):
        with pytest.raises(ValueError, match="crop offset"):
            resize_crop_to_image(u8, 40, 48, offs, [0, 0], 24, 32)
    with pytest.raises(ValueError, match="1 offsets"):
        resize_crop_to_image(u8, 40, 48, [(0, 0)], [0, 0], 24, 32)
    with pytest.raises(ValueError, match="smaller than fineSize"):
        resize_crop_to_image(u8, 40, 48, [(0, 0), (0, 0)], [0, 0], 41, 32)
    with pytest.raises(ValueError, match=r"width of 52 .*16x .*load size 3 .*65 taps"):
        resize_crop_to_image(u8, 40, 3, [(0, 0), (0, 0)], [0, 0], 24, 2)
    with pytest.raises(ValueError, match="uint8"):
        resize_crop_to_image(u8.float(), 40, 48, [(0, 0), (0, 0)], [0, 0], 24, 32)
    assert tmp_bytes(2, 40, 32, 5) == 2 * 40 * 32 * 3 and tmp_bytes(2, 40, 32, 0) == 0


def test_entry_point_refuses_bad_args_without_a_launch():
    from dsgan_hip import _lib
    if not os.path.exists(_lib.LIB_PATH):
        pytest.skip("libdsgan_hip.so not built (run __graft_entry__.build())")
    name = "dsgan_u8_resize_crop_to_image"
    p = 4096   # never dereferenced: every case below is refused on the host

    def args(src=p, N=2, Hs=40, Ws=52, yb=None, yc=None, ky=0, xb=p, xc=p, kx=5, load_h=40, load_w=48, off=p, flip=p,
             fh=24, fw=32, gray=0, tmp=p, tmp_bytes=2 * 40 * 32 * 3, dst=p):
        return (src, N, Hs, Ws, yb, yc, ky, xb, xc, kx, load_h, load_w, off, flip, fh, fw, gray, tmp, tmp_bytes, dst, None)

    for kw in (dict(src=None), dict(off=None), dict(flip=None), dict(dst=None)):
        with pytest.raises(RuntimeError, match="null"):
            _lib.call(name, *args(**kw))
    with pytest.raises(RuntimeError, match="crop 24x49 larger than the load size 40x48"):
        _lib.call(name, *args(fw=49, tmp_bytes=1 << 30))
    with pytest.raises(RuntimeError, match="tmp of 7679 bytes, this call needs 7680"):
        _lib.call(name, *args(tmp_bytes=2 * 40 * 32 * 3 - 1))
    with pytest.raises(RuntimeError, match="tmp of 0 bytes"):
        _lib.call(name, *args(tmp=None))
    with pytest.raises(RuntimeError, match="bad tables"):
        _lib.call(name, *args(xb=None))           # a table is missing
    with pytest.raises(RuntimeError, match="bad tables"):
        _lib.call(name, *args(Hs=41))             # no vertical table, yet the height changes
    with pytest.raises(RuntimeError, match="bad tables"):
        _lib.call(name, *args(kx=66))
