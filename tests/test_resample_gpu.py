"""--load_resize on the GPU: dsgan_u8_resize_crop_to_image against the numpy integer model and against Pillow
(asserted separately: a Pillow change and a kernel bug read differently), the loader with the flag on against
the reference pipeline written out in torch on the CPU, and train.py on raw frames with the flag against the
same run on frames resized offline by PIL.  Every comparison is bit for bit."""
import os
import random

import numpy as np
import pytest
import torch
from PIL import Image

pytestmark = pytest.mark.gpu

PIL_FILTER = {"bicubic": Image.BICUBIC, "bilinear": Image.BILINEAR}
# (source) -> (load) -> (fine), all (h, w)
GEOMETRIES = [((37, 53), (40, 48), (24, 32)),      # odd row pitch
              ((64, 80), (36, 44), (24, 32)),
              ((33, 47), (33, 20), (33, 16)),      # vertical axis unchanged
              ((47, 33), (20, 33), (16, 33)),      # horizontal axis unchanged, fw odd
              ((20, 20), (57, 63), (57, 63)),      # crop = load
              ((120, 160), (72, 72), (64, 62))]    # fw no multiple of 4
FLIPS = [0, 1, 0]


def _frames(kind, shape, seed):
    rng = np.random.default_rng(seed)
    if kind == "bytes":
        return rng.integers(0, 256, (3,) + shape + (3,), dtype=np.uint8)
    return (rng.integers(0, 2, (3,) + shape + (3,), dtype=np.uint8) * 255).astype(np.uint8)


def _offsets(load, fine):
    dh, dw = load[0] - fine[0], load[1] - fine[1]
    return [(0, 0), (dh, dw), (dh // 2, (dw + 1) // 2)]


def _expect(resized, offsets, fine, gray):
    """numpy crop -> the existing to_images on that crop"""
    from data import to_images
    crops = np.stack([r[ho:ho + fine[0], wo:wo + fine[1]] for r, (ho, wo) in zip(resized, offsets)])
    return to_images(torch.from_numpy(crops), FLIPS, gray)


@pytest.mark.parametrize("kind", ["bytes", "0_255"])
@pytest.mark.parametrize("gray", [0, 1])
@pytest.mark.parametrize("filt", ["bicubic", "bilinear"])
@pytest.mark.parametrize("src,load,fine", GEOMETRIES)
def test_kernel_equals_model_and_pillow(src, load, fine, filt, gray, kind):
    from dsgan_hip.resample import resize_crop_to_image, resize_u8_reference
    frames = _frames(kind, src, src[0] * 100 + load[1])
    offsets = _offsets(load, fine)
    got = resize_crop_to_image(torch.from_numpy(frames), load[0], load[1], offsets, FLIPS, fine[0], fine[1], bool(gray), filt)
    assert got.shape == (3, 1 if gray else 3, fine[0], fine[1]) and got.dtype == torch.float32
    model = _expect([resize_u8_reference(f, load[0], load[1], filt) for f in frames], offsets, fine, bool(gray))
    assert torch.equal(got, model), "kernel != numpy integer model"
    pil = _expect([np.asarray(Image.fromarray(f).resize((load[1], load[0]), PIL_FILTER[filt])) for f in frames],
                  offsets, fine, bool(gray))
    assert torch.equal(got, pil), "kernel != PIL.Image.resize"


@pytest.mark.parametrize("gray", [0, 1])
@pytest.mark.parametrize("load,fine", [((40, 52), (24, 32)), ((37, 53), (21, 30)), ((32, 32), (32, 32))])
def test_unchanged_axes_equal_to_images_on_the_host_crop(load, fine, gray):
    """Frames already at the load size: no pass, crop + convert only, dsgan_u8_to_image's bits."""
    from dsgan_hip.resample import resize_crop_to_image
    frames = _frames("bytes", load, 7)
    offsets = _offsets(load, fine)
    got = resize_crop_to_image(torch.from_numpy(frames), load[0], load[1], offsets, FLIPS, fine[0], fine[1], bool(gray))
    assert torch.equal(got, _expect(frames, offsets, fine, bool(gray)))


@pytest.mark.parametrize("filt,gray", [("bicubic", False), ("bilinear", False), ("bicubic", True)])
def test_loader_equals_reference_pipeline(tmp_path, filt, gray):
    """CreateDataLoader with --load_resize == Image.resize, then the reference's torch CPU transforms: ToTensor
    (/255), crop, Normalize(0.5, 0.5), flip, RGB->gray (the expectation of tests/test_eval_gpu.py with the resize
    in front).  A frames are 40x52, B frames 44x60 (h x w)."""
    from data import CreateDataLoader
    from options.train_options import default_train_opt
    rng = np.random.default_rng(1)
    d = tmp_path / "train_all"
    d.mkdir()
    for i in range(4):
        for side, shape in (("a", (40, 52)), ("b", (44, 60))):
            Image.fromarray(rng.integers(0, 256, shape + (3,), dtype=np.uint8)).save(str(d / ("%s_%d.png" % (side, i))))
    opt = default_train_opt(gpu_ids=[0], dataroot=str(tmp_path), phase="train_all", loadSize_w=48, fineSize_w=32,
                            loadSize_h=40, fineSize_h=24, batchSize=2, nThreads=0, serial_batches=True,
                            input_nc=1 if gray else 3, load_resize=filt)
    loader = CreateDataLoader(opt, "train").load_data()
    random.seed(9)
    batches = list(loader)
    assert len(batches) == 2
    random.seed(9)
    for bi, data in enumerate(batches):
        assert sorted(data) == ["A", "A_paths", "B", "B_paths", "global_batch"] and data["global_batch"] == 2
        for j in range(2):
            k = 2 * bi + j
            wo, ho = random.randint(0, 48 - 32 - 1), random.randint(0, 40 - 24 - 1)
            flip = random.random() < 0.5
            for side, key, g in (("a", "A", gray), ("b", "B", False)):
                img = Image.open(str(d / ("%s_%d.png" % (side, k)))).convert("RGB").resize((48, 40), PIL_FILTER[filt])
                t = torch.from_numpy(np.array(img)).permute(2, 0, 1).contiguous().float().div(255)
                t = t[:, ho:ho + 24, wo:wo + 32]
                m = torch.tensor([0.5, 0.5, 0.5])[:, None, None]
                t = t.sub(m).div(m)
                if flip:
                    t = t.index_select(2, torch.arange(31, -1, -1))
                if g:
                    t = (t[0] * 0.299 + t[1] * 0.587 + t[2] * 0.114).unsqueeze(0)
                got = data[key][j].cpu()
                assert got.shape == t.shape and torch.equal(got, t), (k, key)


def test_single_dataset_loader_equals_reference_pipeline(tmp_path):
    """--dataset_mode single with the flag: the A half, resized, cropped at offsets drawn over load - fine, unflipped."""
    from data import CreateDataLoader
    from options.test_options import default_test_opt
    rng = np.random.default_rng(4)
    for i in range(4):   # make_dataset serves the first half of the sorted walk
        Image.fromarray(rng.integers(0, 256, (40, 52, 3), dtype=np.uint8)).save(str(tmp_path / ("a_%d.png" % i)))
    opt = default_test_opt(gpu_ids=[0], dataroot=str(tmp_path), loadSize_w=48, fineSize_w=32, loadSize_h=44,
                           fineSize_h=24, batchSize=2, nThreads=0, load_resize="bilinear")
    random.seed(6)
    batches = list(CreateDataLoader(opt, "test").load_data())
    assert len(batches) == 1 and sorted(batches[0]) == ["A", "A_paths", "global_batch"]
    random.seed(6)
    for j in range(2):
        wo, ho = random.randint(0, 48 - 32), random.randint(0, 44 - 24)
        img = Image.open(str(tmp_path / ("a_%d.png" % j))).convert("RGB").resize((48, 44), Image.BILINEAR)
        t = torch.from_numpy(np.array(img)).permute(2, 0, 1).contiguous().float().div(255)[:, ho:ho + 24, wo:wo + 32]
        m = torch.tensor([0.5, 0.5, 0.5])[:, None, None]
        assert torch.equal(batches[0]["A"][j].cpu(), t.sub(m).div(m)), j


def test_train_on_raw_frames_equals_train_on_pil_resized_frames(tmp_path):
    """What a user who used to resize offline expects: one epoch of train.py on four 40x48 (h x w) pairs with
    --load_resize bicubic, load 36, fine 32, ends with the generator and discriminator weights of the same run on
    the pairs resized to 36x36 by PIL beforehand with the flag none, bit for bit."""
    import train as T
    rng = np.random.default_rng(3)
    raw, pre = tmp_path / "raw" / "train_all", tmp_path / "pre" / "train_all"
    raw.mkdir(parents=True)
    pre.mkdir(parents=True)
    for i in range(4):
        for side in ("a", "b"):
            img = Image.fromarray(rng.integers(0, 256, (40, 48, 3), dtype=np.uint8))
            img.save(str(raw / ("%s_%d.png" % (side, i))))
            img.resize((36, 36), Image.BICUBIC).save(str(pre / ("%s_%d.png" % (side, i))))

    def run(root, out, flag):
        T.main(["--dataroot", str(tmp_path / root), "--out", str(tmp_path / out), "--gpu_ids", "0", "--batchSize", "2",
                "--nThreads", "0", "--niter", "1", "--niter_decay", "0", "--precision", "fp32", "--pool_size", "0",
                "--loadSize_w", "36", "--loadSize_h", "36", "--fineSize_w", "32", "--fineSize_h", "32",
                "--load_resize", flag], output_freq=1)
        ck = tmp_path / out / "checkpoints" / "experiment_name"
        return [torch.load(str(ck / n), map_location="cpu", weights_only=True)
                for n in ("1_useSE_net_G.pth", "1_useSE_net_D.pth")]

    on, off = run("raw", "out_on", "bicubic"), run("pre", "out_off", "none")
    for x, y in zip(on, off):
        assert list(x) == list(y) and len(x) > 0
        assert all(torch.equal(x[k], y[k]) for k in x)
