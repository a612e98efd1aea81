"""The evaluation kernels (csrc/evalimg.hip) against the CPU oracle: the batched skimage-style SSIM + PSNR,
the uint8 panels, the per-image gaussian SSIM behind ``MS_SSIM.ssim(size_average=False)`` and
``util.metrics.EvalMetrics``.

Tolerances are the project's: |d ssim| < 1e-5 and |d psnr| < 1e-4 for the uint8 metrics
(tests/test_eval_gpu.py::test_train_loop_metrics_vs_oracle), 2e-5 for the fp32 gaussian SSIM / MS-SSIM
(tests/test_eval_gpu.py); the panels are bit-exact."""
import numpy as np
import pytest
import torch

from oracle import dsgan_cpu as O

pytestmark = pytest.mark.gpu
DEV = "cuda"

# one window; smaller than a tile; partial tiles in both directions; 2x2 full-ish tiles
METRIC_SHAPES = [(2, 3, 7, 7), (3, 3, 23, 40), (2, 1, 39, 70), (1, 3, 64, 64)]


def _pair(shape):
    """label in [-1.2, 1.2] and a noisy result: both sides of the uint8 clip are exercised."""
    g = torch.Generator().manual_seed(sum(shape))
    real = torch.rand(shape, generator=g) * 2.4 - 1.2
    fake = real + 0.3 * torch.randn(shape, generator=g)
    return fake, real


def _oracle(fake, real):
    out = []
    for n in range(fake.shape[0]):
        lab, res = O.to_u8_hwc(real[n]), O.to_u8_hwc(fake[n])
        out.append((O.sk_ssim(lab, res), float(O.cal_psnr(lab, res))))
    return out


def _check(got, ref):
    got = got.cpu().tolist()
    assert len(got) == len(ref)
    for n, ((s, p), (rs, rp)) in enumerate(zip(got, ref)):
        print("image %d: ssim %.8f vs %.8f, psnr %.6f vs %.6f" % (n, s, rs, p, rp))
        assert np.isfinite(rs) and np.isfinite(rp)
        assert abs(s - rs) < 1e-5, (n, s, rs)
        assert abs(p - rp) < 1e-4, (n, p, rp)


@pytest.mark.parametrize("shape", METRIC_SHAPES)
def test_img_metrics_batch_vs_oracle(shape):
    from dsgan_hip import functional as HF
    fake, real = _pair(shape)
    got = HF.img_metrics_batch(fake.to(DEV), real.to(DEV))
    assert got.shape == (shape[0], 2) and got.dtype == torch.float32
    _check(got, _oracle(fake, real))


def test_img_metrics_batch_identical_and_constant():
    from dsgan_hip import functional as HF
    _, real = _pair((2, 3, 39, 45))
    got = HF.img_metrics_batch(real.to(DEV), real.to(DEV)).cpu()
    assert torch.equal(got, torch.tensor([[1.0, 100.0]] * 2)), got
    fake = torch.full((2, 3, 39, 45), 0.2)
    real = torch.full((2, 3, 39, 45), -0.4)
    real[1] = 0.2 + 1e-4   # quantises to the same uint8 value: psnr 100
    got = HF.img_metrics_batch(fake.to(DEV), real.to(DEV))
    _check(got, _oracle(fake, real))
    assert got[1, 1].item() == 100.0


@pytest.mark.parametrize("shape", [(3, 3, 23, 40), (2, 1, 39, 70), (2, 3, 64, 64)])
def test_img_metrics_batch_is_deterministic_and_batch_independent(shape):
    from dsgan_hip import functional as HF
    fake, real = (t.to(DEV) for t in _pair(shape))
    a = HF.img_metrics_batch(fake, real)
    b = HF.img_metrics_batch(fake, real)
    assert torch.equal(a, b)
    for n in range(shape[0]):   # alone, and at another place of another batch
        assert torch.equal(HF.img_metrics_batch(fake[n:n + 1], real[n:n + 1])[0], a[n]), n
    rev = HF.img_metrics_batch(fake.flip(0), real.flip(0))
    assert torch.equal(rev.flip(0), a)


@pytest.mark.parametrize("shape", [(1, 3, 23, 40), (1, 3, 64, 64), (1, 1, 39, 70)])
def test_img_metrics_batch_vs_train_metrics(shape):
    """Both are fp64 sums rounded once to fp32: within 2 fp32 ulp of the value (ssim < 1: 1.2e-7;
    psnr < 128: 1.6e-5)."""
    from dsgan_hip import functional as HF
    from util.metrics import TrainMetrics
    fake, real = (t.to(DEV) for t in _pair(shape))
    m = TrainMetrics(torch.device(DEV))
    m.update(fake[0], real[0])
    s, p = m.averages()
    got = HF.img_metrics_batch(fake, real).cpu()[0].tolist()
    print("ssim %.9f vs %.9f, psnr %.7f vs %.7f" % (got[0], s, got[1], p))
    assert abs(got[0] - s) <= 1.2e-7 and abs(got[1] - p) <= 1.6e-5


def test_img_metrics_batch_refuses_small_planes():
    from dsgan_hip import functional as HF
    x = torch.zeros(1, 3, 6, 9, device=DEV)
    with pytest.raises(RuntimeError, match="bad args"):
        HF.img_metrics_batch(x, x)
    with pytest.raises(RuntimeError, match="bad args"):
        HF.img_metrics_batch(x.transpose(2, 3), x.transpose(2, 3))


# ---- uint8 panels ---------------------------------------------------------------------------

def _panel_input(shape, seed):
    """Every value the loader produces ((k/255 - 0.5)/0.5), +-1, +-1.2, then random values past the clip."""
    g = torch.Generator().manual_seed(seed)
    n = int(np.prod(shape))
    pool = torch.cat([(torch.arange(256, dtype=torch.float32) / 255 - 0.5) / 0.5,
                      torch.tensor([1.0, -1.0, 1.2, -1.2]), torch.rand(max(n - 260, 0), generator=g) * 2.6 - 1.3])
    if n < pool.numel():   # a small tensor: a different slice of the loader's values per seed
        pool = pool.roll(-61 * seed)
    return pool[:n][torch.randperm(n, generator=g)].reshape(shape)


def _panel_ref(imgs):
    out = []
    for n in range(imgs[0].shape[0]):
        u8 = [O.to_u8_hwc(t[n]) for t in imgs]
        out.append(np.hstack([np.repeat(a, 3, axis=2) if a.shape[2] == 1 else a for a in u8]))
    return np.stack(out)


# W = 7 and 130: one pixel per thread; W = 64: the four-pixel form
@pytest.mark.parametrize("nhw", [(2, 5, 7), (3, 33, 130), (2, 9, 64)])
@pytest.mark.parametrize("chans", [(1, 3, 3), (3, 3), (3,), (1,)])
def test_images_to_u8_bit_exact(nhw, chans):
    from dsgan_hip import functional as HF
    N, H, W = nhw
    imgs = [_panel_input((N, c, H, W), 7 * i + c) for i, c in enumerate(chans)]
    got = HF.images_to_u8(*[t.to(DEV) for t in imgs])
    assert got.dtype == torch.uint8 and got.shape == (N, H, len(chans) * W, 3)
    assert np.array_equal(got.cpu().numpy(), _panel_ref(imgs))


def test_images_to_u8_all_loader_values_and_nan():
    from dsgan_hip import functional as HF
    x = ((torch.arange(256, dtype=torch.float32) / 255 - 0.5) / 0.5).reshape(1, 1, 4, 64)
    got = HF.images_to_u8(x.to(DEV)).cpu()
    # (the reference's truncating conversion is not the loader's inverse: the oracle says what each value becomes)
    assert np.array_equal(got[0].numpy(), np.repeat(O.to_u8_hwc(x[0]), 3, axis=2))
    y = torch.tensor([float("nan"), 1.0, -1.0, 1.2, -1.2, 0.0, float("inf")]).reshape(1, 1, 1, 7)
    assert HF.images_to_u8(y.to(DEV)).cpu()[0, 0, :, 1].tolist() == [0, 255, 0, 255, 0, 127, 255]
    with pytest.raises(RuntimeError, match="channels"):
        HF.images_to_u8(torch.zeros(1, 2, 4, 4, device=DEV))


# ---- per-image gaussian SSIM ----------------------------------------------------------------

def _ssim_pair(shape):
    g = torch.Generator().manual_seed(shape[2] * shape[3] + shape[1])
    X = torch.rand(shape, generator=g)
    Y = (X + 0.15 * torch.randn(shape, generator=g)).clamp(0, 1)
    return X, Y


@pytest.mark.parametrize("shape", [(3, 3, 11, 11), (2, 1, 43, 75), (2, 3, 64, 64)])
def test_ssim_per_image_vs_oracle(shape):
    import MS_SSIM as M
    from dsgan_hip import functional as HF
    X, Y = _ssim_pair(shape)
    Xd, Yd = X.to(DEV), Y.to(DEV)
    got = M.ssim(Xd, Yd, data_range=1.0, size_average=False)
    assert got.shape == (shape[0],)
    for n in range(shape[0]):
        ref = float(O.ssim(X[n:n + 1], Y[n:n + 1]))
        print("image %d: %.7f vs %.7f" % (n, got[n].item(), ref))
        assert abs(got[n].item() - ref) < 2e-5, (n, got[n].item(), ref)
    mean = M.ssim(Xd, Yd, data_range=1.0).item()   # the existing no-grad batch mean
    assert abs(HF.ssim_eval_affine(Xd, Yd, 1.0, 0.0, 1.0).item() - mean) < 1e-6
    assert abs(got.mean().item() - mean) < 1e-6
    # an image's value does not depend on the batch around it
    assert torch.equal(M.ssim(Xd[-1:], Yd[-1:], data_range=1.0, size_average=False)[0], got[-1])


def test_ssim_nonnegative():
    import MS_SSIM as M
    X, Y = _ssim_pair((2, 3, 43, 75))
    Y[:, 0] = 1 - X[:, 0]   # an inverted plane: SSIM about -0.96
    per_ch = O.ssim_terms(X, Y)[0]
    assert (per_ch[:, 0] < -0.5).all() and (per_ch[:, 1:] > 0).all()
    Xd, Yd = X.to(DEV), Y.to(DEV)
    plain = M.ssim(Xd, Yd, data_range=1.0, size_average=False).cpu()
    nn_ = M.ssim(Xd, Yd, data_range=1.0, size_average=False, nonnegative_ssim=True).cpu()
    assert (plain - per_ch.mean(1)).abs().max() < 2e-5
    assert (nn_ - torch.relu(per_ch).mean(1)).abs().max() < 2e-5
    assert (nn_ - plain).min() > 0.2
    avg = M.ssim(Xd, Yd, data_range=1.0, nonnegative_ssim=True).item()
    assert abs(avg - float(torch.relu(per_ch).mean())) < 2e-5


def test_ssim_modules_return_the_functions_values():
    import MS_SSIM as M
    X, Y = (t.to(DEV) for t in _ssim_pair((2, 3, 43, 75)))
    assert torch.equal(M.SSIM(data_range=1.0, size_average=False, nonnegative_ssim=True)(X, Y),
                       M.ssim(X, Y, data_range=1.0, size_average=False, nonnegative_ssim=True))
    assert torch.equal(M.SSIM(data_range=1.0)(X, Y), M.ssim(X, Y, data_range=1.0))
    X2, Y2 = (t.to(DEV) for t in _ssim_pair((1, 3, 176, 176)))
    assert torch.equal(M.MS_SSIM(data_range=1.0, size_average=False)(X2, Y2),
                       M.ms_ssim(X2, Y2, data_range=1.0, size_average=False))
    Yg = Y.clone().requires_grad_(True)   # the gradient-carrying default path still works through the module
    M.SSIM(data_range=1.0)(X, Yg).backward()
    assert Yg.grad is not None and torch.isfinite(Yg.grad).all()
    with pytest.raises(NotImplementedError):
        M.SSIM(data_range=1.0, size_average=False)(X, Yg)


def test_ms_ssim_still_refuses_two_gradients():
    import MS_SSIM as M
    X, Y = (t.to(DEV).requires_grad_(True) for t in _ssim_pair((1, 3, 176, 176)))
    with pytest.raises(NotImplementedError):
        M.ms_ssim(X, Y, data_range=1.0)


# ---- EvalMetrics ------------------------------------------------------------------------------

def test_eval_metrics_rows():
    from dsgan_hip import functional as HF
    from util.metrics import EvalMetrics
    fake, real = _pair((3, 3, 64, 64))
    fd, rd = fake.clamp(-1, 1).to(DEV), real.clamp(-1, 1).to(DEV)
    m = EvalMetrics(torch.device(DEV), 5)
    m.update(fd[:2], rd[:2])
    m.update(fd[2:], rd[2:])
    rows = torch.tensor(m.rows())
    assert rows.shape == (3, 4) and torch.isnan(rows[:, 3]).all()
    assert torch.equal(rows[:, :2], HF.img_metrics_batch(fd, rd).cpu())
    for n in range(3):
        ref = float(O.ssim((rd[n:n + 1].cpu() + 1) / 2, (fd[n:n + 1].cpu() + 1) / 2))
        assert abs(rows[n, 2].item() - ref) < 2e-5
    means = m.means()
    assert abs(means[0] - rows[:, 0].double().mean().item()) < 1e-9 and np.isnan(means[3])
    with pytest.raises(ValueError, match="capacity"):
        m.update(fd, rd)
    m.reset()
    assert m.rows() == []


def test_eval_metrics_ms_ssim_and_graph_capture():
    """Above 160 px the fourth column is MS-SSIM; and ``update`` only enqueues work: it can be captured
    in a graph, whose replay on new data gives the eager rows."""
    from util.metrics import EvalMetrics
    dev = torch.device(DEV)
    g = torch.Generator().manual_seed(5)
    real = [torch.rand((1, 3, 176, 176), generator=g) * 2 - 1 for _ in range(2)]
    fake = [(r + 0.2 * torch.randn(r.shape, generator=g)).clamp(-1, 1) for r in real]
    m = EvalMetrics(dev, 1)
    eager = []
    for f, r in zip(fake, real):
        m.reset()
        m.update(f.to(dev), r.to(dev))
        eager.append(torch.tensor(m.rows()))
    ref = float(O.ms_ssim((real[0] + 1) / 2, (fake[0] + 1) / 2))
    assert abs(eager[0][0, 3].item() - ref) < 2e-5, (eager[0], ref)
    sf, sr = fake[0].to(dev), real[0].to(dev)
    m.reset()
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        m.update(sf, sr)
    for i in (1, 0):
        sf.copy_(fake[i])
        sr.copy_(real[i])
        m.buf.fill_(float("nan"))
        graph.replay()
        assert torch.equal(torch.tensor(m.rows()), eager[i]), i
