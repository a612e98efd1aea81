"""train.py's per-iteration image metrics on the device (DSGAN/train.py:27-44, 110-124).

The reference moves image 0 of real_A / fake_B / real_B to the host every iteration, converts
them to uint8 and runs skimage SSIM / PSNR on the CPU.  ``TrainMetrics.update`` runs the same
arithmetic on the GPU (``dsgan_img_metrics``) and accumulates the sums in device memory; the
host reads them only when it prints (``averages``), so the loop has no per-iteration sync."""
import torch

from dsgan_hip._lib import call, ptr, stream


class TrainMetrics:
    def __init__(self, device):
        self.acc = torch.zeros(3, device=device, dtype=torch.float32)
        self.part = torch.empty(128, device=device, dtype=torch.float64)

    def reset(self):
        self.acc.zero_()

    def update(self, fake, real):
        """fake, real: one [C,H,W] image each in [-1, 1] (fake_B[0], real_B[0])."""
        fake, real = fake.detach().contiguous(), real.detach().contiguous()
        C, H, W = fake.shape
        call("dsgan_img_metrics", ptr(fake), ptr(real), C, H, W, ptr(self.part), ptr(self.acc), stream())

    def averages(self):
        s, p, n = self.acc.tolist()
        n = max(n, 1.0)
        return s / n, p / n


class EvalMetrics:
    """Per-image test-set metrics in a preallocated device buffer of ``capacity`` rows (evaluate.py,
    train.py --eval_freq).  A row is COLUMNS:

      ssim        the skimage-style SSIM train.py logs (uint8 images, uniform 7x7 window)
      psnr        of the same uint8 images
      ssim_gauss  MS_SSIM.ssim of (t+1)/2 with data_range 1 (11-tap gaussian window)
      ms_ssim     MS_SSIM.ms_ssim of the same; NaN when the smaller side is <= 160

    ``update`` only enqueues kernels (no .item(), .cpu() or synchronize; it can be captured in a HIP
    graph); ``rows`` and ``means`` read the buffer back once."""

    COLUMNS = ("ssim", "psnr", "ssim_gauss", "ms_ssim")
    MS_MIN_SIDE = 160   # (win_size - 1) * 2^4, DSGAN/MS_SSIM.py:194-197

    def __init__(self, device, capacity):
        self.buf = torch.full((int(capacity), len(self.COLUMNS)), float("nan"), device=device, dtype=torch.float32)
        self.n = 0

    def reset(self):
        self.n = 0

    def update(self, fake, real):
        """fake, real: [N,C,H,W] batches in [-1, 1]; appends one row per image."""
        from dsgan_hip import functional as HF
        N, _, H, W = fake.shape
        if self.n + N > self.buf.shape[0]:
            raise ValueError("EvalMetrics: %d rows of capacity, %d images" % (self.buf.shape[0], self.n + N))
        rows = self.buf[self.n:self.n + N]
        both = HF.img_metrics_batch(fake, real)
        rows[:, 0:2].copy_(both)
        if min(H, W) > 10:
            rows[:, 2].copy_(HF.ssim_eval_affine(real, fake, 0.5, 0.5, 1.0, size_average=False))
        else:   # smaller than the 11-tap window
            rows[:, 2].fill_(float("nan"))
        if min(H, W) > self.MS_MIN_SIDE:
            rows[:, 3].copy_(HF.ms_ssim_affine(real, fake, 0.5, 0.5, 1.0, size_average=False))
        else:
            rows[:, 3].fill_(float("nan"))
        self.n += N

    def rows(self):
        """The rows so far as a list of [ssim, psnr, ssim_gauss, ms_ssim] lists (one read-back)."""
        return self.buf[:self.n].cpu().tolist()

    def means(self):
        """Column means over the rows so far (NaN for a column that holds NaN, or without rows)."""
        if self.n == 0:
            return [float("nan")] * len(self.COLUMNS)
        return self.buf[:self.n].double().mean(0).cpu().tolist()
