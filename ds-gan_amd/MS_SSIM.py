"""SSIM / MS-SSIM on the HIP path (DSGAN/MS_SSIM.py:95-225 interface).

``ssim(X, Y, data_range, size_average=True)`` with the default 11-tap sigma-1.5 gaussian runs
the fused SSIM kernel (forward + analytic backward).  ``ms_ssim`` (DSGAN/MS_SSIM.py:153-225)
runs the MS-SSIM kernels: five scales of the SSIM / contrast-structure plane means with the
padded 2x2 average pool between them, combined on the device.  Both are differentiable like the
reference's autograd versions: when one operand requires grad the training kernels run
(``HF.SSIMFn`` / ``HF.MSSSIMFn``, analytic backward through the gaussian filters and the
pyramid) and the gradient flows to that operand.  SSIM is symmetric in (X, Y), so the operand
that requires grad is passed as the kernels' differentiated argument.  A gradient w.r.t. both
operands at once is not implemented and raises (never a silent zero gradient); without any
operand requiring grad, ``ms_ssim`` uses the evaluation kernel (per-image values for
``size_average=False``).  ``ssim(size_average=False)`` and ``nonnegative_ssim=True`` are evaluation
only (``HF.ssim_eval_affine``): with an operand that requires grad they raise.  ``SSIM`` / ``MS_SSIM``
are the reference's ``nn.Module`` wrappers of the two functions.
"""
import torch

from dsgan_hip import functional as HF


def _grad_order(X, Y, name):
    """(const, differentiated) operands, or None when no grad is needed."""
    need = torch.is_grad_enabled()
    gx, gy = need and X.requires_grad, need and Y.requires_grad
    if gx and gy:
        raise NotImplementedError("HIP %s differentiates w.r.t. one operand; both X and Y require grad" % name)
    if gy:
        return X, Y
    if gx:
        return Y, X     # SSIM(X, Y) == SSIM(Y, X): differentiate the X side
    return None


def ssim(X, Y, data_range=255, size_average=True, win_size=11, win_sigma=1.5, win=None,
         K=(0.01, 0.03), nonnegative_ssim=False):
    if X.shape != Y.shape:
        raise ValueError(f"Input images should have the same dimensions, but got {X.shape} and {Y.shape}.")
    if X.dim() != 4:
        raise ValueError("HIP ssim supports 4-d (N,C,H,W) tensors")
    if win is not None or win_size != 11 or win_sigma != 1.5 or tuple(K) != (0.01, 0.03):
        raise NotImplementedError("HIP ssim implements the default window (11, 1.5) and K=(0.01, 0.03)")
    if not size_average or nonnegative_ssim:
        # per-image values / the relu'd per-channel form: evaluation only (HF.ssim_eval_affine)
        if torch.is_grad_enabled() and (X.requires_grad or Y.requires_grad):
            raise NotImplementedError("HIP ssim with a gradient implements size_average=True without relu")
        return HF.ssim_eval_affine(X, Y, 1.0, 0.0, float(data_range), size_average, nonnegative_ssim)
    order = _grad_order(X, Y, "ssim")
    real, fake = order if order is not None else (X, Y)
    return HF.ssim_affine(real, fake, 1.0, 0.0, float(data_range))


def ms_ssim(X, Y, data_range=255, size_average=True, win_size=11, win_sigma=1.5, win=None, weights=None,
            K=(0.01, 0.03)):
    if X.shape != Y.shape:
        raise ValueError(f"Input images should have the same dimensions, but got {X.shape} and {Y.shape}.")
    if X.dim() != 4:
        raise ValueError("HIP ms_ssim supports 4-d (N,C,H,W) tensors")
    if win is not None or win_size != 11 or win_sigma != 1.5 or tuple(K) != (0.01, 0.03):
        raise NotImplementedError("HIP ms_ssim implements the default window (11, 1.5) and K=(0.01, 0.03)")
    w = HF.MS_SSIM_WEIGHTS if weights is None else tuple(float(v) for v in weights)
    smaller_side = min(X.shape[-2:])
    assert smaller_side > (win_size - 1) * (2 ** (len(w) - 1)), \
        "Image size should be larger than %d due to the 4 downsamplings in ms-ssim" % ((win_size - 1) * (2 ** 4))
    order = _grad_order(X, Y, "ms_ssim")
    if order is None:
        return HF.ms_ssim_affine(X, Y, 1.0, 0.0, float(data_range), w, size_average)
    if not size_average:
        raise NotImplementedError("HIP ms_ssim gradient implements size_average=True (the batch mean)")
    real, fake = order
    return HF.ms_ssim_loss_affine(real, fake, 1.0, 0.0, float(data_range), w)


class SSIM(torch.nn.Module):
    """``ssim`` as a module with the reference's constructor arguments (DSGAN/MS_SSIM.py:228-268).
    ``channel`` and ``spatial_dims`` only sized the reference's window tensor: the kernels build the
    one 11-tap window themselves, so the module keeps (win_size, win_sigma) and the function refuses
    anything but the default."""

    def __init__(self, data_range=255, size_average=True, win_size=11, win_sigma=1.5, channel=3, spatial_dims=2,
                 K=(0.01, 0.03), nonnegative_ssim=False):
        super().__init__()
        if spatial_dims != 2:
            raise NotImplementedError("HIP SSIM supports 2 spatial dimensions")
        self.data_range, self.size_average = data_range, size_average
        self.win_size, self.win_sigma, self.channel = win_size, win_sigma, channel
        self.K, self.nonnegative_ssim = K, nonnegative_ssim

    def forward(self, X, Y):
        return ssim(X, Y, data_range=self.data_range, size_average=self.size_average, win_size=self.win_size,
                    win_sigma=self.win_sigma, K=self.K, nonnegative_ssim=self.nonnegative_ssim)


class MS_SSIM(torch.nn.Module):
    """``ms_ssim`` as a module with the reference's constructor arguments (DSGAN/MS_SSIM.py:271-311)."""

    def __init__(self, data_range=255, size_average=True, win_size=11, win_sigma=1.5, channel=3, spatial_dims=2,
                 weights=None, K=(0.01, 0.03)):
        super().__init__()
        if spatial_dims != 2:
            raise NotImplementedError("HIP MS_SSIM supports 2 spatial dimensions")
        self.data_range, self.size_average = data_range, size_average
        self.win_size, self.win_sigma, self.channel = win_size, win_sigma, channel
        self.weights, self.K = weights, K

    def forward(self, X, Y):
        return ms_ssim(X, Y, data_range=self.data_range, size_average=self.size_average, win_size=self.win_size,
                       win_sigma=self.win_sigma, weights=self.weights, K=self.K)
