"""Load-time resize (--load_resize): Pillow's 8-bit resampler restated, and its device call.

``PIL.Image.resize`` on 8-bit images is integer arithmetic (Pillow, src/libImaging/Resample.c).  Per axis
``precompute_coeffs`` builds, in double, a window ``(xmin, n)`` and ``n`` normalised weights for every
output index; ``normalize_coeffs_8bpc`` rounds them to 22-bit fixed point; a pass is
``clip8((2^21 + sum p * k) >> 22)`` in ``int``.  The horizontal pass runs first into a uint8 intermediate,
then the vertical one; a pass whose axis keeps its size is skipped.

  pil_coeffs            the tables of one axis, operation for operation in Python floats (IEEE doubles)
  resize_u8_reference   the numpy integer model of the two passes: the written definition of what
                        csrc/resample.hip computes, and the tests' second oracle beside Pillow itself
  device_tables         the tables on the device, cached per (in, out, filter, device)
  resize_crop_to_image  dsgan_u8_resize_crop_to_image: resize, crop at per-sample offsets, flip, normalise,
                        optional gray -- fp32 NCHW, bit-exact with PIL resize -> host crop -> dsgan_u8_to_image
"""
import math

import numpy as np

PRECISION_BITS = 32 - 8 - 2     # Pillow's: 22-bit coefficients, int accumulation of 8-bit samples
MAX_SCALE = 16                  # source axis / load axis: bounds the window at MAX_TAPS coefficients
MAX_TAPS = 65                   # ceil(2 * 16) * 2 + 1, the bicubic window at 16x down-scaling
FILTERS = ("bicubic", "bilinear")


def _bilinear(x):
    if x < 0.0:
        x = -x
    if x < 1.0:
        return 1.0 - x
    return 0.0


def _bicubic(x):
    a = -0.5   # Pillow's; the polynomials as Resample.c writes them
    if x < 0.0:
        x = -x
    if x < 1.0:
        return ((a + 2.0) * x - (a + 3.0)) * x * x + 1
    if x < 2.0:
        return (((x - 5) * x + 8) * x - 4) * a
    return 0.0


_FILTER = {"bicubic": (_bicubic, 2.0), "bilinear": (_bilinear, 1.0)}


def check_scale(in_size, out_size, what="axis"):
    if in_size < 1 or out_size < 1:
        raise ValueError("load resize: %s of %d -> %d pixels" % (what, in_size, out_size))
    if in_size > MAX_SCALE * out_size:
        raise ValueError("load resize: source %s of %d pixels is more than %dx the load size %d (the filter window "
                         "is capped at %d taps)" % (what, in_size, MAX_SCALE, out_size, MAX_TAPS))


def pil_coeffs(in_size, out_size, filter="bicubic"):
    """(bounds int32 [out][2] = (xmin, n), coef int32 [out][ksize]) of one axis: Pillow's precompute_coeffs
    followed by normalize_coeffs_8bpc."""
    if filter not in _FILTER:
        raise ValueError("load resize: filter %r, expected one of %s" % (filter, ", ".join(FILTERS)))
    in_size, out_size = int(in_size), int(out_size)
    check_scale(in_size, out_size)
    f, fsupport = _FILTER[filter]
    scale = filterscale = float(in_size) / out_size
    if filterscale < 1.0:
        filterscale = 1.0
    support = fsupport * filterscale
    ksize = int(math.ceil(support)) * 2 + 1
    ss = 1.0 / filterscale
    bounds = np.zeros((out_size, 2), dtype=np.int32)
    coef = np.zeros((out_size, ksize), dtype=np.int32)
    one = float(1 << PRECISION_BITS)
    for xx in range(out_size):
        center = (xx + 0.5) * scale
        xmin = int(center - support + 0.5)
        if xmin < 0:
            xmin = 0
        xmax = int(center + support + 0.5)
        if xmax > in_size:
            xmax = in_size
        xmax -= xmin
        w = [f((x + xmin - center + 0.5) * ss) for x in range(xmax)]
        ww = 0.0
        for v in w:
            ww += v
        if ww != 0.0:
            w = [v / ww for v in w]
        for x, v in enumerate(w):
            coef[xx, x] = int(-0.5 + v * one) if v < 0 else int(0.5 + v * one)
        bounds[xx] = (xmin, xmax)
    return bounds, coef


def _pass_rows(img, bounds, coef):
    """One pass along axis 0 of uint8 [in][...] -> uint8 [out][...]: int accumulation, +2^21, >> 22, clip."""
    out = np.empty((bounds.shape[0],) + img.shape[1:], dtype=np.uint8)
    src = img.astype(np.int64)
    for i, (lo, n) in enumerate(bounds):
        k = coef[i, :n].astype(np.int64).reshape((n,) + (1,) * (img.ndim - 1))
        acc = (src[lo:lo + n] * k).sum(axis=0) + (1 << (PRECISION_BITS - 1))
        out[i] = np.clip(acc >> PRECISION_BITS, 0, 255)
    return out


def resize_u8_reference(img, out_h, out_w, filter="bicubic"):
    """uint8 [H][W] or [H][W][C] -> uint8 [out_h][out_w]...: PIL.Image.resize((out_w, out_h), filter) in
    numpy integers.  Horizontal pass first, uint8 between the passes, an unchanged axis skipped."""
    img = np.ascontiguousarray(img, dtype=np.uint8)
    H, W = img.shape[:2]
    if W != out_w:
        b, c = pil_coeffs(W, out_w, filter)
        img = np.swapaxes(_pass_rows(np.swapaxes(img, 0, 1), b, c), 0, 1)
    if H != out_h:
        b, c = pil_coeffs(H, out_h, filter)
        img = _pass_rows(img, b, c)
    return np.ascontiguousarray(img)


def tmp_bytes(N, Hs, fw, kx):
    """Bytes of the horizontal pass's uint8 intermediate [N][Hs][fw][3] (none when that axis is unchanged)."""
    return int(N) * int(Hs) * int(fw) * 3 if kx else 0


_TABLES = {}


def device_tables(in_size, out_size, filter, device):
    """(bounds, coef, ksize) as device int32 tensors; (None, None, 0) when the axis keeps its size."""
    if in_size == out_size:
        return None, None, 0
    import torch
    key = (int(in_size), int(out_size), filter, str(device))
    if key not in _TABLES:
        b, c = pil_coeffs(in_size, out_size, filter)
        _TABLES[key] = (torch.from_numpy(b).to(device), torch.from_numpy(c).to(device), int(c.shape[1]))
    return _TABLES[key]


def check_geometry(load_h, load_w, fh, fw):
    if load_h < fh or load_w < fw:
        raise ValueError("--load_resize: loadSize %dx%d (h x w) is smaller than fineSize %dx%d: the crop is taken "
                         "from the resized image" % (load_h, load_w, fh, fw))


def check_offsets(offsets, load_h, load_w, fh, fw):
    """offsets: N pairs (h_off, w_off) of the crop window inside the load_h x load_w image."""
    for n, (ho, wo) in enumerate(offsets):
        if not (0 <= int(ho) <= load_h - fh and 0 <= int(wo) <= load_w - fw):
            raise ValueError("load resize: sample %d crop offset (h %d, w %d) outside [0, %d] x [0, %d] "
                             "(load %dx%d, fine %dx%d)" % (n, ho, wo, load_h - fh, load_w - fw, load_h, load_w, fh, fw))


def resize_crop_to_image(u8, load_h, load_w, offsets, flip, fh, fw, gray=False, filter="bicubic"):
    """uint8 [N][Hs][Ws][3] frames (host or device) -> fp32 [N][1|3][fh][fw] on the GPU: each frame resized
    to load_h x load_w as PIL does it, cropped at offsets[n] = (h_off, w_off), flipped where flip[n],
    normalised to [-1, 1], gray when asked.  Everything is validated on the host before the upload."""
    import torch
    from ._lib import call, ptr, stream
    if u8.dim() != 4 or u8.shape[3] != 3 or u8.dtype != torch.uint8:
        raise ValueError("load resize: expected uint8 [N][H][W][3] frames, got %s %s" % (u8.dtype, tuple(u8.shape)))
    N, Hs, Ws, _ = u8.shape
    load_h, load_w, fh, fw = int(load_h), int(load_w), int(fh), int(fw)
    check_geometry(load_h, load_w, fh, fw)
    check_scale(Hs, load_h, "height")
    check_scale(Ws, load_w, "width")
    offsets = [(int(a), int(b)) for a, b in offsets]
    flip = [int(v) for v in flip]
    if len(offsets) != N or len(flip) != N:
        raise ValueError("load resize: %d frames, %d offsets, %d flip flags" % (N, len(offsets), len(flip)))
    check_offsets(offsets, load_h, load_w, fh, fw)
    dev = torch.device("cuda", torch.cuda.current_device())
    yb, yc, ky = device_tables(Hs, load_h, filter, dev)
    xb, xc, kx = device_tables(Ws, load_w, filter, dev)
    u8 = u8.to(dev, non_blocking=True).contiguous()
    off = torch.tensor(offsets, dtype=torch.int32).reshape(N, 2).to(dev, non_blocking=True)
    fl = torch.tensor(flip, dtype=torch.int32).to(dev, non_blocking=True)
    need = tmp_bytes(N, Hs, fw, kx)
    tmp = torch.empty(need, device=dev, dtype=torch.uint8) if need else None
    out = torch.empty((N, 1 if gray else 3, fh, fw), device=dev, dtype=torch.float32)
    call("dsgan_u8_resize_crop_to_image", ptr(u8), N, Hs, Ws, ptr(yb), ptr(yc), ky, ptr(xb), ptr(xc), kx,
         load_h, load_w, ptr(off), ptr(fl), fh, fw, int(gray), ptr(tmp), need, ptr(out), stream())
    return out
