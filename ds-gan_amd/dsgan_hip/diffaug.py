"""Differentiable augmentation of the discriminator's input (--diffaug), restated without a GPU.

The device kernels (csrc/diffaug.hip) and this module compute the same function; this one is the
reference the tests hold the kernels to, as resample.py is for the resize.  Pure Python / numpy / torch
on the CPU: no import of the HIP library.

Sample ``i`` of call ``k`` of the stream ``(seed, stream)`` draws eight words,

    w = Philox4x32-10(key = seed, counter = (i, 0, k mod 2^32, stream))
    v = Philox4x32-10(key = seed, counter = (i, 1, k mod 2^32, stream))

and with ``u24(x) = (x >> 8) * 2^-24`` and ``mulhi(x, m) = (x * m) >> 32``:

  color        b = u24(w0) - 1/2, s = 2 u24(w1), c = u24(w2) + 1/2, on the image channels only:
               u = x + b;  u' = (u - mean_c u) s + mean_c u;  u'' = (u' - M) c + M, M = the sample's mean of u'
  translation  tx = mulhi(w3, 2 Sx + 1) - Sx, ty = mulhi(v0, 2 Sy + 1) - Sy, Sx = floor(W/8 + 1/2), Sy alike:
               y[r, q] = x[r - ty, q - tx] inside the image, 0 outside (condition and image together)
  cutout       ch = floor(H/2 + 1/2), oy = mulhi(v1, H + 1 - ch % 2) (cw, ox from v2 alike):
               rows [oy - ch//2, oy - ch//2 + ch) x the like columns, clipped to the image, are 0

``v3`` is unused.  Every word is drawn whatever the policy is; an op outside the policy is the identity.
"""
import numpy as np

OPS = ("color", "translation", "cutout")   # the order of application
BITS = {"color": 1, "translation": 2, "cutout": 4}


def parse_policy(policy):
    """'color,translation,cutout' (any subset, any order) -> the tuple of its ops in the order they are
    applied; '' / None -> ().  An unknown or repeated name raises ValueError naming it."""
    if policy is None:
        return ()
    names = [p.strip() for p in policy.split(",")] if isinstance(policy, str) else [str(p) for p in policy]
    names = [p for p in names if p]
    for p in names:
        if p not in OPS:
            raise ValueError("--diffaug: unknown augmentation %r (choose from %s)" % (p, ", ".join(OPS)))
        if names.count(p) > 1:
            raise ValueError("--diffaug: augmentation %r given more than once" % p)
    return tuple(p for p in OPS if p in names)


def policy_string(policy):
    """The canonical spelling of a policy (what a state file records)."""
    return ",".join(parse_policy(policy))


def policy_bits(policy):
    """The kernels' policy word: bit 0 color, bit 1 translation, bit 2 cutout."""
    return sum(BITS[p] for p in parse_policy(policy))


_M0, _M1 = np.uint64(0xD2511F53), np.uint64(0xCD9E8D57)
_W0, _W1 = 0x9E3779B9, 0xBB67AE85
_LO = np.uint64(0xFFFFFFFF)
_S32 = np.uint64(32)


def philox4x32_10(counter, key):
    """Philox-4x32-10 (Salmon et al., SC'11).  counter: four words (ints or equal-length arrays),
    key: two words.  Returns a uint32 array [..., 4]."""
    c = [np.asarray(x, dtype=np.uint64) & _LO for x in np.broadcast_arrays(*[np.asarray(x, dtype=np.uint64) for x in counter])]
    k0, k1 = int(key[0]) & 0xFFFFFFFF, int(key[1]) & 0xFFFFFFFF
    c0, c1, c2, c3 = c
    for _ in range(10):
        p0, p1 = _M0 * c0, _M1 * c2
        n0 = (p1 >> _S32) ^ c1 ^ np.uint64(k0)
        n2 = (p0 >> _S32) ^ c3 ^ np.uint64(k1)
        c0, c1, c2, c3 = n0, p1 & _LO, n2, p0 & _LO
        k0, k1 = (k0 + _W0) & 0xFFFFFFFF, (k1 + _W1) & 0xFFFFFFFF
    return np.stack([c0, c1, c2, c3], axis=-1).astype(np.uint32)


def _u24(x):
    return (x >> np.uint32(8)).astype(np.float32) * np.float32(2.0 ** -24)


def _mulhi(x, m):
    return ((x.astype(np.uint64) * np.uint64(m)) >> _S32).astype(np.int32)


def geometry(H, W):
    """(Sx, Sy, ch, cw): the largest shifts and the cutout's size for an H x W image."""
    return (W + 4) // 8, (H + 4) // 8, (H + 1) // 2, (W + 1) // 2


def draw_params(seed, stream, call, n, H, W):
    """The draws of samples 0..n-1 of call ``call``: a dict of float32 arrays ``b, s, c`` and int32 arrays
    ``tx, ty, oy, ox``, each of n elements.  The key is the 64-bit seed split low word first, as the
    dropout's; the call enters with its low 32 bits."""
    seed = int(seed) & (2 ** 64 - 1)
    key = (seed & 0xFFFFFFFF, seed >> 32)
    i = np.arange(int(n), dtype=np.uint64)
    k = int(call) & 0xFFFFFFFF
    w = philox4x32_10((i, 0, k, int(stream)), key)
    v = philox4x32_10((i, 1, k, int(stream)), key)
    Sx, Sy, ch, cw = geometry(H, W)
    return {"b": _u24(w[:, 0]) - np.float32(0.5),
            "s": np.float32(2.0) * _u24(w[:, 1]),
            "c": _u24(w[:, 2]) + np.float32(0.5),
            "tx": _mulhi(w[:, 3], 2 * Sx + 1) - np.int32(Sx),
            "ty": _mulhi(v[:, 0], 2 * Sy + 1) - np.int32(Sy),
            "oy": _mulhi(v[:, 1], H + 1 - ch % 2),
            "ox": _mulhi(v[:, 2], W + 1 - cw % 2)}


PARAM_FIELDS = ("b", "s", "c", "tx", "ty", "oy", "ox")


def pack_params(p):
    """The [n, 8] float32 table dsgan_diffaug_params writes: floats as they are, integers as int32 bit
    patterns, the last column 0."""
    n = len(p["b"])
    out = np.zeros((n, 8), dtype=np.float32)
    for j, f in enumerate(PARAM_FIELDS):
        a = np.asarray(p[f])
        out[:, j] = a.astype(np.float32) if j < 3 else a.astype(np.int32).view(np.float32)
    return out


def unpack_params(table):
    """The inverse of pack_params."""
    t = np.ascontiguousarray(np.asarray(table, dtype=np.float32))
    return {f: (t[:, j].copy() if j < 3 else t[:, j].copy().view(np.int32)) for j, f in enumerate(PARAM_FIELDS)}


def concat_params(*ps):
    """The draws of several calls, one after the other (a stacked launch's samples)."""
    return {f: np.concatenate([np.asarray(p[f]) for p in ps]) for f in PARAM_FIELDS}


def cutout_box(oy, ox, H, W):
    """(y0, y1, x0, x1): the zeroed rows and columns, clipped to the image."""
    _, _, ch, cw = geometry(H, W)
    y0, x0 = int(oy) - ch // 2, int(ox) - cw // 2
    return max(y0, 0), min(y0 + ch, H), max(x0, 0), min(x0 + cw, W)


def augment_reference(x, Ca, policy, params):
    """The transform of ``x`` [n, Ca+Cb, H, W] (a torch tensor) with the draws ``params`` (draw_params'
    dict, sample j of x taking entry j), in torch ops on x's dtype: autograd through it on float64 is the
    reference backward."""
    import torch
    import torch.nn.functional as F

    ops = parse_policy(policy)
    n, C, H, W = x.shape
    if C <= Ca:
        raise ValueError("augment_reference: no image channels behind the %d condition channels" % Ca)
    Sx, Sy, _, _ = geometry(H, W)
    out = []
    for j in range(n):
        a, u = x[j, :Ca], x[j, Ca:]
        if "color" in ops:
            b, s, c = (float(params[f][j]) for f in ("b", "s", "c"))
            u = u + b
            m = u.mean(dim=0, keepdim=True)
            u = (u - m) * s + m
            M = u.mean()
            u = (u - M) * c + M
        y = torch.cat([a, u], dim=0)
        if "translation" in ops:
            tx, ty = int(params["tx"][j]), int(params["ty"][j])
            y = F.pad(y, (Sx, Sx, Sy, Sy))[:, Sy - ty:Sy - ty + H, Sx - tx:Sx - tx + W]
        if "cutout" in ops:
            y0, y1, x0, x1 = cutout_box(params["oy"][j], params["ox"][j], H, W)
            keep = torch.ones((H, W), dtype=torch.bool, device=x.device)
            keep[y0:y1, x0:x1] = False
            y = torch.where(keep, y, torch.zeros((), dtype=y.dtype, device=y.device))
        out.append(y)
    return torch.stack(out, dim=0)


def backward_closed_form(dy, Ca, policy, params):
    """The transpose of augment_reference applied to ``dy`` [n, Ca+Cb, H, W], for the image channels:
    g = dy shifted back where the forward wrote an uncut pixel, else 0;  g1 = c g + (1 - c) mean_chw g;
    dx = s g1 + (1 - s) mean_c g1  (brightness is the identity).  Returns [n, Cb, H, W] in dy's dtype."""
    import torch

    ops = parse_policy(policy)
    n, C, H, W = dy.shape
    out = []
    for j in range(n):
        g = dy[j, Ca:]
        if "cutout" in ops:
            y0, y1, x0, x1 = cutout_box(params["oy"][j], params["ox"][j], H, W)
            g = g.clone()
            g[:, y0:y1, x0:x1] = 0
        if "translation" in ops:
            tx, ty = int(params["tx"][j]), int(params["ty"][j])
            sh = torch.zeros_like(g)
            r0, r1 = max(0, -ty), min(H, H - ty)     # rows r with 0 <= r + ty < H
            q0, q1 = max(0, -tx), min(W, W - tx)
            sh[:, r0:r1, q0:q1] = g[:, r0 + ty:r1 + ty, q0 + tx:q1 + tx]
            g = sh
        if "color" in ops:
            s, c = float(params["s"][j]), float(params["c"][j])
            g = c * g + (1.0 - c) * g.mean()
            g = s * g + (1.0 - s) * g.mean(dim=0, keepdim=True)
        out.append(g)
    return torch.stack(out, dim=0)
