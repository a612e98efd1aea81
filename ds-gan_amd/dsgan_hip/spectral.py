"""Spectral normalisation of the discriminator's conv weights (--spectral_norm), restated without a GPU.

The device kernels (csrc/spectral.hip) and this module compute the same function; this one is the
reference the tests hold the kernels to, as diffaug.py is for the augmentation.  Pure Python / numpy /
torch on the CPU: no import of the HIP library.

A conv weight ``W [Cout, Cin, kh, kw]`` is viewed as the matrix ``[R, C] = [Cout, Cin kh kw]``; with unit
vectors ``u [R]``, ``v [C]`` and ``eps = 1e-12``:

  refresh(W, u, v, iterate=True)     v <- W^T u / max(|W^T u|, eps);  a = W v;  u <- a / max(|a|, eps);
                                     sigma = u . a;  W_sn = W / sigma
  refresh(W, u, v, iterate=False)    u and v are kept;  a = W v;  sigma = u . a;  W_sn = W / sigma
  backward(G, W_sn, u, v, sigma)     dL/dW = (G - <G, W_sn> u v^T) / sigma     (u, v constants)

The iterating form is one power iteration with the arithmetic of ``torch.nn.utils.spectral_norm`` in
training mode (Miyato et al., ICLR 2018), and ``backward`` is what autograd gives through it.  Unlike
torch's wrapper, which iterates at every forward, the model refreshes once per discriminator weight
version (the SN-GAN paper's rule): at construction and right after every ``optimizer_D.step()``.
"""
import numpy as np

EPS = 1e-12
U_SEED = 0x534E   # the private generator of layer i is seeded with U_SEED + i


def as_matrix(W):
    """The [Cout, Cin kh kw] view of a conv weight (numpy or torch)."""
    return W.reshape(W.shape[0], -1)


def refresh(W, u, v=None, iterate=True, eps=EPS):
    """numpy, in W's dtype (float64 for the reference, float32 to measure what the format costs).
    Returns (W_sn, u, v, sigma); W_sn has W's shape.  ``v`` may be None only when iterating."""
    W = np.asarray(W)
    dt = W.dtype
    M = as_matrix(W)
    u = np.asarray(u, dtype=dt)
    if iterate:
        t = M.T @ u
        v = t / max(np.sqrt((t * t).sum(dtype=dt)), dt.type(eps))
        a = M @ v
        u = a / max(np.sqrt((a * a).sum(dtype=dt)), dt.type(eps))
    else:
        if v is None:
            raise ValueError("refresh(iterate=False) needs v")
        v = np.asarray(v, dtype=dt)
        a = M @ v
    sigma = (u * a).sum(dtype=dt)
    return (W / sigma).astype(dt), u.astype(dt), v.astype(dt), dt.type(sigma)


def backward(G, W_sn, u, v, sigma):
    """numpy: the gradient w.r.t. W of a loss whose gradient w.r.t. W_sn is ``G`` (W's shape)."""
    G = np.asarray(G)
    dt = G.dtype
    g, ws = as_matrix(G), as_matrix(np.asarray(W_sn, dtype=dt))
    s = (g * ws).sum(dtype=dt)
    out = (g - s * np.outer(np.asarray(u, dtype=dt), np.asarray(v, dtype=dt))) / dt.type(sigma)
    return out.reshape(G.shape).astype(dt)


def refresh_torch(W, u, v=None, iterate=True, eps=EPS):
    """The same function on torch tensors, in W's dtype.  ``u`` and ``v`` are treated as constants and the
    result stays attached to ``W``: autograd through it gives ``backward``.  Returns (W_sn, u, v, sigma)."""
    import torch
    M = as_matrix(W)
    with torch.no_grad():
        if iterate:
            t = M.detach().t().mv(u)
            v = t / t.norm().clamp_min(eps)
            a = M.detach().mv(v)
            u = a / a.norm().clamp_min(eps)
        elif v is None:
            raise ValueError("refresh_torch(iterate=False) needs v")
    sigma = torch.dot(u, M.mv(v))
    return W / sigma, u, v, sigma


def initial_u(index, rows):
    """Layer ``index``'s starting u [rows], fp32: N(0, 1) from a private torch.Generator seeded with
    U_SEED + index, normalised.  The global RNG is not touched and every rank draws the same vector."""
    import torch
    g = torch.Generator(device="cpu")
    g.manual_seed(U_SEED + int(index))
    u = torch.randn(int(rows), generator=g, dtype=torch.float32)
    return u / u.norm().clamp_min(EPS)


# ---- checkpoint keys (torch.nn.utils.spectral_norm's: weight_orig, weight_u, weight_v beside bias) ----
SN_SUFFIXES = ("weight_orig", "weight_u", "weight_v")


def is_spectral_state(keys):
    """True when a state dict's keys are those of a spectrally normalised network."""
    return any(k.rsplit(".", 1)[-1] in SN_SUFFIXES for k in keys)


def check_state_keys(own_keys, file_keys, what="the discriminator"):
    """Refuse a checkpoint of the other kind: a plain file offered to a spectrally normalised network, or
    the reverse.  The RuntimeError names the keys the network needs and the file lacks."""
    own_keys, file_keys = list(own_keys), set(file_keys)
    if is_spectral_state(own_keys) == is_spectral_state(file_keys):
        return
    missing = [k for k in own_keys if k not in file_keys]
    if is_spectral_state(own_keys):
        raise RuntimeError("%s is spectrally normalised (--spectral_norm) but the checkpoint is not: missing keys %s"
                           % (what, missing))
    raise RuntimeError("the checkpoint is of a spectrally normalised network (--spectral_norm) but %s is not: "
                       "missing keys %s" % (what, missing))
