"""Shared pieces of the U-Net generator tests and of tests/golden/gen_golden_v7.py (no test here):

  * ``unet_levels`` / ``unet_spec``: the state_dict (name, shape) list of
    ``UnetGenerator(input_nc, output_nc, num_downs, ngf, norm_layer, use_dropout)`` in the reference's
    order (DSGAN/models/networks.py:445-529): convs carry a bias only under InstanceNorm, the outermost
    ConvTranspose2d always does, every block has one (1,) PReLU weight, BatchNorm layers add their
    affine pair and three buffers, dropout adds nothing;
  * ``unet_params``: the parameter recipe -- oracle.recipe.make_params(spec, "fanin", 8000) over the
    whole state_dict, then the tensors that recipe has no rule for, each from its own
    ``torch.Generator().manual_seed(9000 + position)``: PReLU weight = 0.25 + 0.15 N(0,1) (not all 0.25,
    some negative), BatchNorm weight = 1 + 0.2 N(0,1), bias = 0.1 N(0,1), running_mean = 0.1 N(0,1),
    running_var = 1 + 0.2 U(0,1), num_batches_tracked = 0;
  * ``torch_unet``: the network restated in torch functional ops (any dtype, CPU) WITH the reference's
    in-place quirk: ``downrelu`` is ``nn.LeakyReLU(0.2, True)`` and mutates the block's input before
    ``torch.cat([x, model(x)], 1)`` reads it, so the skip half is lrelu(x).  Dropout is a multiply by a
    supplied 0/1 mask and by 2;
  * ``philox_mask``: the numpy twin of the dropout kernels' mask (HF.dropout_mask).
"""
from collections import OrderedDict

import numpy as np
import torch
import torch.nn.functional as F

from oracle.recipe import make_params

UNET_SEED0, UNET_SEED1 = 8000, 9000


def unet_levels(input_nc, output_nc, num_downs, ngf, use_dropout=False):
    """[(kind, outer_nc, inner_nc, input_nc, dropout)] from the outermost block inwards."""
    lv = [("outer", output_nc, ngf, input_nc, False), ("mid", ngf, ngf * 2, ngf, False),
          ("mid", ngf * 2, ngf * 4, ngf * 2, False), ("mid", ngf * 4, ngf * 8, ngf * 4, False)]
    lv += [("mid", ngf * 8, ngf * 8, ngf * 8, bool(use_dropout))] * (num_downs - 5)
    return lv + [("inner", ngf * 8, ngf * 8, ngf * 8, False)]


# Sequential indices of (downconv, downnorm, submodule, uprelu, upconv, upnorm) per block kind
_IDX = {"outer": (0, None, 1, 2, 3, None), "mid": (1, 2, 3, 4, 5, 6), "inner": (1, None, None, 2, 3, 4)}


def _bn_entries(prefix, c):
    return [(prefix + "weight", (c,)), (prefix + "bias", (c,)), (prefix + "running_mean", (c,)),
            (prefix + "running_var", (c,)), (prefix + "num_batches_tracked", ())]


def unet_spec(input_nc, output_nc, num_downs, ngf, norm, use_dropout=False):
    use_bias = norm == "instance"

    def block(levels, pre):
        kind, outer, inner, inp, _ = levels[0]
        dc, dn, sub, pr, uc, un = _IDX[kind]
        sp = [(pre + "%d.weight" % dc, (inner, inp, 4, 4))]
        if use_bias:
            sp.append((pre + "%d.bias" % dc, (inner,)))
        if dn is not None and norm == "batch":
            sp += _bn_entries(pre + "%d." % dn, inner)
        if sub is not None:
            sp += block(levels[1:], pre + "%d.model." % sub)
        sp.append((pre + "%d.weight" % pr, (1,)))
        sp.append((pre + "%d.weight" % uc, (inner if kind == "inner" else inner * 2, outer, 4, 4)))
        if use_bias or kind == "outer":
            sp.append((pre + "%d.bias" % uc, (outer,)))
        if un is not None and norm == "batch":
            sp += _bn_entries(pre + "%d." % un, outer)
        return sp

    return block(unet_levels(input_nc, output_nc, num_downs, ngf, use_dropout), "model.model.")


def unet_params(spec):
    p = make_params(spec, "fanin", UNET_SEED0)
    bn = {k[:-len("running_mean")] for k, _ in spec if k.endswith("running_mean")}
    for i, (k, shp) in enumerate(spec):
        g = torch.Generator().manual_seed(UNET_SEED1 + i)
        if k[:k.rindex(".") + 1] in bn:
            if k.endswith(".weight"):
                p[k] = 1.0 + 0.2 * torch.randn(shp, generator=g)
            elif k.endswith(".bias") or k.endswith("running_mean"):
                p[k] = 0.1 * torch.randn(shp, generator=g)
            elif k.endswith("running_var"):
                p[k] = 1.0 + 0.2 * torch.rand(shp, generator=g)
            else:
                p[k] = torch.zeros((), dtype=torch.int64)
        elif tuple(shp) == (1,):
            p[k] = 0.25 + 0.15 * torch.randn(shp, generator=g)
    return p


def prelu_keys(spec):
    return [k for k, shp in spec if tuple(shp) == (1,)]


def conv_bias_before_instnorm(spec, norm):
    """The conv / ConvTranspose biases an InstanceNorm follows directly (a mathematically zero
    gradient): every bias but the outermost block's two and the innermost down conv's."""
    if norm != "instance":
        return []
    b = [k for k, shp in spec if k.endswith(".bias")]
    depth = max(k.count("model.") for k in b)
    inner_down = [k for k in b if k.count("model.") == depth and k.endswith(".1.bias")]
    return [k for k in b if k not in ("model.model.0.bias", "model.model.3.bias") and k not in inner_down]


def torch_unet(x, p, levels, norm, masks=None, training=True, zlog=None):
    """The network on ``x`` with the tensors of ``p`` (an unet_params dict in x's dtype; BatchNorm
    buffers are updated in place when training).  ``masks``: one 0/1 tensor per dropout block,
    outermost first (None: no dropout).  ``zlog`` (a list) receives min |input| of every LeakyReLU
    and PReLU."""
    masks = list(masks) if masks is not None else None

    def note(t):
        if zlog is not None:
            zlog.append(float(t.detach().abs().min()))

    def nrm(t, pre):
        if norm == "instance":
            return F.instance_norm(t, eps=1e-5)
        if training:
            p[pre + "num_batches_tracked"] += 1
        return F.batch_norm(t, p[pre + "running_mean"], p[pre + "running_var"], p[pre + "weight"], p[pre + "bias"],
                            training, 0.1, 1e-5)

    def block(li, x, pre):
        kind, _, _, _, drop = levels[li]
        dc, dn, sub, pr, uc, un = _IDX[kind]
        if kind != "outer":
            note(x)
            x = F.leaky_relu(x, 0.2)   # in place in the reference: the skip half below is lrelu(x)
        z = F.conv2d(x, p[pre + "%d.weight" % dc], p.get(pre + "%d.bias" % dc), stride=2, padding=1)
        if dn is not None:
            z = nrm(z, pre + "%d." % dn)
        if sub is not None:
            z = block(li + 1, z, pre + "%d.model." % sub)
        note(z)
        u = F.conv_transpose2d(F.prelu(z, p[pre + "%d.weight" % pr]), p[pre + "%d.weight" % uc],
                               p.get(pre + "%d.bias" % uc), stride=2, padding=1)
        if kind == "outer":
            return torch.tanh(u)
        u = nrm(u, pre + "%d." % un)
        if drop and masks is not None:
            u = u * masks.pop(0).to(u.dtype) * 2.0
        return torch.cat([x, u], 1)

    return block(0, x, "model.model.")


def torch_unet_grads(x, params, levels, norm, dtype, masks=None):
    """(output, {name: gradient, "input": input gradient}, buffers) in fp64, for the loss
    sum(out * probe) / numel with the fixed probe cos(0.37 i + 0.11): computed in ``dtype``."""
    p = OrderedDict()
    for k, v in params.items():
        fl = v.is_floating_point()
        p[k] = v.clone().to(dtype).requires_grad_() if fl and "running" not in k else (v.clone().to(dtype) if fl else v.clone())
    x = x.clone().to(dtype).requires_grad_()
    o = torch_unet(x, p, levels, norm, masks)
    (o * loss_probe(o.shape).to(dtype)).sum().div(o.numel()).backward()
    g = OrderedDict((k, v.grad.double()) for k, v in p.items() if v.requires_grad)
    g["input"] = x.grad.double()
    buf = OrderedDict((k, v.detach().double()) for k, v in p.items() if "running" in k or "tracked" in k)
    return o.detach().double(), g, buf


def out_view(t):
    """What golden_v7 stores of a network output [N, C, S, S]: all of it up to 32^2, every second row and
    column above (keeps the file within the size range of the other goldens); the full tensor's norm is
    stored beside it."""
    return t if t.shape[-1] <= 32 else t[..., ::2, ::2]


def loss_probe(shape):
    n = int(np.prod(shape))
    return torch.cos(0.37 * torch.arange(n, dtype=torch.float64) + 0.11).reshape(tuple(shape))


def unet_conv_calls(N, size, input_nc, output_nc, num_downs, ngf, norm="instance"):
    """The plain inputs of every conv_{fwd,dgrad,wgrad}_family question the U-Net's train step asks
    (dense tensors at 256-byte aligned addresses, offset 0), as rows {"layer", "op", ...kwargs}:
    per level the down conv (forward, data-grad, weight-grad) and the ConvTranspose (its forward is a
    data-grad, its input grad a forward conv, its weight-grad has x and dy swapped).  An inner level's
    down-conv data-grad accumulates into the gradient buffer the parent's PReLU backward wrote (batch
    stride twice the tensor's); the stem's input needs no gradient.  ``pbs`` / ``gbs`` are 0 and the
    epilogue pointers None: no U-Net conv has a fused pre-activation."""
    bias = norm == "instance"
    rows = []
    s = size
    for li, (kind, outer, inner, inp, _) in enumerate(unet_levels(input_nc, output_nc, num_downs, ngf)):
        h = s // 2
        name = "L%d" % li
        fwd = dict(Cin=inp, H=s, W=s, Cout=inner, KH=4, KW=4, stride=2, pad=1, xbs=inp * s * s, ybs=inner * h * h,
                   pbs=0, x_ptr=0, y_ptr=0, w_ptr=0, pre_ptr=None, w_dim=4, w_contig=True,
                   act="lrelu" if kind == "outer" else None, xact=None, accumulate=False)
        rows.append(dict(layer=name + ".down", op="fwd", **fwd))
        if kind != "outer":
            rows.append(dict(layer=name + ".down", op="dgrad", Cin=inp, H=s, W=s, Cout=inner, KH=4, KW=4, stride=2, pad=1,
                             Ho=h, Wo=h, dybs=inner * h * h, dxbs=2 * inp * s * s, gbs=0, dy_ptr=0, dx_ptr=0, w_ptr=0,
                             gpre_ptr=None, w_dim=4, w_contig=True, act=None, has_bias=False, accumulate=True))
        rows.append(dict(layer=name + ".down", op="wgrad", N=N, Cin=inp, H=s, W=s, Cout=inner, KH=4, KW=4, stride=2, pad=1,
                         dybs=inner * h * h, xbs=inp * s * s, dy_ptr=0, x_ptr=0, w_dim=4, w_contig=True, xact=None,
                         has_db=bias))
        cin_t = inner if kind == "inner" else 2 * inner   # the ConvTranspose's input channels
        up_bias = bias or kind == "outer"
        rows.append(dict(layer=name + ".up", op="dgrad", Cin=outer, H=s, W=s, Cout=cin_t, KH=4, KW=4, stride=2, pad=1,
                         Ho=h, Wo=h, dybs=cin_t * h * h, dxbs=outer * s * s, gbs=0, dy_ptr=0, dx_ptr=0, w_ptr=0,
                         gpre_ptr=None, w_dim=4, w_contig=True, act=None, has_bias=up_bias, accumulate=False))
        rows.append(dict(layer=name + ".up", op="fwd", Cin=outer, H=s, W=s, Cout=cin_t, KH=4, KW=4, stride=2, pad=1,
                         xbs=outer * s * s, ybs=cin_t * h * h, pbs=0, x_ptr=0, y_ptr=0, w_ptr=0, pre_ptr=None, w_dim=4,
                         w_contig=True, act=None, xact=None, accumulate=False))
        rows.append(dict(layer=name + ".up", op="wgrad", N=N, Cin=outer, H=s, W=s, Cout=cin_t, KH=4, KW=4, stride=2, pad=1,
                         dybs=cin_t * h * h, xbs=outer * s * s, dy_ptr=0, x_ptr=0, w_dim=4, w_contig=True, xact=None,
                         has_db=False))
        s = h
    return rows


# ---- the dropout mask: Philox-4x32-10, key = seed, counter = (group lo, group hi, call counter, stream) ----
_M0, _M1, _W0, _W1 = 0xD2511F53, 0xCD9E8D57, 0x9E3779B9, 0xBB67AE85
_U32 = np.uint64(0xFFFFFFFF)


def philox_words(g, seed, stream, counter):
    """[len(g), 4] uint64 (values < 2^32): the generator's four output words for the groups ``g``."""
    g = np.asarray(g, dtype=np.uint64)
    seed = int(seed) & (2 ** 63 - 1)
    c = [g & _U32, g >> np.uint64(32), np.full_like(g, int(counter) & 0xFFFFFFFF), np.full_like(g, int(stream))]
    k0, k1 = seed & 0xFFFFFFFF, seed >> 32
    for _ in range(10):
        p0, p1 = np.uint64(_M0) * c[0], np.uint64(_M1) * c[2]
        c = [(p1 >> np.uint64(32)) ^ c[1] ^ np.uint64(k0), p1 & _U32, (p0 >> np.uint64(32)) ^ c[3] ^ np.uint64(k1), p0 & _U32]
        k0, k1 = (k0 + _W0) & 0xFFFFFFFF, (k1 + _W1) & 0xFFFFFFFF
    return np.stack(c, 1)


def philox_mask(shape, seed, stream, counter, p=0.5):
    """1.0 where the element is kept: element i (row-major over ``shape``) looks at word i & 3 of
    the generator's output for group i >> 2, kept iff word >= round(p * 2^32)."""
    n = int(np.prod(shape))
    words = philox_words(np.arange((n + 3) // 4, dtype=np.uint64), seed, stream, counter).reshape(-1)[:n]
    return (words >=np.uint64(int(round(float(p) * 2.0 ** 32)))).astype(np.float32).reshape(tuple(shape))
