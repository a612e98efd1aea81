"""Shared pieces of the --norm batch tests and of tests/golden/gen_golden_v6.py (no test here):

  * ``d_spec_bn``: the state_dict (name, shape) list of the BatchNorm PatchGAN, in the reference's
    order (DSGAN/models/networks.py:533-579 -- bias-free convs in front of a BatchNorm2d);
  * ``d_params_bn``: its parameter recipe -- oracle.recipe.make_params(spec, "fanin", 5000) over the
    whole state_dict (so a conv tensor's seed is 5000 + its state_dict position), with the BatchNorm
    tensors, for which oracle/recipe.py has no rule, set here: weight = 1 + 0.2 N(0,1),
    bias = 0.1 N(0,1), running_mean = 0.1 N(0,1), running_var = 1 + 0.2 U(0,1), each from its own
    ``torch.Generator().manual_seed(6000 + position)``, num_batches_tracked = 0;
  * ``torch_patchgan_bn``: the discriminator restated in torch functional ops (any dtype, CPU),
    the fp64 reference of the parameter / input gradients.
"""
from collections import OrderedDict

import torch
import torch.nn.functional as F

from oracle.recipe import make_params

BN_SEED0 = 6000


def d_spec_bn(input_nc=6, ndf=32, n_layers=3):
    ch = [input_nc] + [ndf * min(2 ** n, 8) for n in range(n_layers + 1)] + [1]
    idx = [0] + [2 + 3 * i for i in range(len(ch) - 2)]
    sp = []
    for j, (i, ci, co) in enumerate(zip(idx, ch[:-1], ch[1:])):
        sp.append(("model.%d.weight" % i, (co, ci, 4, 4)))
        if j == 0 or j == len(idx) - 1:
            sp.append(("model.%d.bias" % i, (co,)))
        else:
            b = "model.%d." % (i + 1)
            sp += [(b + "weight", (co,)), (b + "bias", (co,)), (b + "running_mean", (co,)), (b + "running_var", (co,)),
                   (b + "num_batches_tracked", ())]
    return sp


def bn_indices(spec):
    """Sequential indices of the BatchNorm layers of a d_spec_bn list."""
    return [int(k.split(".")[1]) for k, _ in spec if k.endswith("running_mean")]


def d_params_bn(spec):
    p = make_params(spec, "fanin", 5000)
    bn = {"model.%d." % i for i in bn_indices(spec)}
    for i, (k, shp) in enumerate(spec):
        if k[:k.rindex(".") + 1] not in bn:
            continue
        g = torch.Generator().manual_seed(BN_SEED0 + i)
        if k.endswith(".weight"):
            p[k] = 1.0 + 0.2 * torch.randn(shp, generator=g)
        elif k.endswith(".bias") or k.endswith("running_mean"):
            p[k] = 0.1 * torch.randn(shp, generator=g)
        elif k.endswith("running_var"):
            p[k] = 1.0 + 0.2 * torch.rand(shp, generator=g)
        else:
            p[k] = torch.zeros((), dtype=torch.int64)
    return p


def torch_patchgan_bn(x, p, sigmoid, training=True):
    """The BatchNorm PatchGAN on ``x`` with the tensors of ``p`` (a d_params_bn dict in x's dtype;
    the running buffers are updated in place when training)."""
    convs = [int(k.split(".")[1]) for k in p if k.endswith(".weight") and p[k].dim() == 4]
    h = F.leaky_relu(F.conv2d(x, p["model.0.weight"], p["model.0.bias"], stride=2, padding=1), 0.2)
    mid = convs[1:-1]
    for j, i in enumerate(mid):
        b = "model.%d." % (i + 1)
        h = F.conv2d(h, p["model.%d.weight" % i], None, stride=2 if j < len(mid) - 1 else 1, padding=1)
        h = F.batch_norm(h, p[b + "running_mean"], p[b + "running_var"], p[b + "weight"], p[b + "bias"], training, 0.1, 1e-5)
        h = F.leaky_relu(h, 0.2)
    i = convs[-1]
    h = F.conv2d(h, p["model.%d.weight" % i], p["model.%d.bias" % i], stride=1, padding=1)
    return torch.sigmoid(h) if sigmoid else h


def torch_patchgan_bn_grads(x, params, dtype, sigmoid):
    """(output, {name: gradient, "input": input gradient}) in fp64 of the loss against the label
    True (least squares with the sigmoid, BCE-with-logits without), computed in ``dtype``."""
    p = OrderedDict()
    for k, v in params.items():
        p[k] = v.clone().to(dtype).requires_grad_() if v.is_floating_point() and "running" not in k else \
            (v.clone().to(dtype) if v.is_floating_point() else v.clone())
    x = x.clone().to(dtype).requires_grad_()
    o = torch_patchgan_bn(x, p, sigmoid)
    loss = torch.mean((o - 1.0) ** 2) if sigmoid else F.binary_cross_entropy_with_logits(o, torch.ones_like(o))
    loss.backward()
    g = OrderedDict((k, v.grad.double()) for k, v in p.items() if v.requires_grad)
    g["input"] = x.grad.double()
    return o.detach().double(), g
