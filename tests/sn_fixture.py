"""A plain-torch CPU restatement of the spectrally normalised discriminators (--spectral_norm), for the
GPU tests: F.conv2d on W_sn = W / sigma of dsgan_hip.spectral's reference, LeakyReLU(0.2), no norm layer,
the optional sigmoid; autograd runs through W / sigma with u and v constants, as in torch's wrapper.
float64 throughout.  Also the shared parameter recipe (fan-in weights, unit u, v consistent with them)."""
from collections import OrderedDict

import torch
import torch.nn.functional as F

from oracle.recipe import make_params

from dsgan_hip import spectral as SN

# (state-dict prefix of the conv, stride, LeakyReLU after it) per Sequential
PATCH = [("0.", 2, True), ("2.", 2, True), ("5.", 2, True), ("8.", 1, True), ("11.", 1, False)]
PIXEL = [("0.", 1, True), ("2.", 1, True), ("5.", 1, False)]


def sn_params(net, seed=5000):
    """Values for ``net.state_dict()``: fan-in weights and biases (oracle.recipe), each layer's seeded
    starting u (dsgan_hip.spectral.initial_u, what the constructor drew) and the v one power iteration of
    the float64 reference gives from it -- a consistent (W, u, v) as a checkpoint holds."""
    spec = [(k, tuple(v.shape)) for k, v in net.state_dict().items()]
    p = make_params(spec, "fanin", seed)
    out = OrderedDict()
    convs = [k[:-len("weight_orig")] for k, _ in spec if k.endswith("weight_orig")]
    for k, _ in spec:
        out[k] = p[k].clone()
    for i, pre in enumerate(convs):
        W = out[pre + "weight_orig"].double().numpy()
        _, u, v, _ = SN.refresh(W, SN.initial_u(i, W.shape[0]).double().numpy())
        out[pre + "weight_u"] = torch.from_numpy(u).float()
        out[pre + "weight_v"] = torch.from_numpy(v).float()
    return out


class RefSND:
    """``kind``: basic / pixel / multi; ``params``: the net's state dict (any float dtype)."""

    def __init__(self, kind, params, use_sigmoid):
        self.kind, self.sigmoid = kind, bool(use_sigmoid)
        self.p = OrderedDict((k, v.detach().clone().double().cpu()) for k, v in params.items())
        for k, v in self.p.items():
            if k.endswith(("weight_orig", "bias")):
                v.requires_grad_(True)
        if kind == "basic":
            self.seqs = [("model.", PATCH, 1)]
        elif kind == "pixel":
            self.seqs = [("net.", PIXEL, 0)]
        else:   # result[i] = layer<2 - i>(input pooled i times)
            self.seqs = [("layer%d." % (2 - i), PATCH, 2) for i in range(3)]
        self.layers = [k[:-len("weight_orig")] for k in self.p if k.endswith("weight_orig")]

    def parameters(self):
        return [v for v in self.p.values() if v.requires_grad]

    def named_parameters(self):
        return [(k, v) for k, v in self.p.items() if v.requires_grad]

    def refresh(self, iterate=True):
        with torch.no_grad():
            for pre in self.layers:
                _, u, v, _ = SN.refresh_torch(self.p[pre + "weight_orig"], self.p[pre + "weight_u"],
                                              self.p[pre + "weight_v"], iterate)
                self.p[pre + "weight_u"], self.p[pre + "weight_v"] = u, v

    def w_sn(self, pre):
        """(W_sn attached to weight_orig, sigma) with the stored (u, v)."""
        w, _, _, s = SN.refresh_torch(self.p[pre + "weight_orig"], self.p[pre + "weight_u"], self.p[pre + "weight_v"], False)
        return w, s

    def sigmas(self):
        with torch.no_grad():
            return torch.stack([self.w_sn(pre)[1] for pre in self.layers])

    def _seq(self, x, prefix, plan, pad):
        h = x
        for name, stride, act in plan:
            w, _ = self.w_sn(prefix + name)
            h = F.conv2d(h, w, self.p[prefix + name + "bias"], stride=stride, padding=pad)
            if act:
                h = F.leaky_relu(h, 0.2)
        return torch.sigmoid(h) if self.sigmoid else h

    def __call__(self, x):
        """The predictions, one per scale (a list of one for basic / pixel)."""
        outs = []
        for i, (prefix, plan, pad) in enumerate(self.seqs):
            outs.append(self._seq(x, prefix, plan, pad))
            if i + 1 < len(self.seqs):
                x = F.avg_pool2d(x, 3, 2, 1, count_include_pad=False)
        return outs


def gan_loss(outs, target, lsgan):
    """GANLoss / GANLoss_multi on the list of predictions: BCE-with-logits, or least squares summed over
    the scales."""
    t = 1.0 if target else 0.0
    if lsgan:
        return sum(torch.mean((o - t) ** 2) for o in outs)
    (o,) = outs
    return F.binary_cross_entropy_with_logits(o, torch.full_like(o, t))
