"""The U-Net generator (DSGAN/models/networks.py:445-529): ``--which_model_netG unet_128``.

The module tree is the reference's -- ``nn.Conv2d`` / ``nn.ConvTranspose2d`` / ``nn.PReLU`` / the norm
layer / ``nn.Dropout`` / ``nn.Tanh`` nested in ``model`` Sequentials -- so ``state_dict()`` keys, shapes
and order, the post-order draw of ``init_weights`` and reference checkpoints are the reference's.  The
modules are parameter containers only; the forward runs on the HIP ops of dsgan_hip.functional.

What the forward computes is the reference's arithmetic, not the textbook U-Net: ``downrelu`` is
``nn.LeakyReLU(0.2, True)`` and runs IN PLACE on the block's input before ``torch.cat([x, model(x)], 1)``
reads it, so the skip half of every concatenation is ``lrelu(x)`` and the parent's PReLU sees
``cat(lrelu(x), up)``.  Here each activated tensor h = lrelu(.) is produced once, by the epilogue of the
kernel in front of it (the stem conv, or the block's ``downnorm``), and read twice: by the child's down
conv and, as the skip half, by the parent's PReLU (``HF.prelu_cat(h, up, weight)`` reads the two halves
where they lie: the concatenation itself is never materialised).  ``uprelu`` is ``nn.PReLU()``: one
learnable slope per block, a parameter of the net like any other.

Dropout draws from a counter-based generator (HF.DropoutState): the seed is torch's seed at
construction, each dropout layer has its own stream id (rank << 16 | layer index) and a device-side
call counter, a non-persistent buffer that never appears in ``state_dict()``.
"""
import functools

import torch
import torch.nn as nn

from dsgan_hip import dist as hdist
from dsgan_hip import functional as HF


def _shared(h):
    """h feeds the child's down conv and the parent's PReLU: one gradient buffer for the two."""
    return HF.share(h) if torch.is_grad_enabled() and h.requires_grad else h


def _norm(layer, z, act):
    if isinstance(layer, nn.BatchNorm2d):
        return HF.batch_norm(z, layer, act=act)
    if isinstance(layer, nn.InstanceNorm2d) and not layer.affine and not layer.track_running_stats:
        if z.shape[2] * z.shape[3] == 1:   # torch's own error (F.instance_norm), before any launch
            raise ValueError("Expected more than 1 spatial element when training, got input size %s"
                             % (torch.Size(z.shape),))
        return HF.instance_norm(z, act=act)
    raise NotImplementedError("UnetGenerator: norm layer %s is not on the HIP path (get_norm_layer's "
                              "'instance' or 'batch')" % type(layer).__name__)


def _down(conv, h, act=None):
    H, W = h.shape[2], h.shape[3]
    if H + 2 < 4 or W + 2 < 4:   # torch's own error (conv2d), before any launch
        raise RuntimeError("Calculated padded input size per channel: (%d x %d). Kernel size: (4 x 4). Kernel size "
                           "can't be greater than actual input size" % (H + 2, W + 2))
    return HF.conv2d(h, conv.weight, conv.bias, stride=2, pad=1, act=act)


class UnetSkipConnectionBlock(nn.Module):
    """DSGAN/models/networks.py:478-529.  ``model`` holds the reference's layers at the reference's
    indices.  The outermost block is the net's forward; an inner block runs through ``_run``, which
    takes the block's input already activated, h = lrelu(x), and returns the up branch (the parent
    pairs it with h)."""

    def __init__(self, outer_nc, inner_nc, input_nc=None, submodule=None, outermost=False, innermost=False,
                 norm_layer=nn.BatchNorm2d, use_dropout=False):
        super().__init__()
        self.outermost, self.innermost = outermost, innermost
        if type(norm_layer) == functools.partial:
            use_bias = norm_layer.func == nn.InstanceNorm2d
        else:
            use_bias = norm_layer == nn.InstanceNorm2d
        if input_nc is None:
            input_nc = outer_nc
        downconv = nn.Conv2d(input_nc, inner_nc, kernel_size=4, stride=2, padding=1, bias=use_bias)
        downrelu = nn.LeakyReLU(0.2, True)
        downnorm = norm_layer(inner_nc)
        uprelu = nn.PReLU()
        upnorm = norm_layer(outer_nc)
        drop = None
        if outermost:
            upconv = nn.ConvTranspose2d(inner_nc * 2, outer_nc, kernel_size=4, stride=2, padding=1)
            model = [downconv, submodule, uprelu, upconv, nn.Tanh()]
            downnorm = upnorm = None
        elif innermost:
            upconv = nn.ConvTranspose2d(inner_nc, outer_nc, kernel_size=4, stride=2, padding=1, bias=use_bias)
            model = [downrelu, downconv, uprelu, upconv, upnorm]
            downnorm = None
        else:
            upconv = nn.ConvTranspose2d(inner_nc * 2, outer_nc, kernel_size=4, stride=2, padding=1, bias=use_bias)
            model = [downrelu, downconv, downnorm, submodule, uprelu, upconv, upnorm]
            if use_dropout:
                drop = nn.Dropout(0.5)
                model.append(drop)
        self.model = nn.Sequential(*model)
        # the layers by role (a tuple: not registered a second time)
        self._parts = (downconv, downnorm, submodule, uprelu, upconv, upnorm, drop)
        self.drop_seed, self.drop_stream = 0, 0
        if drop is not None:
            self.register_buffer("drop_counter", torch.zeros(1, dtype=torch.int64), persistent=False)

    def _run(self, h):
        downconv, downnorm, sub, uprelu, upconv, upnorm, drop = self._parts
        z = _down(downconv, h)
        if self.innermost:
            p = HF.prelu(z, uprelu.weight)
        else:
            hn = _shared(_norm(downnorm, z, "lrelu"))   # the child's in-place LeakyReLU, in the norm's epilogue
            p = HF.prelu_cat(hn, sub._run(hn), uprelu.weight)
        u = _norm(upnorm, HF.conv_transpose4s2(p, upconv.weight, upconv.bias), None)
        if drop is not None:
            u = HF.dropout(u, drop.p, HF.DropoutState(self.drop_seed, self.drop_stream, self.drop_counter),
                           self.training)
        return u

    def forward(self, x):
        if not self.outermost:
            raise NotImplementedError("UnetSkipConnectionBlock: an inner block runs inside UnetGenerator (its input "
                                      "is the parent's activated tensor)")
        downconv, _, sub, uprelu, upconv, _, _ = self._parts
        h = _shared(_down(downconv, x, act="lrelu"))   # the stem conv + the child's in-place LeakyReLU
        p = HF.prelu_cat(h, sub._run(h), uprelu.weight)
        return HF.tanh(HF.conv_transpose4s2(p, upconv.weight, upconv.bias))


class UnetGenerator(nn.Module):
    """DSGAN/models/networks.py:449-472: ``num_downs`` stride-2 levels (a 2^num_downs image reaches
    1x1 at the bottleneck); ``num_downs - 5`` middle blocks at ngf*8 carry the dropout."""

    def __init__(self, input_nc, output_nc, num_downs, ngf=64, norm_layer=nn.BatchNorm2d, use_dropout=False):
        super().__init__()
        if norm_layer is None:
            raise NotImplementedError("UnetGenerator: norm [none] is not supported (the reference itself fails: "
                                      "norm_layer is None)")
        blk = UnetSkipConnectionBlock(ngf * 8, ngf * 8, norm_layer=norm_layer, innermost=True)
        for _ in range(num_downs - 5):
            blk = UnetSkipConnectionBlock(ngf * 8, ngf * 8, submodule=blk, norm_layer=norm_layer,
                                          use_dropout=use_dropout)
        blk = UnetSkipConnectionBlock(ngf * 4, ngf * 8, submodule=blk, norm_layer=norm_layer)
        blk = UnetSkipConnectionBlock(ngf * 2, ngf * 4, submodule=blk, norm_layer=norm_layer)
        blk = UnetSkipConnectionBlock(ngf, ngf * 2, submodule=blk, norm_layer=norm_layer)
        self.model = UnetSkipConnectionBlock(output_nc, ngf, input_nc=input_nc, submodule=blk, outermost=True,
                                             norm_layer=norm_layer)
        # dropout streams: torch's seed now, one stream id per dropout layer (outermost first)
        seed, idx = torch.initial_seed(), 0
        for m in self.modules():
            if isinstance(m, UnetSkipConnectionBlock) and m._parts[6] is not None:
                m.drop_seed, m.drop_stream = seed, (hdist.rank() << 16) | idx
                idx += 1

    def dropout_blocks(self):
        """The blocks that carry a dropout layer, outermost first (their stream ids count up from 0)."""
        return [m for m in self.modules() if isinstance(m, UnetSkipConnectionBlock) and m._parts[6] is not None]

    def forward(self, input):
        return self.model(input)
