"""Network factory, init, scheduler, GAN losses and the discriminators (DSGAN/models/networks.py).

Keeps the reference's string-dispatch surface (``define_G`` / ``define_D``, unknown names raise
``NotImplementedError``) for the networks on the DS-GAN path: ``MixConvNeXtML`` and every
discriminator ``Pix2PixModel`` can train under ``--norm instance``: the ``basic`` / ``n_layers``
PatchGAN, the ``pixel`` 1x1 discriminator and the three-scale ``multi`` discriminator, each with or
without the trailing ``nn.Sigmoid`` (``use_sigmoid``).  Both objectives are here: BCE-with-logits
(the default) and least squares (``GANLoss(use_lsgan=True)`` / ``GANLoss_multi``), which the
reference's backwards-wired ``--no_lsgan`` turns ON together with the sigmoid (quirk q3).  ``multi``
without the sigmoid raises: the reference pairs it with ``BCELoss`` on raw logits, which fails in
torch itself.  ``--norm batch`` builds the ``basic`` / ``n_layers`` PatchGAN on BatchNorm2d (fused
BatchNorm + LeakyReLU kernels, HF.batch_norm).  ``define_D(..., spectral_norm=True)`` (--spectral_norm)
builds any of them as an SN-PatchGAN: spectrally normalised conv holders (``SNConv2d``), no norm layer,
and a ``SpectralState`` that keeps W_sn current (csrc/spectral.hip).  ``define_G`` builds ``MixConvNeXtML`` and the
``unet_128`` U-Net (models/unet.py: PReLU, dropout and tanh on HIP kernels, either norm); the other
reference generators (``unet_256`` by name, the ResNets, ``gll``, ``cascaded``) are out of scope
 and raise the reference's own error.
"""
import functools
import math

import torch
import torch.nn as nn
from torch.nn import init
from torch.optim import lr_scheduler

from dsgan_hip import functional as HF
from .mixconvnext import MixConvNeXtML
from .unet import UnetGenerator, UnetSkipConnectionBlock  # noqa: F401  (the reference's names live here)


def get_norm_layer(norm_type="instance"):
    """DSGAN/models/networks.py:21-30."""
    if norm_type == "batch":
        return functools.partial(nn.BatchNorm2d, affine=True, track_running_stats=True)
    if norm_type == "instance":
        return functools.partial(nn.InstanceNorm2d, affine=False, track_running_stats=False)
    if norm_type == "none":
        return None
    raise NotImplementedError("normalization layer [%s] is not found" % norm_type)


def get_scheduler(optimizer, opt):
    """DSGAN/models/networks.py:33-46 (lambda rule kept verbatim in behaviour, quirk q4)."""
    if opt.lr_policy == "lambda":
        def lambda_rule(epoch):
            return 1.0 - max(0, epoch + 1 + opt.epoch_count - opt.niter) / float(opt.niter_decay + 1)
        return lr_scheduler.LambdaLR(optimizer, lr_lambda=lambda_rule)
    if opt.lr_policy == "step":
        return lr_scheduler.StepLR(optimizer, step_size=opt.lr_decay_iters, gamma=0.1)
    if opt.lr_policy == "plateau":
        return lr_scheduler.ReduceLROnPlateau(optimizer, mode="min", factor=0.2, threshold=0.01, patience=5)
    return NotImplementedError("learning rate policy [%s] is not implemented", opt.lr_policy)


def init_weights(net, init_type="normal", gain=0.02):
    """DSGAN/models/networks.py:49-70: Conv*/Linear weights ~ N(0, gain) (or xavier/kaiming/
    orthogonal), biases 0, applied post-order with ``net.apply``."""
    def init_func(m):
        classname = m.__class__.__name__
        if hasattr(m, "weight") and (classname.find("Conv") != -1 or classname.find("Linear") != -1):
            # (a spectrally normalised holder's parameter is weight_orig; its .weight is derived)
            w = m.weight_orig if isinstance(m, SNConv2d) else m.weight
            if init_type == "normal":
                init.normal_(w.data, 0.0, gain)
            elif init_type == "xavier":
                init.xavier_normal_(w.data, gain=gain)
            elif init_type == "kaiming":
                init.kaiming_normal_(w.data, a=0, mode="fan_in")
            elif init_type == "orthogonal":
                init.orthogonal_(w.data, gain=gain)
            else:
                raise NotImplementedError("initialization method [%s] is not implemented" % init_type)
            if hasattr(m, "bias") and m.bias is not None:
                init.constant_(m.bias.data, 0.0)
        elif classname.find("BatchNorm2d") != -1:
            init.normal_(m.weight.data, 1.0, gain)
            init.constant_(m.bias.data, 0.0)

    print("initialize network with %s" % init_type)
    net.apply(init_func)


def init_net(net, init_type="normal", gpu_ids=()):
    """DSGAN/models/networks.py:73-79, minus ``nn.DataParallel``: the build runs one process
    per GPU (torch.distributed over RCCL), so the net is moved to this rank's device only.

    The weights are drawn on the CPU generator BEFORE the move, i.e. exactly the reference's
    ``gpu_ids=[]`` init (module construction and the post-order N(0, 0.02) draws consume the
    global CPU RNG in the same order; pinned by tests/golden/golden_v2.npz INIT_*).  (The
    reference with GPUs draws from the CUDA generator after ``net.to``, which no CPU run can pin;
    every rank of a multi-GPU run draws the same values, and rank 0's are broadcast anyway.)"""
    init_weights(net, init_type)
    if len(gpu_ids) > 0:
        assert torch.cuda.is_available(), "gpu_ids given but no ROCm GPU is visible"
        net.to(torch.device("cuda", gpu_ids[0]))
    return net


def define_G(input_nc, output_nc, ngf, which_model_netG, norm="batch", use_dropout=False,
             init_type="normal", gpu_ids=()):
    """DSGAN/models/networks.py:81-113.  ``unet_128`` is the U-Net with 7 downsamplings (models/unet.py)
    under ``norm`` instance or batch.  ``unet_256`` (8 downsamplings) raises: ``UnetGenerator`` supports
    ``num_downs=8``, but the name is pinned as unsupported by the host test suite."""
    if which_model_netG == "MixConvNeXtML":
        netG = MixConvNeXtML()
    elif which_model_netG == "unet_128":
        if norm not in ("instance", "batch"):
            raise NotImplementedError("define_G: norm [%s] is not supported by the MI355X U-Net (instance or batch; "
                                      "[none] fails in the reference itself: norm_layer is None)" % norm)
        netG = UnetGenerator(input_nc, output_nc, 7, ngf, norm_layer=get_norm_layer(norm_type=norm),
                             use_dropout=use_dropout)
    elif which_model_netG == "unet_256":
        raise NotImplementedError(
            "Generator model name [unet_256] is not recognized: models.unet.UnetGenerator supports num_downs=8, "
            "but the name stays off because tests/test_host_cpu.py::test_unknown_networks_raise pins it to raise; "
            "use unet_128, or build UnetGenerator(input_nc, output_nc, 8, ngf, ...) directly")
    else:
        raise NotImplementedError("Generator model name [%s] is not recognized" % which_model_netG)
    return init_net(netG, init_type, gpu_ids)


def define_D(input_nc, ndf, which_model_netD, n_layers_D=3, norm="batch", use_sigmoid=False,
             init_type="normal", gpu_ids=(), spectral_norm=False):
    """DSGAN/models/networks.py:115-131.  The discriminators run InstanceNorm (affine=False, the
    reference default ``--norm instance``) fused into their conv kernels.  ``--norm batch`` (affine
    BatchNorm2d with running statistics, bias-free convs in front of it) is built for the ``basic`` /
    ``n_layers`` PatchGAN on the fused BatchNorm kernels (HF.batch_norm); ``pixel`` / ``multi`` with it,
    and ``none`` (which fails in the reference itself: ``norm_layer`` is None), raise instead of
    silently training a different discriminator.

    ``spectral_norm`` (--spectral_norm, a build extension) builds the SN-PatchGAN form of any of them:
    every conv a spectrally normalised holder (SNConv2d) with a bias, ``nn.Identity()`` where the norm
    layer stood (the Sequential indices and the keys do not move) and LeakyReLU in the conv epilogue;
    ``norm`` is then not looked at (it steers the generator only).  The returned net carries its
    SpectralState (``net.spectral``), refreshed once."""
    if spectral_norm:
        return _define_sn_D(input_nc, ndf, which_model_netD, n_layers_D, use_sigmoid, init_type, gpu_ids)
    if norm == "batch" and which_model_netD in ("pixel", "multi"):
        raise NotImplementedError("define_D: norm [batch] is not supported for the [%s] discriminator on the "
                                  "MI355X build (basic / n_layers only)" % which_model_netD)
    if norm not in ("instance", "batch"):
        raise NotImplementedError("define_D: norm [%s] is not supported by the MI355X PatchGAN "
                                  "(instance, the reference default, or batch)" % norm)
    norm_layer = get_norm_layer(norm_type=norm)
    if which_model_netD == "basic":
        netD = NLayerDiscriminator(input_nc, ndf, n_layers=3, norm_layer=norm_layer, use_sigmoid=use_sigmoid)
    elif which_model_netD == "n_layers":
        netD = NLayerDiscriminator(input_nc, ndf, n_layers_D, norm_layer=norm_layer, use_sigmoid=use_sigmoid)
    elif which_model_netD == "pixel":
        netD = PixelDiscriminator(input_nc, ndf, norm_layer=norm_layer, use_sigmoid=use_sigmoid)
    elif which_model_netD == "multi":
        if not use_sigmoid:
            raise NotImplementedError(
                "define_D: [multi] without --no_lsgan is not supported: the reference pairs it with "
                "GANLoss_multi's nn.BCELoss on raw logits, which fails in the reference itself "
                "(\"all elements of input should be between 0 and 1\"); pass --no_lsgan (sigmoid + least squares)")
        netD = MultiscaleDiscriminator(input_nc, ndf, n_layers_D, norm_layer, use_sigmoid, num_D=3, getIntermFeat=False)
    else:
        raise NotImplementedError("Discriminator model name [%s] is not recognized" % which_model_netD)
    return init_net(netD, init_type, gpu_ids)


def _define_sn_D(input_nc, ndf, which_model_netD, n_layers_D, use_sigmoid, init_type, gpu_ids):
    if which_model_netD == "basic":
        netD = NLayerDiscriminator(input_nc, ndf, n_layers=3, norm_layer=None, use_sigmoid=use_sigmoid, spectral_norm=True)
    elif which_model_netD == "n_layers":
        netD = NLayerDiscriminator(input_nc, ndf, n_layers_D, norm_layer=None, use_sigmoid=use_sigmoid,
                                   spectral_norm=True)
    elif which_model_netD == "pixel":
        netD = PixelDiscriminator(input_nc, ndf, norm_layer=None, use_sigmoid=use_sigmoid, spectral_norm=True)
    elif which_model_netD == "multi":
        if not use_sigmoid:
            raise NotImplementedError("define_D: [multi] without --no_lsgan is not supported (with or without "
                                      "--spectral_norm): pass --no_lsgan (sigmoid + least squares)")
        netD = MultiscaleDiscriminator(input_nc, ndf, n_layers_D, None, use_sigmoid, num_D=3, getIntermFeat=False,
                                       spectral_norm=True)
    else:
        raise NotImplementedError("Discriminator model name [%s] is not recognized" % which_model_netD)
    netD = init_net(netD, init_type, gpu_ids)
    netD.spectral = SpectralState(netD)
    return netD


class SNConv2d(nn.Module):
    """A conv holder whose ``.weight`` is the spectrally normalised W_sn = weight_orig / sigma.  Parameters
    and buffers carry torch.nn.utils.spectral_norm's names and order (``bias``, ``weight_orig``;
    ``weight_u``, ``weight_v``), so the state dict loads into the same conv wrapped by torch, and back.
    ``.weight`` is a plain tensor, not a parameter: a persistent leaf that the net's SpectralState
    rewrites in place (dsgan_hip.spectral states the function).  ``index``: the layer's number in its
    discriminator, which seeds the draw of the starting ``u``."""

    def __init__(self, in_channels, out_channels, kernel_size, stride=1, padding=0, index=0):
        super().__init__()
        from dsgan_hip import spectral as hsn
        k = int(kernel_size)
        self.in_channels, self.out_channels = int(in_channels), int(out_channels)
        self.kernel_size, self.stride, self.padding = (k, k), (int(stride),) * 2, (int(padding),) * 2
        self.index = int(index)
        ref = nn.Conv2d(in_channels, out_channels, k, stride, padding)   # the default init, the same RNG draws
        self.bias = nn.Parameter(ref.bias.detach().clone())
        self.weight_orig = nn.Parameter(ref.weight.detach().clone())
        self.register_buffer("weight_u", hsn.initial_u(self.index, out_channels))
        self.register_buffer("weight_v", torch.zeros(in_channels * k * k))
        self.weight = None   # set by SpectralState

    def forward(self, x):
        return nn.functional.conv2d(x, self.weight, self.bias, self.stride, self.padding)

    def extra_repr(self):
        return "%d, %d, kernel_size=%s, stride=%s, padding=%s, spectral_norm" % (
            self.in_channels, self.out_channels, self.kernel_size, self.stride, self.padding)


def spectral_weights(net):
    """The W_sn tensors of ``net``'s spectrally normalised convs ([] for a plain net)."""
    return [m.weight for m in net.modules() if isinstance(m, SNConv2d) and m.weight is not None]


class SpectralState:
    """What --spectral_norm keeps beside a discriminator's parameters, and the two batched calls over its
    layers (csrc/spectral.hip): ``refresh`` rewrites every layer's u, v, sigma and W_sn from the current
    ``weight_orig`` (once per weight version: at construction, after every optimizer step, ``iterate=False``
    after a load), ``backward`` folds the gradients the conv kernels accumulated into the W_sn leaves'
    ``.grad`` scratch into ``weight_orig.grad`` and leaves the scratch zeroed.

    W_sn, the scratch, sigma and the temporaries are persistent device buffers; the kernels find them
    through a device table of addresses, rebuilt when a parameter or buffer has moved (FlatParams rebinds
    the parameters into its flat buffers).  On the CPU (no hot path there: tests, state-dict handling)
    ``refresh`` runs dsgan_hip.spectral's torch reference and ``backward`` is not available."""

    def __init__(self, net):
        self.convs = [m for m in net.modules() if isinstance(m, SNConv2d)]
        if not self.convs:
            raise ValueError("SpectralState: the net has no spectrally normalised conv")
        self.device = self.convs[0].weight_orig.device
        self._bound, self._tab = None, None
        if self.device.type == "cuda":
            offs, n = [], 0
            for c in self.convs:   # every tensor on a 256-byte boundary, as FlatParams lays them
                offs.append(n)
                n += (c.weight_orig.numel() + 63) // 64 * 64
            self.wsn = torch.zeros(n, device=self.device, dtype=torch.float32)
            self.scratch = torch.zeros(n, device=self.device, dtype=torch.float32)
            self.sigma = torch.zeros(len(self.convs), device=self.device, dtype=torch.float32)
            for conv, off in zip(self.convs, offs):
                k, shape = conv.weight_orig.numel(), conv.weight_orig.shape
                conv.weight = self.wsn[off:off + k].view(shape).detach().requires_grad_(True)
                conv.weight.grad = self.scratch[off:off + k].view(shape)
        else:
            self.sigma = torch.zeros(len(self.convs))
        self.weights = None
        self.refresh(iterate=True)
        self.weights = [c.weight for c in self.convs]
        # a state dict loaded through nn.Module.load_state_dict brings its own (u, v): recompute W_sn
        net.register_load_state_dict_post_hook(lambda module, incompatible: self.refresh(iterate=False))

    def table(self):
        """The HF.SpectralTable over the layers, rebuilt when a parameter, its gradient or a buffer has moved."""
        for c in self.convs:
            if c.weight_orig.grad is None:   # a free-standing net: FlatParams binds .grad up front
                c.weight_orig.grad = torch.zeros_like(c.weight_orig)
        bound = tuple(t.data_ptr() for c in self.convs for t in (c.weight_orig, c.weight_orig.grad, c.weight_u, c.weight_v))
        if bound != self._bound:
            if torch.cuda.is_current_stream_capturing():
                raise RuntimeError("SpectralState: a parameter moved during a HIP graph capture")
            self._tab = HF.SpectralTable([(c.weight_orig.detach(), c.weight.detach(), c.weight_u, c.weight_v, c.weight.grad,
                                           c.weight_orig.grad) for c in self.convs], sigma=self.sigma)
            self._bound = bound
        return self._tab

    @torch.no_grad()
    def refresh(self, iterate=True):
        if self.device.type != "cuda":
            from dsgan_hip import spectral as hsn
            for i, c in enumerate(self.convs):
                w, u, v, s = hsn.refresh_torch(c.weight_orig.detach(), c.weight_u, c.weight_v, iterate)
                c.weight_u.copy_(u)
                c.weight_v.copy_(v)
                self.sigma[i] = s
                if c.weight is None:
                    c.weight = w.detach().clone()
                else:
                    c.weight.copy_(w)
            return
        self.table().refresh(iterate)
        if self.weights is not None:   # the cached tap-major and 16-bit copies of W_sn rebuild in place
            HF.bump_weight_generation(self.weights)

    @torch.no_grad()
    def backward(self):
        if self.device.type != "cuda":
            raise RuntimeError("SpectralState.backward needs a ROCm GPU (there is no CPU execution path)")
        self.table().backward()


def _fusable(*xs):
    """Loss terms HF.loss_sum takes: 0-d fp32 device tensors (a disabled term may be a python 0)."""
    ts = [x for x in xs if not (not torch.is_tensor(x) and x == 0)]
    return bool(ts) and len(ts) <= 8 and all(torch.is_tensor(x) and x.dim() == 0 and x.dtype == torch.float32
                                             and x.is_cuda for x in ts)


class GANLoss(nn.Module):
    """DSGAN/models/networks.py:143-163.  use_lsgan=False (the default, quirk q3) is
    BCEWithLogits against a constant label, use_lsgan=True (``--no_lsgan``) nn.MSELoss against it;
    both are fused HIP reductions."""

    def __init__(self, use_lsgan=True, target_real_label=1.0, target_fake_label=0.0):
        super().__init__()
        self.register_buffer("real_label", torch.tensor(target_real_label))
        self.register_buffer("fake_label", torch.tensor(target_fake_label))
        self.use_lsgan = use_lsgan
        self.labels = (float(target_fake_label), float(target_real_label))

    def __call__(self, input, target_is_real):
        if self.use_lsgan:
            return HF.mse_const(input, self.labels[1 if target_is_real else 0])
        return HF.bce_with_logits(input, 1.0 if target_is_real else 0.0)


class GANLoss_multi(nn.Module):
    """DSGAN/models/networks.py:166-208: the least-squares loss of the multi-scale D, summed over the
    scales in list order (``0 + l0 + l1 + l2``).  Takes the D's list of lists (the last entry of each
    scale is its prediction) or one scale's list."""

    def __init__(self, use_lsgan=True, target_real_label=1.0, target_fake_label=0.0, tensor=None):
        super().__init__()
        if not use_lsgan:
            raise NotImplementedError("GANLoss_multi(use_lsgan=False) is nn.BCELoss on the multi D's output, which "
                                      "the reference itself cannot train (define_D rejects that pairing)")
        self.real_label, self.fake_label = float(target_real_label), float(target_fake_label)

    def __call__(self, input, target_is_real):
        t = self.real_label if target_is_real else self.fake_label
        if not isinstance(input[0], list):
            return HF.mse_const(input[-1], t)
        ls = [HF.mse_const(input_i[-1], t) for input_i in input]
        if _fusable(*ls):   # one launch each way; 0 + l0 is l0
            return HF.loss_sum([(l, 1.0) for l in ls])
        loss = 0
        for l in ls:
            loss = loss + l
        return loss


def _patchgan_forward(model, plan, x, pad, sigmoid):
    """A PatchGAN Sequential on HIP kernels: implicit-GEMM 4x4 conv (+bias, +LeakyReLU(0.2) in the
    epilogue for layer 0), InstanceNorm + LeakyReLU fused (or, where the layer after the conv is a
    BatchNorm2d, the bias-free conv and BatchNorm + LeakyReLU fused), and the optional fp32 sigmoid."""
    h = x
    for idx, stride, use_in in plan:
        c = model[idx]
        if use_in is None:      # last conv: raw logits
            h = HF.conv2d(h, c.weight, c.bias, stride=stride, pad=pad)
        elif use_in and isinstance(model[idx + 1], nn.Identity):   # SN-PatchGAN: no norm layer, LeakyReLU in the epilogue
            h = HF.conv2d(h, c.weight, c.bias, stride=stride, pad=pad, act="lrelu")
        elif use_in and isinstance(model[idx + 1], nn.BatchNorm2d):
            h = HF.batch_norm(HF.conv2d(h, c.weight, None, stride=stride, pad=pad), model[idx + 1], act="lrelu")
        elif use_in:
            h = HF.instance_norm(HF.conv2d(h, c.weight, c.bias, stride=stride, pad=pad), act="lrelu")
        else:
            h = HF.conv2d(h, c.weight, c.bias, stride=stride, pad=pad, act="lrelu")
    return HF.sigmoid(h) if sigmoid else h


def has_batch_stats(net):
    """True when ``net`` normalises with statistics taken across the batch (a BatchNorm layer): its
    outputs for one sample then depend on the other samples of the pass."""
    return any(isinstance(m, nn.modules.batchnorm._BatchNorm) for m in net.modules())


def _sn_factories(spectral_norm, norm_layer, first=0):
    """(conv, norm) constructors of a discriminator: nn.Conv2d and ``norm_layer`` as they are, or, spectrally
    normalised, SNConv2d holders numbered from ``first`` in construction order (each with a bias,
    whatever ``bias=`` says) and nn.Identity in the norm layer's place."""
    if not spectral_norm:
        return nn.Conv2d, norm_layer
    count = [int(first)]

    def conv(cin, cout, kernel_size, stride=1, padding=0, bias=True):
        count[0] += 1
        return SNConv2d(cin, cout, kernel_size, stride, padding, index=count[0] - 1)

    return conv, (lambda ch: nn.Identity())


class NLayerDiscriminator(nn.Module):
    """PatchGAN D, DSGAN/models/networks.py:533-579.  Same ``model.<i>`` Sequential indices as
    the reference (conv holders at 0, 2, 5, 8, 11; ``use_sigmoid`` appends nn.Sigmoid as model.12),
    forward on HIP kernels (_patchgan_forward).  ``norm`` records which normalisation the plan's
    normalised layers use ("instance" or "batch")."""

    def __init__(self, input_nc, ndf=64, n_layers=3, norm_layer=nn.BatchNorm2d, use_sigmoid=False, spectral_norm=False):
        super().__init__()
        if type(norm_layer) == functools.partial:
            use_bias = norm_layer.func == nn.InstanceNorm2d
        else:
            use_bias = norm_layer == nn.InstanceNorm2d
        self.norm = "spectral" if spectral_norm else "instance" if use_bias else "batch"
        Conv2d, norm_layer = _sn_factories(spectral_norm, norm_layer)
        kw, padw = 4, 1
        seq = [Conv2d(input_nc, ndf, kernel_size=kw, stride=2, padding=padw), nn.LeakyReLU(0.2, True)]
        self.plan = [(0, 2, False)]  # (index, stride, normalised)
        nf_mult = 1
        for n in range(1, n_layers):
            nf_prev, nf_mult = nf_mult, min(2 ** n, 8)
            self.plan.append((len(seq), 2, True))
            seq += [Conv2d(ndf * nf_prev, ndf * nf_mult, kernel_size=kw, stride=2, padding=padw, bias=use_bias),
                    norm_layer(ndf * nf_mult), nn.LeakyReLU(0.2, True)]
        nf_prev, nf_mult = nf_mult, min(2 ** n_layers, 8)
        self.plan.append((len(seq), 1, True))
        seq += [Conv2d(ndf * nf_prev, ndf * nf_mult, kernel_size=kw, stride=1, padding=padw, bias=use_bias),
                norm_layer(ndf * nf_mult), nn.LeakyReLU(0.2, True)]
        self.plan.append((len(seq), 1, None))
        seq += [Conv2d(ndf * nf_mult, 1, kernel_size=kw, stride=1, padding=padw)]
        self.use_sigmoid = bool(use_sigmoid)
        if use_sigmoid:
            seq += [nn.Sigmoid()]
        self.model = nn.Sequential(*seq)

    def forward(self, x):
        return _patchgan_forward(self.model, self.plan, x, 1, self.use_sigmoid)


class NLayerDiscriminator_multi(nn.Module):
    """One scale of the multi-scale D, DSGAN/models/networks.py:582-631 (getIntermFeat=False): the
    PatchGAN with ``padw = ceil(1.5) = 2``, a bias on every conv and channels doubling up to 512."""

    def __init__(self, input_nc, ndf=64, n_layers=3, norm_layer=nn.BatchNorm2d, use_sigmoid=False, getIntermFeat=False,
                 spectral_norm=False, sn_first=0):
        super().__init__()
        if getIntermFeat:
            raise NotImplementedError("NLayerDiscriminator_multi: getIntermFeat=True is not on the DS-GAN path")
        self.n_layers = n_layers
        Conv2d, norm_layer = _sn_factories(spectral_norm, norm_layer, sn_first)
        kw = 4
        self.padw = padw = int(math.ceil((kw - 1.0) / 2))
        seq = [Conv2d(input_nc, ndf, kernel_size=kw, stride=2, padding=padw), nn.LeakyReLU(0.2, True)]
        self.plan = [(0, 2, False)]
        nf = ndf
        for n in range(1, n_layers):
            nf_prev, nf = nf, min(nf * 2, 512)
            self.plan.append((len(seq), 2, True))
            seq += [Conv2d(nf_prev, nf, kernel_size=kw, stride=2, padding=padw), norm_layer(nf),
                    nn.LeakyReLU(0.2, True)]
        nf_prev, nf = nf, min(nf * 2, 512)
        self.plan.append((len(seq), 1, True))
        seq += [Conv2d(nf_prev, nf, kernel_size=kw, stride=1, padding=padw), norm_layer(nf), nn.LeakyReLU(0.2, True)]
        self.plan.append((len(seq), 1, None))
        seq += [Conv2d(nf, 1, kernel_size=kw, stride=1, padding=padw)]
        self.use_sigmoid = bool(use_sigmoid)
        if use_sigmoid:
            seq += [nn.Sigmoid()]
        self.model = nn.Sequential(*seq)

    def forward(self, x):
        return _patchgan_forward(self.model, self.plan, x, self.padw, self.use_sigmoid)


class PixelDiscriminator(nn.Module):
    """DSGAN/models/networks.py:634-656: three 1x1 convs (``net.{0,2,5}``) on the pointwise kernels."""

    def __init__(self, input_nc, ndf=64, norm_layer=nn.BatchNorm2d, use_sigmoid=False, spectral_norm=False):
        super().__init__()
        if type(norm_layer) == functools.partial:
            use_bias = norm_layer.func == nn.InstanceNorm2d
        else:
            use_bias = norm_layer == nn.InstanceNorm2d
        self.spectral_norm = bool(spectral_norm)
        Conv2d, norm_layer = _sn_factories(spectral_norm, norm_layer)
        net = [Conv2d(input_nc, ndf, kernel_size=1, stride=1, padding=0), nn.LeakyReLU(0.2, True),
               Conv2d(ndf, ndf * 2, kernel_size=1, stride=1, padding=0, bias=use_bias), norm_layer(ndf * 2),
               nn.LeakyReLU(0.2, True),
               Conv2d(ndf * 2, 1, kernel_size=1, stride=1, padding=0, bias=use_bias)]
        self.use_sigmoid = bool(use_sigmoid)
        if use_sigmoid:
            net.append(nn.Sigmoid())
        self.net = nn.Sequential(*net)

    def forward(self, x):
        c0, c2, c5 = self.net[0], self.net[2], self.net[5]
        h = HF.conv2d(x, c0.weight, c0.bias, act="lrelu")
        if self.spectral_norm:   # no norm layer: LeakyReLU in the conv epilogue
            h = HF.conv2d(h, c2.weight, c2.bias, act="lrelu")
        else:
            h = HF.instance_norm(HF.conv2d(h, c2.weight, c2.bias), act="lrelu")
        h = HF.conv2d(h, c5.weight, c5.bias)
        return HF.sigmoid(h) if self.use_sigmoid else h


class MultiscaleDiscriminator(nn.Module):
    """DSGAN/models/networks.py:659-699 with num_D scales and getIntermFeat=False: ``layer<i>`` are
    the scales' Sequentials (keys ``layer{0,1,2}.{0,2,5,8,11}.{weight,bias}``); ``result[i]`` is
    ``[layer<num_D-1-i>(input pooled i times)]``, the pool AvgPool2d(3, 2, 1, count_include_pad=False)
    in one HIP pass per level.  An input that needs a gradient feeds a scale's stem conv and the next
    pool: the two data-grads meet in one buffer (HF.share)."""

    def __init__(self, input_nc, ndf=64, n_layers=3, norm_layer=nn.BatchNorm2d, use_sigmoid=False, num_D=3,
                 getIntermFeat=False, spectral_norm=False):
        super().__init__()
        if getIntermFeat:
            raise NotImplementedError("MultiscaleDiscriminator: getIntermFeat=True is not on the DS-GAN path")
        self.num_D, self.n_layers, self.getIntermFeat = num_D, n_layers, False
        self.use_sigmoid = bool(use_sigmoid)
        for i in range(num_D):
            netD = NLayerDiscriminator_multi(input_nc, ndf, n_layers, norm_layer, use_sigmoid, False,
                                             spectral_norm=spectral_norm, sn_first=i * (n_layers + 2))
            setattr(self, "layer" + str(i), netD.model)
            self.plan, self.padw = netD.plan, netD.padw
        self.downsample = nn.AvgPool2d(3, stride=2, padding=[1, 1], count_include_pad=False)

    def forward(self, input):
        result = []
        x = input
        for i in range(self.num_D):
            last = i == self.num_D - 1
            if not last and torch.is_grad_enabled() and x.requires_grad:
                x = HF.share(x)
            model = getattr(self, "layer" + str(self.num_D - 1 - i))
            result.append([_patchgan_forward(model, self.plan, x, self.padw, self.use_sigmoid)])
            if not last:
                x = HF.avg_pool3s2(x)
        return result
