"""Training flags (DSGAN/options/train_options.py:5-27), unchanged names and defaults."""
from .base_options import BaseOptions


class TrainOptions(BaseOptions):
    def initialize(self, parser):
        parser = BaseOptions.initialize(self, parser)
        parser.add_argument("--display_freq", type=int, default=100, help="frequency of showing training results on screen")
        parser.add_argument("--display_ncols", type=int, default=4, help="images per row in the web display")
        parser.add_argument("--update_html_freq", type=int, default=1000, help="frequency of saving training results to html")
        parser.add_argument("--print_freq", type=int, default=100, help="frequency of showing training results on console")
        parser.add_argument("--save_latest_freq", type=int, default=5000, help="frequency of saving the latest results")
        parser.add_argument("--save_epoch_freq", type=int, default=50, help="frequency of saving checkpoints at the end of epochs")
        parser.add_argument("--continue_train", action="store_true", default=False, help="continue training: load the latest model")
        parser.add_argument("--epoch_count", type=int, default=1, help="the starting epoch count")
        parser.add_argument("--phase", type=str, default="train_all/", help="train, val, test, etc")
        parser.add_argument("--which_epoch", type=str, default="1", help="which epoch to load?")
        parser.add_argument("--niter", type=int, default=10, help="# of iter at starting learning rate")
        parser.add_argument("--niter_decay", type=int, default=10, help="# of iter to linearly decay learning rate to zero")
        parser.add_argument("--beta1", type=float, default=0.5, help="momentum term of adam")
        parser.add_argument("--lr", type=float, default=0.0002, help="initial learning rate for adam")
        parser.add_argument("--no_lsgan", action="store_true", help="do *not* use least square GAN, if false, use vanilla GAN")
        parser.add_argument("--pool_size", type=int, default=50, help="the size of image buffer that stores previously generated images")
        parser.add_argument("--no_html", action="store_true", help="do not save intermediate training results")
        parser.add_argument("--lr_policy", type=str, default="lambda", help="learning rate policy: lambda|step|plateau")
        parser.add_argument("--lr_decay_iters", type=int, default=50, help="multiply by a gamma every lr_decay_iters iterations")
        # build extension (not a reference flag): the structural term of backward_G
        # (DSGAN/models/pix2pix_model.py:193-195 uses single-scale ssim; BASELINE config 4 names the
        # gaussian-pyramid MS-SSIM of DSGAN/MS_SSIM.py:153-225, which needs images > 160 px)
        parser.add_argument("--ssim_loss", type=str, default="ssim", choices=["ssim", "ms_ssim"],
                            help="structural loss term: ssim (reference) or ms_ssim (opt-in)")
        # build extension: a device-side inf/nan scan of each network's flat gradient before its Adam
        # step; a non-finite gradient skips that optimizer step (parameters and moments untouched)
        # instead of writing NaN into the weights.  -1 = on for --precision bf16 (fp16 always has it
        # through its loss scaler), off for the fp32 parity mode.
        parser.add_argument("--cuda_graph", type=int, default=-1, choices=[-1, 0, 1],
                            help="replay optimize_parameters as two captured HIP graphs around the ImagePool "
                                 "query (-1: on for one process with device-side loss scaling / guard)")
        parser.add_argument("--nonfinite_guard", type=int, default=-1, choices=[-1, 0, 1],
                            help="skip an optimizer step whose gradient has inf/nan (-1: on for bf16)")
        # build extension: an exponential moving average of the generator's weights, updated by the
        # generator's Adam kernel on every applied step (ema = decay * ema + (1 - decay) * weights);
        # saved as {epoch}_useSE_net_G_ema.pth beside the raw G, scored by evaluate.py --use_ema
        parser.add_argument("--ema_decay", type=float, default=0.0,
                            help="decay of the generator's weight average, in [0, 1) (0: off; e.g. 0.999)")
        # build extension: Differentiable Augmentation (Zhao et al., NeurIPS 2020) of every batch the
        # discriminator sees, real or fake, in one HIP pass that also forms the D input; the generator's
        # gradient flows back through the same transform.  The remedy for a D that memorises a small set.
        parser.add_argument("--diffaug", type=_diffaug_policy, default="",
                            help="augment the discriminator's input: a comma-separated subset of "
                                 "color,translation,cutout (empty: off)")
        # build extension: the SN-PatchGAN (Miyato et al., ICLR 2018).  Every conv of the discriminator is
        # spectrally normalised (one power iteration per D weight version, on HIP kernels), the norm layers
        # leave (they would cancel the rescaling) and LeakyReLU moves into the conv epilogue.  It bounds how
        # sharp the discriminator can get; --diffaug is the remedy for one that memorises.
        parser.add_argument("--spectral_norm", action="store_true",
                            help="spectrally normalised discriminator without norm layers (SN-PatchGAN), any "
                                 "--which_model_netD; --norm then only steers the generator")
        self.isTrain = True
        return parser


def _diffaug_policy(s):
    """--diffaug's value in its canonical spelling; an unknown or repeated name is a ValueError naming it
    (argparse reports it as a usage error)."""
    from dsgan_hip.diffaug import policy_string
    return policy_string(s)


def default_train_opt(args=None, **overrides):
    """Programmatic TrainOptions (no argv, no opt.txt written): the reference defaults plus
    ``overrides``.  Used by bench.py, __graft_entry__.smoke() and the tests."""
    import os
    o = TrainOptions()
    opt = o.gather_options(list(args or []))
    opt.isTrain = True
    opt.gpu_ids = [int(s) for s in str(opt.gpu_ids).split(",") if int(s) >= 0]
    if "LOCAL_RANK" in os.environ and opt.gpu_ids:
        opt.gpu_ids = [int(os.environ["LOCAL_RANK"])]
    opt.checkpoints_dir = os.path.join(os.environ.get("TMPDIR", "/tmp"), "dsgan_checkpoints")
    for k, v in overrides.items():
        setattr(opt, k, v)
    opt.diffaug = _diffaug_policy(opt.diffaug)
    return opt
