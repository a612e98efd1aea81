"""BaseModel lifecycle (DSGAN/models/base_model.py:7-177) for the MI355X build.

Same public methods and semantics: initialize / setup / eval / test / set_input /
optimize_parameters / update_learning_rate / get_current_visuals / get_current_losses /
save_networks / load_networks / print_networks / set_requires_grad.  Device selection follows
``opt.gpu_ids`` as in the reference; with one process per GPU each rank owns ``cuda:LOCAL_RANK``.
"""
import os
from collections import OrderedDict

import torch

from dsgan_hip import spectral as hspectral
from . import networks


def atomic_save(obj, path):
    """torch.save under a temporary name in the same directory, then os.replace: a reader sees the old
    file or the whole new one, never a part."""
    tmp = "%s.tmp%d" % (path, os.getpid())
    try:
        torch.save(obj, tmp)
        os.replace(tmp, path)
    finally:
        if os.path.exists(tmp):
            os.remove(tmp)


def rng_state_dict(device=None):
    """The python ``random``, numpy, torch-CPU and (``device`` given) torch-device generator states as
    tensors and plain lists, so that the file loads with ``torch.load(weights_only=True)``."""
    import random
    import numpy as np
    ver, words, gauss = random.getstate()
    kind, keys, pos, has_gauss, cached = np.random.get_state()
    out = {"python": [ver, list(words), gauss],
           "numpy": {"kind": str(kind), "keys": torch.from_numpy(keys.astype(np.int64)), "pos": int(pos),
                     "has_gauss": int(has_gauss), "cached_gaussian": float(cached)},
           "torch_cpu": torch.get_rng_state().clone()}
    if device is not None and torch.device(device).type == "cuda":
        out["torch_device"] = torch.cuda.get_rng_state(device).clone()
    return out


def load_rng_state_dict(sd, device=None):
    import random
    import numpy as np
    ver, words, gauss = sd["python"]
    random.setstate((ver, tuple(words), gauss))
    n = sd["numpy"]
    np.random.set_state((n["kind"], n["keys"].numpy().astype(np.uint32), n["pos"], n["has_gauss"], n["cached_gaussian"]))
    torch.set_rng_state(sd["torch_cpu"].to("cpu", torch.uint8))
    if device is not None and "torch_device" in sd and torch.device(device).type == "cuda":
        torch.cuda.set_rng_state(sd["torch_device"].to("cpu", torch.uint8), device)


def train_state_filename(which_epoch, rank=0):
    """Rank 0's file holds the whole state; rank r > 0 adds what is its own (pool, RNGs, dropout counters)."""
    return "%s_train_state.pth" % which_epoch if rank == 0 else "%s_train_state_rank%d.pth" % (which_epoch, rank)


class BaseModel:
    @staticmethod
    def modify_commandline_options(parser, is_train):
        return parser

    def name(self):
        return "BaseModel"

    def initialize(self, opt):
        self.opt = opt
        self.gpu_ids = opt.gpu_ids
        self.isTrain = opt.isTrain
        self.device = torch.device("cuda:{}".format(self.gpu_ids[0])) if self.gpu_ids else torch.device("cpu")
        self.save_dir = os.path.join(opt.checkpoints_dir, opt.name)
        self.loss_names = []
        self.model_names = []
        self.visual_names = []
        self.image_paths = []

    ema_on = False     # a model that keeps a moving average of its generator (--ema_decay) says so
    load_suffix = ""   # "_ema": load_networks reads the averaged generator's files (evaluate.py --use_ema)

    def set_input(self, input):
        self.input = input

    def forward(self):
        pass

    def setup(self, opt, parser=None):
        if self.isTrain:
            self.schedulers = [networks.get_scheduler(optimizer, opt) for optimizer in self.optimizers]
        if not self.isTrain or opt.continue_train:
            self.load_networks(opt.which_epoch)
            if self.isTrain and self.ema_on:   # after G: a missing EMA file restarts it from the loaded weights
                self.load_ema(opt.which_epoch)
        self.print_networks(opt.verbose)

    def eval(self):
        for name in self.model_names:
            if isinstance(name, str):
                getattr(self, "net" + name).eval()

    def test(self):
        with torch.no_grad():
            self.forward()

    def get_image_paths(self):
        return self.image_paths

    def optimize_parameters(self):
        pass

    def update_learning_rate(self):
        for scheduler in self.schedulers:
            scheduler.step()
        lr = self.optimizers[0].param_groups[0]["lr"]
        print("learning rate = %.7f" % lr)

    def get_current_visuals(self):
        visual_ret = OrderedDict()
        for name in self.visual_names:
            if isinstance(name, str):
                visual_ret[name] = getattr(self, name)
        return visual_ret

    def get_current_losses(self):
        errors_ret = OrderedDict()
        for name in self.loss_names:
            if isinstance(name, str):
                v = getattr(self, "loss_" + name)
                errors_ret[name] = float(v.detach() if torch.is_tensor(v) else v)
        return errors_ret

    def save_networks(self, which_epoch):
        """'{epoch}_useSE_net_{G,D}.pth' as the reference writes (:95).  Keys carry no
        ``module.`` prefix (no DataParallel wrapper); load_networks accepts both.  With --ema_decay
        on, '{epoch}_useSE_net_G_ema.pth' as well: the averaged generator, G's keys and shapes."""
        os.makedirs(self.save_dir, exist_ok=True)
        for name in self.model_names:
            if isinstance(name, str):
                save_filename = "%s_useSE_net_%s.pth" % (which_epoch, name)
                net = getattr(self, "net" + name)
                sd = OrderedDict((k, v.detach().cpu().clone()) for k, v in net.state_dict().items())
                torch.save(sd, os.path.join(self.save_dir, save_filename))
        if self.ema_on:
            with self.ema_scope():
                sd = OrderedDict((k, v.detach().cpu().clone()) for k, v in self.netG.state_dict().items())
            torch.save(sd, os.path.join(self.save_dir, "%s_useSE_net_G_ema.pth" % which_epoch))

    def load_networks(self, which_epoch):
        """Reads '{epoch}_net_{name}.pth' like the reference (:119) and, if that is absent, the
        '{epoch}_useSE_net_{name}.pth' this build (and the reference) saves -- the reference's
        save/load name mismatch is bridged instead of failing.  (``load_suffix`` "_ema": the same two
        names with ``_ema`` before the extension.)  ``module.`` prefixes from
        DataParallel checkpoints are stripped.  As the reference's ``load_state_dict(strict=False)``
        (:148): missing / unexpected keys are allowed (and printed), a shape mismatch raises."""
        for name in self.model_names:
            if isinstance(name, str):
                net = getattr(self, "net" + name)
                cands = ["%s_net_%s%s.pth" % (which_epoch, name, self.load_suffix),
                         "%s_useSE_net_%s%s.pth" % (which_epoch, name, self.load_suffix)]
                paths = [os.path.join(self.save_dir, c) for c in cands]
                path = next((p for p in paths if os.path.exists(p)), paths[0])
                print("loading the model from %s" % path)
                state_dict = torch.load(path, map_location="cpu", weights_only=True)
                state_dict = OrderedDict((k[7:] if k.startswith("module.") else k, v) for k, v in state_dict.items())
                own = net.state_dict()
                # a plain D file offered to a --spectral_norm run, or the reverse: refused, naming the keys
                hspectral.check_state_keys(own.keys(), state_dict.keys(), "net%s" % name)
                # the reference's pre-0.4 InstanceNorm patch (:108-109): running statistics saved for a
                # layer that tracks none are dropped; a BatchNorm's own buffers load like any key
                state_dict = {k: v for k, v in state_dict.items()
                              if k in own or not (k.endswith("running_mean") or k.endswith("running_var"))}
                bad = ["%s: checkpoint %s vs model %s" % (k, tuple(v.shape), tuple(own[k].shape))
                       for k, v in state_dict.items() if k in own and own[k].shape != v.shape]
                if bad:
                    raise RuntimeError("Error(s) in loading state_dict for %s:\n\tsize mismatch for %s"
                                       % (type(net).__name__, "\n\tsize mismatch for ".join(bad)))
                missing = [k for k in own if k not in state_dict]
                unexpected = [k for k in state_dict if k not in own]
                if missing or unexpected:
                    print("load_networks(%s): missing keys %s, unexpected keys %s" % (name, missing, unexpected))
                with torch.no_grad():
                    for k, v in state_dict.items():
                        if k in own:
                            own[k].copy_(v.to(own[k].device, own[k].dtype))
                if getattr(net, "spectral", None) is not None:   # W_sn and sigma of the loaded (W, u, v)
                    net.spectral.refresh(iterate=False)

    # ---- resumable training: everything beside the weights (--save_state / --resume) ----
    RANK_STATE_KEYS = ("version", "epoch", "world_size", "precision", "pool", "dropout", "rng", "diffaug")

    def train_state_dict(self):
        """What a model needs beside its network files to continue bit for bit (Pix2PixModel)."""
        raise NotImplementedError("%s keeps no resumable training state" % self.name())

    def load_train_state_dict(self, sd, own):
        raise NotImplementedError("%s keeps no resumable training state" % self.name())

    def save_train_state(self, which_epoch):
        """'{epoch}_train_state.pth' in save_dir, written after the network files of that epoch and
        atomically (atomic_save), so that a job killed mid-save leaves the previous epoch resumable.
        Under ``torchrun`` EVERY rank calls this (train_state_dict compares the ranks' fingerprints with one
        collective): rank 0 writes the whole state, rank r > 0 '{epoch}_train_state_rank{r}.pth' with what is
        its own (RANK_STATE_KEYS)."""
        from dsgan_hip import dist as hdist
        sd = self.train_state_dict()
        sd["epoch"] = which_epoch
        r = hdist.rank()
        if r > 0:
            # ("diffaug" is there only with the flag on; every other key must be)
            sd = {k: sd[k] for k in self.RANK_STATE_KEYS if k != "diffaug" or k in sd}
        os.makedirs(self.save_dir, exist_ok=True)
        path = os.path.join(self.save_dir, train_state_filename(which_epoch, r))
        atomic_save(sd, path)
        return path

    def load_train_state(self, which_epoch):
        """After load_networks (and load_ema) of the same epoch: restores the state in place and checks the
        buffers' fingerprints against the file's.  Every rank reads rank 0's file and, r > 0, its own."""
        from dsgan_hip import dist as hdist
        path = os.path.join(self.save_dir, train_state_filename(which_epoch))
        print("loading the training state from %s" % path)
        sd = torch.load(path, map_location="cpu", weights_only=True)
        own = sd
        if hdist.rank() > 0:
            own = torch.load(os.path.join(self.save_dir, train_state_filename(which_epoch, hdist.rank())),
                             map_location="cpu", weights_only=True)
        self.load_train_state_dict(sd, own)

    def print_networks(self, verbose):
        print("---------- Networks initialized -------------")
        for name in self.model_names:
            if isinstance(name, str):
                net = getattr(self, "net" + name)
                num_params = sum(p.numel() for p in net.parameters())
                if verbose:
                    print(net)
                print("[Network %s] Total number of parameters : %.3f M" % (name, num_params / 1e6))
        print("-----------------------------------------------")

    def set_requires_grad(self, nets, requires_grad=False):
        if not isinstance(nets, list):
            nets = [nets]
        for net in nets:
            if net is not None:
                for param in net.parameters():
                    param.requires_grad = requires_grad
                # --spectral_norm: the convs read the W_sn leaves, which are no parameters; frozen with
                # the rest, they get no weight-grad launch in the G step
                for w in networks.spectral_weights(net):
                    w.requires_grad = requires_grad
