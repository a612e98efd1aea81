"""Training loop with the reference's semantics (DSGAN/train.py:47-185) on the MI355X build.

Same order of work per iteration: set_input -> optimize_parameters -> get_img_tir / get_img_gen
/ get_img_label -> SSIM + PSNR of image 0 (device-side, util/metrics.py) -> every
``output_freq`` iterations the loss line and ``result.csv``; per epoch ``each_epoch.csv``,
``save_networks(epoch)`` and ``update_learning_rate()``.  The seed is 20 (:48).  Image dumps
(cv2) and the visualizer/HTML are out of scope (SURVEY.md §8 out-of-scope list).

    python ds-gan_amd/train.py --dataroot DATA --out RESULTS [reference TrainOptions flags...]
    python -m torch.distributed.run --nproc-per-node 8 --master-addr 127.0.0.1 \
        ds-gan_amd/train.py --dataroot DATA --out RESULTS --batchSize 128 [...]

Multi-GPU replaces the reference's single-process nn.DataParallel (DSGAN/models/networks.py:
74-77) with one process per GPU: under torchrun (WORLD_SIZE > 1) every rank joins the RCCL
process group and drives cuda:LOCAL_RANK; ``--batchSize`` stays the GLOBAL batch, of which each
rank trains its DataParallel-style chunk (data/__init__.py); the printed / CSV losses are the
global-batch values (an all-reduce of the per-rank means at logging time); only rank 0 writes
checkpoints and CSV files, behind a barrier.

``--eval_freq N`` (default 0: off) with ``--eval_phase`` (default ``test_all/``): every N epochs rank 0
scores the generator in eval mode on that split (evaluate.py's pass) and appends
``[epoch, 'test', ssim_avg, psnr_avg]`` to ``each_epoch.csv`` after the ``train`` row; the pass leaves
the training run bit-identical (``eval_pass``).  With ``--ema_decay`` on, the same pass runs once more on
the averaged generator (``Pix2PixModel.ema_scope``) and appends ``[epoch, 'test_ema', ssim_avg, psnr_avg]``
after the ``test`` row; the checkpoint of each epoch then has its ``_net_G_ema`` file.

``--save_state 1`` (default 0): after each epoch's network files every rank also writes its training state
(``save_train_state``: Adam's moments and step, the scalers, the ImagePool, the dropout counters, the RNGs),
``--keep_states N`` (default 2) epochs of them are kept.  ``--resume`` (implies ``--save_state 1``) continues
after the newest epoch whose state and network files are complete -- ``--continue_train``, ``--which_epoch``
and ``--epoch_count`` are set from it -- or starts fresh when there is none, so one command line both starts
and continues a run; the continued run is bit-identical to an uninterrupted one (README, "Resumable
training").  ``--stop_after_epoch E`` leaves the loop once epoch E is saved, the schedule untouched.
"""
import argparse
import csv
import math
import os
import random
import re
import sys
import time

HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)

import numpy as np  # noqa: E402
import torch  # noqa: E402
import torch.distributed as dist  # noqa: E402


def setup_seed(seed):
    torch.manual_seed(seed)
    torch.cuda.manual_seed_all(seed)
    np.random.seed(seed)
    random.seed(seed)


def init_distributed():
    """(rank, world, local_rank); joins the RCCL process group when launched by torchrun."""
    world = int(os.environ.get("WORLD_SIZE", "1"))
    if world == 1:
        return 0, 1, None
    local = int(os.environ.get("LOCAL_RANK", "0"))
    torch.cuda.set_device(local)
    if not dist.is_initialized():
        dist.init_process_group("nccl", device_id=torch.device("cuda", local))
    return dist.get_rank(), world, local


def global_losses(losses, n_local, n_global):
    """Per-rank batch means -> the global-batch means the reference logs (weights n_rank/n)."""
    if not (dist.is_available() and dist.is_initialized()) or dist.get_world_size() == 1:
        return losses
    dev = torch.device("cuda", torch.cuda.current_device())
    t = torch.tensor([v * n_local / n_global for v in losses.values()], dtype=torch.float64, device=dev)
    dist.all_reduce(t)
    return type(losses)(zip(losses.keys(), t.tolist()))


class NonfiniteMonitor:
    """Reports the optimizer steps that the bf16 non-finite guard or the fp16 loss scaler skipped
    (``Pix2PixModel.nonfinite_report``), so that a network that stops learning shows in the log.

    ``poll()`` runs at logging time.  It returns the text appended to the loss line: empty while no
    step was ever skipped, else the running counts, e.g. ``skipped G 3/400 D 0/400``.  When every
    step of one network since the previous poll was skipped, and there were at least
    ``abort_window`` of them, the network is no longer training: ``poll()`` raises RuntimeError."""

    def __init__(self, model, abort_window=50):
        self.model = model
        self.abort_window = int(abort_window)
        self.last = {}

    def poll(self):
        rep = self.model.nonfinite_report() if hasattr(self.model, "nonfinite_report") else {}
        dead = []
        for net, (skipped, calls) in rep.items():
            s0, c0 = self.last.get(net, (0, 0))
            if calls - c0 >= self.abort_window and skipped - s0 == calls - c0:
                dead.append("%s skipped all of its last %d optimizer steps" % (net, calls - c0))
        self.last = dict(rep)
        if dead:
            raise RuntimeError("non-finite gradients: " + "; ".join(dead) + " (--nonfinite_guard)")
        if not any(s for s, _ in rep.values()):
            return ""
        return "skipped " + " ".join("%s %d/%d" % (k, s, c) for k, (s, c) in rep.items()) + " "


def eval_pass(model, opt, phase):
    """(ssim_avg, psnr_avg) of the generator in eval mode over ``phase`` (evaluate.run_pass: batches in
    order, no flip, no_grad; every module's ``training`` flag restored).  The pass leaves training as it
    was: the loader's worker seed comes from the torch CPU generator and the dataset draws its crop
    offsets from python ``random`` (which the ImagePool also uses), so both states are put back."""
    from data import CreateDataLoader
    from evaluate import eval_options, run_pass
    from util.metrics import EvalMetrics
    py_state, cpu_state = random.getstate(), torch.get_rng_state()
    try:
        dataset = CreateDataLoader(eval_options(opt, phase), "test", local=True).load_data()
        metrics = EvalMetrics(model.device, max(len(dataset), 1))
        run_pass(model.netG, dataset, opt.which_direction == "AtoB", len(dataset), metrics)
        means = metrics.means()
    finally:
        random.setstate(py_state)
        torch.set_rng_state(cpu_state)
    return means[0], means[1]


_STATE_RE = re.compile(r"^(\d+)_train_state(?:_rank(\d+))?\.pth$")


def find_resume_epoch(names, world=1, ema=False):
    """The newest epoch that can be resumed, or None: a pure function of the checkpoint directory's
    listing ``names``.  An epoch counts when its state file(s) -- rank 0's, and under ``world`` ranks every
    rank's -- and its network files (G and D, either naming load_networks reads; with ``ema`` the averaged
    generator's too) are all there.  Temporary files of an interrupted save (another suffix) never match."""
    names = set(names)
    epochs = sorted((int(m.group(1)) for m in map(_STATE_RE.match, names) if m and m.group(2) is None), reverse=True)
    nets = ["G", "D"] + (["G_ema"] if ema else [])
    for e in epochs:
        ranks = all("%d_train_state_rank%d.pth" % (e, r) in names for r in range(1, world))
        files = all("%d_net_%s.pth" % (e, n) in names or "%d_useSE_net_%s.pth" % (e, n) in names for n in nets)
        if ranks and files and "%d_train_state.pth" % e in names:
            return e
    return None


def states_to_prune(names, keep):
    """The state files (every rank's; nothing else) of all but the ``keep`` newest epochs that have any."""
    found = [(int(m.group(1)), n) for n, m in ((n, _STATE_RE.match(n)) for n in names) if m]
    kept = set(sorted({e for e, _ in found}, reverse=True)[:max(int(keep), 0)])
    return sorted(n for e, n in found if e not in kept)


def main(argv=None, output_freq=100):
    from data import CreateDataLoader
    from models import create_model
    from options.train_options import TrainOptions
    from util.metrics import TrainMetrics

    ap = argparse.ArgumentParser(add_help=False)
    ap.add_argument("--out", default=os.path.abspath(os.path.join("..", "resext50_vision1")))
    ap.add_argument("--dataroot", default="/root/dataset/256x256")
    ap.add_argument("--eval_freq", type=int, default=0,
                    help="every N epochs rank 0 scores the generator on --eval_phase (0: never)")
    ap.add_argument("--eval_phase", default="test_all/", help="the split of the per-epoch test pass")
    ap.add_argument("--save_state", type=int, default=0, choices=[0, 1],
                    help="1: after each epoch's save_networks also save_train_state (optimizers, scalers, pool, RNGs)")
    ap.add_argument("--keep_states", type=int, default=2, help="state files of this many newest epochs are kept")
    ap.add_argument("--stop_after_epoch", type=int, default=0,
                    help="leave the epoch loop once this epoch is saved (0: off; the schedule is untouched)")
    ap.add_argument("--resume", action="store_true",
                    help="continue from the newest epoch with a complete state (else start fresh); implies --save_state 1")
    known, rest = ap.parse_known_args(argv)
    save_state = bool(known.save_state) or known.resume
    rank, world, local = init_distributed()
    setup_seed(20)
    out = known.out
    if rank == 0:
        os.makedirs(out, exist_ok=True)
    opt = TrainOptions().parse(known.dataroot, out, rest)   # parse() sets checkpoints_dir = out/checkpoints
    if world > 1:
        opt.gpu_ids = [local]   # one process per GPU: this rank's device
    resumed = None
    if known.resume:
        ckpt_dir = os.path.join(opt.checkpoints_dir, opt.name)
        resumed = find_resume_epoch(os.listdir(ckpt_dir) if os.path.isdir(ckpt_dir) else [], world,
                                    float(getattr(opt, "ema_decay", 0.0) or 0.0) > 0.0)
        if resumed is None:
            print("--resume: no complete training state in %s, starting fresh" % ckpt_dir)
        else:
            print("--resume: continuing after epoch %d" % resumed)
            opt.continue_train, opt.which_epoch, opt.epoch_count = True, str(resumed), resumed + 1
    dataset = CreateDataLoader(opt, "train").load_data()
    print("#training images = %d" % len(dataset))
    model = create_model(opt)
    model.setup(opt)
    if resumed is not None:   # after the weights (and the EMA) of that epoch: their fingerprints are checked
        model.load_train_state(resumed)
    metrics = TrainMetrics(model.device)
    guard = NonfiniteMonitor(model)
    history = []
    for epoch in range(opt.epoch_count, opt.niter + opt.niter_decay + 1):
        metrics.reset()
        epoch_start_time = time.time()
        epoch_iter, i = 0, -1
        for i, data in enumerate(dataset):
            iter_start_time = time.time()
            epoch_iter += opt.batchSize
            model.set_input(data)
            model.optimize_parameters()
            model.get_img_tir(data)
            with torch.no_grad():   # the reference runs this forward with autograd on; output is identical
                model.get_img_gen(data)
            model.get_img_label(data)
            # the reference scores image 0 of the GLOBAL batch only (DSGAN/train.py:110-124); under
            # DDP that image is rank 0's fake_B[0] (Tensor.chunk order), so rank 0's accumulators
            # are exactly the reference's metric and no cross-rank reduction is needed
            metrics.update(model.fake_B[0], model.real_B[0])
            if (i + 1) % output_freq == 0:
                losses = global_losses(model.get_current_losses(), int(model.real_A.shape[0]),
                                       int(data.get("global_batch", model.real_A.shape[0])))
                skipped = guard.poll()   # every rank: a network that stopped learning ends every rank
                if rank != 0:
                    continue
                ssim_avg, psnr_avg = metrics.averages()
                t = (time.time() - iter_start_time) / opt.batchSize
                message = "(epoch: %d, iters: %d, time: %.3f) " % (epoch, epoch_iter, t)
                message += "".join("%s: %.3f " % (k, v) for k, v in losses.items())
                print(message + "ssim: %.4f psnr: %.3f" % (ssim_avg, psnr_avg) + (" " + skipped if skipped else ""))
                with open(os.path.join(out, "result.csv"), "a", newline="") as f:
                    csv.writer(f).writerow([epoch, "".join("%s: %.3f " % (k, v) for k, v in losses.items()) + "  ",
                                            ssim_avg, psnr_avg])
        ssim_avg, psnr_avg = metrics.averages()
        history.append((epoch, ssim_avg, psnr_avg))
        if rank == 0:
            with open(os.path.join(out, "each_epoch.csv"), "a", newline="") as f:
                csv.writer(f).writerow([epoch, "train", ssim_avg, psnr_avg])
            if known.eval_freq > 0 and epoch % known.eval_freq == 0:   # the other ranks wait at the barrier below
                t_ssim, t_psnr = eval_pass(model, opt, known.eval_phase)
                print("test (%s) ssim: %.4f psnr: %.3f" % (known.eval_phase, t_ssim, t_psnr))
                with open(os.path.join(out, "each_epoch.csv"), "a", newline="") as f:
                    csv.writer(f).writerow([epoch, "test", t_ssim, t_psnr])
                if getattr(model, "ema_on", False):   # the averaged generator, on the same split
                    with model.ema_scope():
                        e_ssim, e_psnr = eval_pass(model, opt, known.eval_phase)
                    print("test_ema (%s) ssim: %.4f psnr: %.3f" % (known.eval_phase, e_ssim, e_psnr))
                    with open(os.path.join(out, "each_epoch.csv"), "a", newline="") as f:
                        csv.writer(f).writerow([epoch, "test_ema", e_ssim, e_psnr])
            print("saving the model at the end of epoch %d, iters %d" % (epoch, i + 1))
            model.save_networks(epoch)
            print("End of epoch %d / %d \t Time Taken: %d sec" % (epoch, opt.niter + opt.niter_decay,
                                                                    time.time() - epoch_start_time))
        if world > 1:
            dist.barrier()
        if save_state:   # every rank (its own file; the ranks' fingerprints are compared), after the network files
            model.save_train_state(epoch)
            if rank == 0:
                for name in states_to_prune(os.listdir(model.save_dir), known.keep_states):
                    os.remove(os.path.join(model.save_dir, name))
        model.update_learning_rate()
        if known.stop_after_epoch > 0 and epoch >= known.stop_after_epoch:
            break
    return model, history


if __name__ == "__main__":
    main()
