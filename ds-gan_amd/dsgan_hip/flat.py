"""Flat parameter / gradient buffers and the fused Adam that updates them.

All parameters of one network live in ONE contiguous fp32 device buffer (each ``Parameter`` is
a view into it), and all their gradients in a second one.  That gives:
  * one Adam launch per network per step (``dsgan_adam``),
  * one zeroing launch per network per step,
  * a flat gradient to all-reduce across ranks in a few large RCCL buckets
    (one process per GPU; see ``dsgan_hip.dist``).
State-dict keys and shapes are untouched, so reference checkpoints load unchanged.
"""
import torch

from ._lib import call, ptr, stream
from .functional import fill_, bump_weight_generation


class FlatParams:
    """``order`` (optional): the modules whose parameters come first in the buffer, in that order
    (the rest follow in ``module.parameters()`` order).  The generator passes its backward order
    so that the gradient buckets of dsgan_hip.dist.GradBuckets fill front to back."""

    def __init__(self, module, device, order=None):
        self.params = [p for p in module.parameters()]
        placed = []
        if order:
            seen = set()
            for m in order:
                for p in m.parameters():
                    if id(p) not in seen:
                        seen.add(id(p))
                        placed.append(p)
            placed += [p for p in self.params if id(p) not in seen]
        else:
            placed = list(self.params)
        assert len(placed) == len(self.params)
        # every tensor starts on a 256-byte boundary (vector loads in the kernels)
        offs, n = {}, 0
        self.layout = []
        for p in placed:
            offs[id(p)] = n
            self.layout.append((p, n, p.numel()))
            n += (p.numel() + 63) // 64 * 64
        offs = [offs[id(p)] for p in self.params]
        self.numel = n
        self.data = torch.empty(n, device=device, dtype=torch.float32)
        self.grad = torch.empty(n, device=device, dtype=torch.float32)
        fill_(self.data, 0.0)
        with torch.no_grad():
            for p, off in zip(self.params, offs):
                k = p.numel()
                self.data[off:off + k].copy_(p.detach().reshape(-1).to(device=device, dtype=torch.float32))
                p.data = self.data[off:off + k].view(p.shape)
                p.grad = self.grad[off:off + k].view(p.shape)
        self.zero_grad()

    def zero_grad(self):
        fill_(self.grad, 0.0)


# ---- the moments in torch.optim.Adam's state-dict format (pure functions over CPU tensors) ----
# what torch.optim.Adam's own param_groups carry beside lr / betas / eps: written so that the
# reference's torch.optim.Adam(net.parameters(), ...) takes the file with its own load_state_dict
_TORCH_ADAM_GROUP = dict(weight_decay=0, amsgrad=False, maximize=False, foreach=None, capturable=False,
                         differentiable=False, fused=None)


def adam_state_to_torch(m, v, slots, step, group):
    """torch.optim.Adam's ``state_dict()`` from the flat moments.  ``m`` / ``v``: flat fp32 CPU tensors;
    ``slots``: one (offset, shape) per parameter in ``module.parameters()`` order (the state index);
    ``step``: the applied steps, one number for every parameter (a python scalar tensor each, as torch
    keeps it); ``group``: the param group (lr, betas, eps; ``params`` is replaced by the indices)."""
    state = {}
    for i, (off, shape) in enumerate(slots):
        k = int(torch.Size(shape).numel())
        state[i] = {"step": torch.tensor(float(step), dtype=torch.float32),
                    "exp_avg": m[off:off + k].view(shape).clone(),
                    "exp_avg_sq": v[off:off + k].view(shape).clone()}
    g = dict(_TORCH_ADAM_GROUP)
    g.update({k: (list(x) if isinstance(x, tuple) else x) for k, x in group.items() if k != "params"})
    g["params"] = list(range(len(slots)))
    return {"state": state, "param_groups": [g]}


def adam_state_from_torch(sd, slots, numel, group, names=None):
    """(m, v, step) from a torch.optim.Adam ``state_dict()``: flat fp32 CPU tensors of ``numel`` elements
    (zero outside the slots, as the kernel leaves the padding) and the one common step.  Raises, with the
    parameters' ``names`` (else their indices), on a missing entry, a shape mismatch, differing steps, or
    betas / eps other than ``group``'s.  With names on both sides (``sd['param_names']``) entries pair up
    by name; else by index.  An empty ``state`` (an optimizer that never stepped) is step 0, zero moments."""
    named = names is not None
    names = list(names) if named else [str(i) for i in range(len(slots))]
    groups = sd["param_groups"]
    if len(groups) != 1 or len(groups[0]["params"]) != len(slots):
        raise ValueError("optimizer state: %d param group(s) over %s parameters, this optimizer has one group of %d"
                         % (len(groups), [len(g["params"]) for g in groups], len(slots)))
    for key in ("betas", "eps"):
        a, b = groups[0][key], group[key]
        if (tuple(float(x) for x in a) != tuple(float(x) for x in b)) if key == "betas" else float(a) != float(b):
            raise ValueError("optimizer state: %s %r in the file, %r in this run" % (key, a, b))
    index = list(groups[0]["params"])
    saved = sd.get("param_names")
    if named and saved is not None:
        if sorted(saved) != sorted(names):
            raise ValueError("optimizer state: parameter names differ: only in the file %s, only in this run %s"
                             % (sorted(set(saved) - set(names)), sorted(set(names) - set(saved))))
        index = [index[list(saved).index(n)] for n in names]
    state = sd["state"]
    m, v = torch.zeros(numel, dtype=torch.float32), torch.zeros(numel, dtype=torch.float32)
    if not state:
        return m, v, 0
    missing = [n for n, i in zip(names, index) if i not in state]
    if missing:
        raise ValueError("optimizer state: no entry for %s" % missing)
    steps = {n: float(state[i]["step"]) for n, i in zip(names, index)}
    if len(set(steps.values())) != 1:
        raise ValueError("optimizer state: the parameters' step counts differ (one flat update needs one): %s"
                         % sorted(set(steps.values())))
    step = next(iter(steps.values()))
    if step != int(step) or step < 0:
        raise ValueError("optimizer state: step %r is not a whole number" % step)
    bad = ["%s: %s %s in the file vs %s" % (n, key, tuple(state[i][key].shape), tuple(shape))
           for n, i, (_, shape) in zip(names, index, slots) for key in ("exp_avg", "exp_avg_sq")
           if tuple(state[i][key].shape) != tuple(shape)]
    if bad:
        raise ValueError("optimizer state: size mismatch for " + "; ".join(bad))
    for i, (off, shape) in zip(index, slots):
        k = int(torch.Size(shape).numel())
        m[off:off + k].copy_(state[i]["exp_avg"].detach().reshape(-1).to("cpu", torch.float32))
        v[off:off + k].copy_(state[i]["exp_avg_sq"].detach().reshape(-1).to("cpu", torch.float32))
    return m, v, int(step)


class FlatAdam(torch.optim.Optimizer):
    """torch.optim.Adam (amsgrad=False, weight_decay=0) over a FlatParams buffer in one kernel.

    Subclasses torch.optim.Optimizer so the reference's LambdaLR scheduler (get_scheduler,
    DSGAN/models/networks.py:33-46) drives ``param_groups[0]['lr']`` exactly as before.

    ``ema_decay`` > 0 (--ema_decay): ``self.ema`` is a second flat buffer, a copy of ``flat.data`` at
    construction, and the step's one kernel also moves it toward the updated parameters,
    ``ema.lerp_(p, 1 - ema_decay)`` (dsgan_adam_ema / dsgan_adam_amp_ema): decided on the device, so a
    step the scaler skips does not average and a graph replay averages.  0: no buffer, the plain
    entry points.
    """

    def __init__(self, flat, lr=2e-4, betas=(0.9, 0.999), eps=1e-8, scaler=None, ema_decay=0.0):
        super().__init__(flat.params, dict(lr=lr, betas=betas, eps=eps))
        self.flat = flat
        self.scaler = scaler   # dsgan_hip.amp.LossScaler (--precision fp16): unscale / skip on device
        self.m = torch.zeros_like(flat.data)
        self.v = torch.zeros_like(flat.data)
        self.step_count = 0
        self.ema_decay = float(ema_decay)
        if not 0.0 <= self.ema_decay < 1.0:
            raise ValueError("ema_decay must lie in [0, 1), got %r" % (ema_decay,))
        self.ema = flat.data.clone() if self.ema_decay > 0.0 else None

    def reset_ema(self):
        """The average restarts from the current parameters (after a checkpoint without an EMA file)."""
        if self.ema is not None:
            with torch.no_grad():
                self.ema.copy_(self.flat.data)

    def ema_views(self, module=None):
        """(parameter, its view into the EMA buffer) by the layout offsets: of ``module``'s parameters,
        or of every parameter of the buffer."""
        if self.ema is None:
            raise RuntimeError("FlatAdam.ema_views: no EMA buffer (ema_decay is 0)")
        offs = {id(p): (off, k) for p, off, k in self.flat.layout}
        for p in (module.parameters() if module is not None else self.flat.params):
            off, k = offs[id(p)]
            yield p, self.ema[off:off + k].view(p.shape)

    def zero_grad(self, set_to_none=False):
        self.flat.zero_grad()

    # ---- torch.optim.Adam's state-dict format (resumable training; synchronises) ----
    def _slots(self):
        offs = {id(p): off for p, off, _ in self.flat.layout}
        return [(offs[id(p)], tuple(p.shape)) for p in self.flat.params]

    def applied_steps(self):
        """The update count the bias corrections use: the scaler's device counter, else step_count."""
        return self.scaler.applied_steps() if self.scaler is not None else self.step_count

    def state_dict(self):
        """``torch.optim.Adam``'s: {'state': {i: {'step', 'exp_avg', 'exp_avg_sq'}}, 'param_groups': [...]},
        i over ``flat.params`` (``module.parameters()`` order), CPU tensors of the parameters' shapes; a
        ``torch.optim.Adam`` over the same parameters loads it.  The EMA buffer is not part of it (it is a
        checkpoint file of its own)."""
        return adam_state_to_torch(self.m.cpu(), self.v.cpu(), self._slots(), self.applied_steps(),
                                   self.param_groups[0])

    @torch.no_grad()
    def load_state_dict(self, state_dict, names=None):
        """From this class's or ``torch.optim.Adam``'s state dict, in place: ``m`` and ``v`` keep their
        device buffers (captured graphs hold the pointers) and the step goes back to the counter in use
        (the scaler's ``state[4]``, else ``step_count``).  ``lr`` is NOT restored: the scheduler built from
        ``--epoch_count`` owns it.  ``names``: the parameters' names, for the messages and to pair entries
        with a file that carries ``param_names``."""
        m, v, step = adam_state_from_torch(state_dict, self._slots(), self.flat.numel, self.param_groups[0], names)
        self.m.copy_(m)
        self.v.copy_(v)
        if self.scaler is not None:
            self.scaler.state[4:5].copy_(torch.tensor([float(step)]))
        else:
            self.step_count = step

    @torch.no_grad()
    def step(self, closure=None):
        self.step_count += 1
        g = self.param_groups[0]
        b1, b2 = g["betas"]
        if self.ema is not None:   # the same update, and the moving average in the same pass
            if self.scaler is not None:
                call("dsgan_adam_amp_ema", ptr(self.flat.data), ptr(self.flat.grad), ptr(self.m), ptr(self.v),
                     ptr(self.ema), self.flat.numel, float(g["lr"]), float(b1), float(b2), float(g["eps"]),
                     self.ema_decay, ptr(self.scaler.state), stream())
            else:
                call("dsgan_adam_ema", ptr(self.flat.data), ptr(self.flat.grad), ptr(self.m), ptr(self.v),
                     ptr(self.ema), self.flat.numel, float(g["lr"]), float(b1), float(b2), float(g["eps"]),
                     self.ema_decay, self.step_count, stream())
        elif self.scaler is not None:
            # the scaler's check() has run on this gradient: g / scale, skipped on overflow, its
            # own step count for the bias corrections (step_count here counts calls)
            call("dsgan_adam_amp", ptr(self.flat.data), ptr(self.flat.grad), ptr(self.m), ptr(self.v),
                 self.flat.numel, float(g["lr"]), float(b1), float(b2), float(g["eps"]), ptr(self.scaler.state),
                 stream())
        else:
            call("dsgan_adam", ptr(self.flat.data), ptr(self.flat.grad), ptr(self.m), ptr(self.v),
                 self.flat.numel, float(g["lr"]), float(b1), float(b2), float(g["eps"]),
                 self.step_count, stream())
        bump_weight_generation(self.flat.params)
        return None
