"""Optimisers on the flat parameter buffer: one HIP kernel per step for the whole network.

FusedAdam with its constructor arguments of old is torch.optim.Adam(lr) as built at managers/BaseManager.py:441 of the reference and
launches catseg_adam_step / catseg_adam_step_dev (include/catseg.h).  Weight decay (coupled or decoupled), amsgrad, parameter groups,
momentum SGD and clipping by the global gradient norm run on the kernels of include/catseg_optim.h.  WeightAverage keeps a
running average of the weights (EMA / SWA, torch.optim.swa_utils.AveragedModel's arithmetic) in a shadow of the flat buffer: one launch
of include/catseg_ema.h behind the update.  set_accumulation(n) makes n micro-steps one optimiser step: a window buffer beside the
gradient buffer, folded by catseg_axpy2d, read by the same kernels with the gradient scale divided by the micro-steps it holds."""
import contextlib

import numpy as np
import torch

from . import ops
from .engine import FlatParams

MAX_GROUPS = ops.OPTIM_MAX_GROUPS
# the row device_hyper() uploads: the CATSEG_OPTIM_HYPER_FLOATS entries the optimiser kernels read, then the weight of the running average
AVERAGE_SLOT = ops.OPTIM_HYPER_FLOATS
HYPER_ROW_FLOATS = ops.OPTIM_HYPER_FLOATS + 4


def chunk_group_map(offsets, sizes, groups, total, align=FlatParams.ALIGN):
    """uint8 [ceil(total / align)]: the parameter group of every `align`-float chunk of a flat buffer in which parameter i occupies
    [offsets[i], offsets[i] + sizes[i]) and the zero gap up to the next parameter's start (or `total`) belongs to it too.  Pure numpy."""
    offsets, sizes, groups = (np.asarray(a, dtype=np.int64) for a in (offsets, sizes, groups))
    if not (offsets.shape == sizes.shape == groups.shape) or offsets.ndim != 1 or offsets.size == 0:
        raise ValueError("chunk_group_map: offsets, sizes and groups are three lists of one length")
    if (offsets % align).any() or offsets[0] != 0 or (np.diff(offsets) <= 0).any():
        raise ValueError("chunk_group_map: every parameter starts on a %d-float boundary, the first at 0, in ascending order" % align)
    ends = np.append(offsets[1:], total)
    if (offsets + sizes > ends).any() or (sizes <= 0).any():
        raise ValueError("chunk_group_map: a parameter overlaps the next one (or the end of the buffer)")
    if groups.min() < 0 or groups.max() >= MAX_GROUPS:
        raise ValueError("chunk_group_map: groups are 0 .. %d" % (MAX_GROUPS - 1))
    chunks = (ends + align - 1) // align - offsets // align
    return np.repeat(groups.astype(np.uint8), chunks)


def _is_norm(module):
    return isinstance(module, (torch.nn.modules.batchnorm._NormBase, torch.nn.GroupNorm, torch.nn.LayerNorm))


def param_groups(model, weight_decay, no_decay=("norm", "bias"), lr_mult=None):
    """torch-style parameter groups for the fused optimisers (and the stock ones): [{'params': [...], 'weight_decay': ..., 'lr_mult': ...}].
    no_decay: 'norm' = the weights and biases of BatchNorm / GroupNorm / LayerNorm modules, 'bias' = every parameter named bias, any other
    entry = a substring of the parameter's dotted name; those parameters get weight_decay 0.
    lr_mult: {name prefix: factor}; a parameter whose dotted name starts with a prefix (the longest wins) trains at factor x the
    optimiser's lr (the optimiser turns 'lr_mult' into the group's 'lr').  Empty groups are left out; every parameter lands in one."""
    lr_mult = dict(lr_mult or {})
    no_decay = tuple(no_decay or ())
    owner_is_norm = {}
    for mname, mod in model.named_modules():
        for pname, p in mod.named_parameters(recurse=False):
            owner_is_norm[id(p)] = _is_norm(mod)
    keys, buckets = [], {}
    for mult_key in [None] + list(lr_mult):
        for decay in (True, False):
            keys.append((mult_key, decay))
            buckets[(mult_key, decay)] = []
    for name, p in model.named_parameters():
        plain = False
        for tok in no_decay:
            if tok == "norm":
                plain = plain or owner_is_norm.get(id(p), False)
            elif tok == "bias":
                plain = plain or name.split(".")[-1] == "bias"
            else:
                plain = plain or tok in name
        hit = [k for k in lr_mult if name.startswith(k)]
        mult_key = max(hit, key=len) if hit else None
        buckets[(mult_key, not plain)].append(p)
    out = []
    for mult_key, decay in keys:
        if buckets[(mult_key, decay)]:
            g = {"params": buckets[(mult_key, decay)], "weight_decay": float(weight_decay) if decay else 0.0}
            if mult_key is not None:
                g["lr_mult"] = float(lr_mult[mult_key])
            out.append(g)
    return out


class FusedOptimizer(torch.optim.Optimizer):
    """What the fused optimisers share: the flat state buffers (laid out like the parameters, conv weights OHWI), the step count, the
    parameter groups and their chunk map, the step scalars by value or in device memory (device_hyper(): a launch recorded into a
    hipGraph reads them there), the gradient scale and the gradient-norm clip.

    The first constructor argument is the model.  groups: None (one group of all parameters) or torch-style dicts
    {'params': [...], 'lr': ..., 'weight_decay': ...} ('lr_mult': f stands for 'lr': f x the optimiser's lr); they become
    self.param_groups, so LambdaLR scales each group's rate.  Only lr and weight_decay may differ between groups."""
    _STATE = ()            # ((attribute, state-dict key), ...) of the flat state buffers this optimiser may own
    _STOCK = None          # the stock optimiser whose state-dict format this one speaks

    def __init__(self, model, defaults, groups=None, grad_scale=1.0, max_grad_norm=None):
        self.model = model
        params = list(model.parameters())
        if groups is None:
            groups = params
        else:
            groups = [dict(g) for g in groups]
            if not 1 <= len(groups) <= MAX_GROUPS:
                raise ValueError("%s takes 1 to %d parameter groups, got %d" % (type(self).__name__, MAX_GROUPS, len(groups)))
            seen = {}
            for gi, g in enumerate(groups):
                g["params"] = list(g["params"])
                if "lr_mult" in g:
                    mult = g.pop("lr_mult")
                    g.setdefault("lr", defaults["lr"] * mult)
                for p in g["params"]:
                    if id(p) in seen:
                        raise ValueError("a parameter of shape %s is in parameter groups %d and %d" % (tuple(p.shape), seen[id(p)], gi))
                    seen[id(p)] = gi
                for k in g:
                    if k not in ("params", "lr", "weight_decay") and g[k] != defaults.get(k):
                        raise ValueError("parameter groups may differ in 'lr' and 'weight_decay' only, group %d sets %r" % (gi, k))
            ids = {id(p) for p in params}
            if set(seen) - ids:
                raise ValueError("a parameter group holds a tensor that is not a parameter of the model")
            missing = [tuple(p.shape) for p in params if id(p) not in seen]
            if missing:
                raise ValueError("%d parameters of the model are in no parameter group (first shape %s)" % (len(missing), missing[0]))
        super().__init__(groups, defaults)
        for a, _ in self._STATE:
            setattr(self, a, None)
        self._steps = 0
        self.grad_scale = grad_scale
        self.max_grad_norm = None if max_grad_norm is None else float(max_grad_norm)
        if self.max_grad_norm is not None and not self.max_grad_norm >= 0:
            raise ValueError("max_grad_norm must not be negative")
        self.last_grad_norm = None                     # DEVICE float32 [2] = {norm, clip factor} of the last step; nothing reads it back here
        self._norm_ws = None
        self._map = self._map_key = None
        self._hyper_dev = self._hyper_host = None      # device_hyper(): the step-dependent scalars live in device memory
        self._row = torch.zeros(ops.OPTIM_HYPER_FLOATS, dtype=torch.float32)
        self._avg = None                               # attach_average(): the running average updated behind every step
        self._accum, self._acc, self._folded = 1, None, 0      # set_accumulation(): the window, its flat sum, micro-steps folded so far

    def zero_grad(self, set_to_none=True):
        """The backward tape OVERWRITES each parameter's slice of the flat gradient buffer (it does not accumulate over
        several backward passes: a second backward() before zero_grad() raises); clearing the buffer here matters for
        parameters that receive no gradient in a step (one memset of the flat buffer, ~0.1 ms).  An accumulation window
        (set_accumulation) is not touched: fold() has the micro-step's gradients by then."""
        self.model.zero_grad()
        return None

    # ------------------------------------------------------------------ gradient accumulation
    def set_accumulation(self, n):
        """A window of n micro-steps per optimiser step: every micro-step runs zero_grad / forward / backward / fold(), step() follows
        once window_full() (or earlier, on a partial window of m < n micro-steps: the mean is then taken over m).

            acc = g_1 + g_2 + ... + g_m (fp32, in micro-batch order: one catseg_axpy2d launch per fold over the flat buffer)
            g'  = (acc * grad_scale / m) * clip,    clip = min(1, max_grad_norm / (||acc * grad_scale / m|| + 1e-6))

        and g' is what the update kernels take for the gradient: they read `acc` where they read the gradient buffer and
        grad_scale / m where they read the gradient scale (by value, or from the device row), so no kernel is added.  The stock form
        (loss / n).backward() scales every term before adding; the two differ in rounding only and are identical when n is a power of two.
        BatchNorm takes its statistics and updates its running statistics per micro-batch, as torch does.  Step count, bias corrections,
        LambdaLR and an attached running average follow optimiser steps, not micro-steps.  The window is not part of state_dict():
        checkpoints are written where it is empty.  n = 1 (the default): nothing is allocated, fold() launches nothing, step() is the
        step without a window."""
        if isinstance(n, bool) or not isinstance(n, int) or n < 1:
            raise ValueError("set_accumulation: the window is an int >= 1, got %r" % (n,))
        if n != self._accum and self._folded:
            raise RuntimeError("set_accumulation: %d micro-steps are folded into the open window; step() first" % self._folded)
        self._accum = n
        if n == 1:
            self._acc = None
        return self

    def _carried(self, cur, fp):
        """`cur` if it is a buffer laid out like fp.flat on its device, else a new zero one (with cur's values if the model only moved)"""
        if cur is None or cur.numel() != fp.flat.numel() or cur.device != fp.flat.device:
            new = torch.zeros_like(fp.flat)
            if cur is not None and cur.numel() == fp.flat.numel():
                new.copy_(cur)
            return new
        return cur

    def _window(self, fp):
        """the flat sum of the window's gradients (allocated zero on first use; carried along when the model moved)"""
        self._acc = self._carried(self._acc, fp)
        return self._acc

    def _capturing(self, fp):
        return fp.flat.is_cuda and torch.cuda.is_current_stream_capturing()

    def fold(self):
        """behind every backward pass: acc += grad (one launch over the whole flat buffer; the gradient buffer is left as it is).  Inside
        a stream capture the launch is recorded and nothing is counted: the replay's caller counts (graph.GraphedTrainStep)."""
        if self._accum == 1:
            return
        fp = self.model.flat()
        acc = self._window(fp)
        n = fp.grad.numel()
        assert n % FlatParams.ALIGN == 0 and acc.numel() == n, "the flat buffers are a multiple of %d floats" % FlatParams.ALIGN
        ops.axpy(fp.grad.view(n // FlatParams.ALIGN, FlatParams.ALIGN), acc.view(n // FlatParams.ALIGN, FlatParams.ALIGN), 1.0, accumulate=True)
        if not self._capturing(fp):
            self._folded += 1

    def window_full(self):
        return self._folded >= self._accum

    def _scale(self):
        """the gradient scale of the step about to be launched: grad_scale, over the micro-steps folded into the window"""
        return self.grad_scale if self._accum == 1 else self.grad_scale / max(self._folded, 1)

    def _grad(self, fp):
        """what step() reads for the gradient: the gradient buffer, or the window's sum (which must hold a micro-step; a capture
        records the launches of a step whose count the replay's caller keeps)"""
        if self._accum == 1:
            return fp.grad
        if self._folded < 1 and not self._capturing(fp):
            raise RuntimeError("step() on an empty accumulation window: fold() a backward pass first")
        return self._window(fp)

    def _close_window(self, fp):
        """behind the update and the running average: the window starts over"""
        if self._accum > 1:
            self._acc.zero_()
            if not self._capturing(fp):
                self._folded = 0

    # ------------------------------------------------------------------ state
    def _live(self):
        """the attributes of the state buffers the current options need"""
        return [a for a, _ in self._STATE]

    def _state(self, fp):
        """the flat state buffers (allocated zero on first use; carried along when the model moved), in _live() order"""
        out = []
        for a in self._live():
            setattr(self, a, self._carried(getattr(self, a), fp))
            out.append(getattr(self, a))
        if self.max_grad_norm is not None and (self.last_grad_norm is None or self.last_grad_norm.device != fp.flat.device):
            self.last_grad_norm = torch.zeros(2, dtype=torch.float32, device=fp.flat.device)
            self._norm_ws = torch.zeros(max(ops.grad_norm_workspace(fp.flat.numel()), 8), dtype=torch.uint8, device=fp.flat.device)
        return out

    def state_buffers(self):
        """every flat state tensor of this optimiser (what a snapshot of the training state has to hold besides `_steps`)"""
        fp = self.model.flat()
        own = self._state(fp)
        if self._accum > 1:
            own = own + [self._window(fp)]
        return own if self._avg is None else own + self._avg.buffers()

    def attach_average(self, avg):
        """avg: a WeightAverage over this optimiser's model (None detaches).  Every step() launches its update behind the parameter
        update, on the same stream; its shadows join state_buffers(); its update count follows this optimiser's step count."""
        if avg is not None:
            if not isinstance(avg, WeightAverage) or avg.model is not self.model:
                raise ValueError("attach_average takes a WeightAverage over the optimiser's own model")
            avg._attach(self)
        elif self._avg is not None:
            self._avg.optimiser = None
        self._avg = avg
        return avg

    def _average(self):
        if self._avg is not None:
            self._avg.update()

    def _group_map(self, fp):
        """DEVICE uint8 per 64-float chunk, or None with one group"""
        if len(self.param_groups) == 1:
            return None
        key = (id(fp.flat), fp.flat.device)
        if self._map is None or self._map_key != key:
            group_of = {id(p): gi for gi, g in enumerate(self.param_groups) for p in g["params"]}
            m = chunk_group_map([fp.offsets[id(p)] for p in fp.params], [p.numel() for p in fp.params], [group_of[id(p)] for p in fp.params],
                                fp.flat.numel())
            self._map, self._map_key = torch.from_numpy(m).to(fp.flat.device), key
        return self._map

    # ------------------------------------------------------------------ step scalars
    def _fill_hyper(self, row):
        """the step scalars of the CURRENT step count into a host float32 row"""
        raise NotImplementedError

    def device_hyper(self):
        """switch to the device-scalar kernel form (catseg_adam_step_dev, the hyper_dev form of catseg_optim.h); bit-identical updates"""
        if self._hyper_dev is None:
            fp = self.model.flat()
            n = HYPER_ROW_FLOATS
            self._hyper_host = torch.zeros((16, n), dtype=torch.float32).pin_memory()     # a ring: the host may run steps ahead of the GPU
            self._hyper_events = [None] * 16
            self._hyper_dev = torch.zeros(n, dtype=torch.float32, device=fp.flat.device)
        return self

    def upload_hyper(self):
        """the step scalars of the CURRENT step count -> device (asynchronous copy from pinned memory on the current stream: ordered in
        front of the next launch / graph replay on it)"""
        slot = self._steps % 16
        if self._hyper_events[slot] is not None:
            self._hyper_events[slot].synchronize()         # (the copy that last read this pinned slot, 16 steps ago)
        row = self._hyper_host[slot]
        self._fill_hyper(row)
        if self._avg is not None:
            row[AVERAGE_SLOT] = self._avg.weight()     # (behind the entries the optimiser kernels read)
        self._hyper_dev.copy_(row, non_blocking=True)
        ev = torch.cuda.Event()
        ev.record()
        self._hyper_events[slot] = ev

    def _advance(self):
        """step count and scalars of the step about to be launched; returns the row the launch reads (HOST = by value, or DEVICE).
        Inside a capture nothing advances: the replay's caller does (graph.GraphedTrainStep)."""
        if self._hyper_dev is not None:
            if not torch.cuda.is_current_stream_capturing():
                self._steps += 1
                self.upload_hyper()
            return self._hyper_dev
        self._steps += 1
        self._fill_hyper(self._row)
        return self._row

    def _clip(self, grad, hyper):
        """the two norm launches over the gradient step() reads, right in front of the update; returns the update kernel's clip pointer"""
        if self.max_grad_norm is None:
            return None
        ops.grad_norm(grad, self.last_grad_norm, self._norm_ws, self.max_grad_norm, self._scale(), hyper if hyper.is_cuda else None)
        return self.last_grad_norm

    # ------------------------------------------------------------------ stock-format (de)serialisation
    def _ordered(self):
        return [p for g in self.param_groups for p in g["params"]]

    def _state_entry(self, views):
        raise NotImplementedError

    def state_dict(self):
        """the stock optimiser's format: tensors in the parameters' logical OIHW shape, indices consecutive over the groups in group order"""
        fp = self.model.flat()
        groups, i = [], 0
        for g in self.param_groups:
            d = {k: v for k, v in g.items() if k != "params"}
            d["params"] = list(range(i, i + len(g["params"])))
            i += len(g["params"])
            groups.append(d)
        state = {}
        live = [(a, key) for a, key in self._STATE if a in self._live() and getattr(self, a) is not None]
        if self._steps > 0 and (live or not self._live()):
            for i, p in enumerate(self._ordered()):
                o = fp.offsets[id(p)]
                entry = self._state_entry({key: FlatParams._view(getattr(self, a), o, p).detach().clone().contiguous() for a, key in live})
                if entry is not None:
                    state[i] = entry
        return {"state": state, "param_groups": groups}

    def _load_groups(self, sd):
        fp = self.model.flat()
        if len(sd["param_groups"]) != len(self.param_groups):
            raise ValueError("optimiser state has %d parameter groups, this optimiser has %d" % (len(sd["param_groups"]), len(self.param_groups)))
        for gi, (g, s) in enumerate(zip(self.param_groups, sd["param_groups"])):
            if len(g["params"]) != len(s["params"]):
                if len(self.param_groups) == 1:
                    raise ValueError("optimiser state has %d parameters, the model has %d" % (len(s["params"]), len(fp.params)))
                raise ValueError("parameter group %d of the optimiser state has %d parameters, here it has %d" % (gi, len(s["params"]), len(g["params"])))
        for g, s in zip(self.param_groups, sd["param_groups"]):
            g.update({k: v for k, v in s.items() if k != "params"})
        return fp, [i for g in sd["param_groups"] for i in g["params"]]


def _stock_defaults(cls, **kw):
    """every key a stock instance writes into its param_groups, with the stock defaults of the installed torch"""
    return dict(cls([torch.nn.Parameter(torch.zeros(1))], **kw).defaults)


class FusedAdam(FusedOptimizer):
    """Drop-in for ``torch.optim.Adam`` (``AdamW`` with decoupled=True) on an EngineNet: lr, betas, eps, weight_decay, amsgrad, parameter
    groups; max_grad_norm clips by the global gradient norm inside the update.  Works with ``torch.optim.lr_scheduler.LambdaLR``.

    With one group, no weight decay, no amsgrad and no clip -- the arguments FusedAdam always had -- step() launches catseg_adam_step /
    catseg_adam_step_dev; anything else launches catseg_adam_step_ex, which writes the same bits where the two overlap.

    ``state_dict()`` / ``load_state_dict()`` speak ``torch.optim.Adam``'s format (per-parameter ``step`` / ``exp_avg`` / ``exp_avg_sq``
    [/ ``max_exp_avg_sq``] in the parameters' logical OIHW shape, indices consecutive over the groups), so an ``optimiser_state_dict``
    written by the reference (BaseManager.py:471-495) resumes here and a checkpoint written here resumes under the stock optimiser.
    Internally the moments are flat fp32 buffers laid out like the parameters (conv weights OHWI)."""
    _STATE = (("_m", "exp_avg"), ("_v", "exp_avg_sq"), ("_vmax", "max_exp_avg_sq"))

    def __init__(self, model, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, grad_scale=1.0, weight_decay=0, amsgrad=False, decoupled=False,
                 groups=None, max_grad_norm=None):
        defaults = _stock_defaults(torch.optim.Adam, lr=lr, betas=betas, eps=eps, weight_decay=weight_decay, amsgrad=amsgrad)
        if "decoupled_weight_decay" in defaults or decoupled:
            defaults["decoupled_weight_decay"] = bool(decoupled)
        super().__init__(model, defaults, groups, grad_scale, max_grad_norm)

    def _live(self):
        return ["_m", "_v", "_vmax"] if self.param_groups[0].get("amsgrad", False) else ["_m", "_v"]

    def _moments(self, fp):
        return tuple(self._state(fp)[:2])

    def _plain(self):
        g = self.param_groups[0]
        return len(self.param_groups) == 1 and not g.get("weight_decay", 0) and not g.get("amsgrad", False) and self.max_grad_norm is None

    def _fill_hyper(self, row):
        g = self.param_groups[0]
        if self._plain():       # {lr, 1 - beta1^step, sqrt(1 - beta2^step), grad_scale}: the row of catseg_adam_step_dev
            ops.lib.catseg_adam_hyper(float(g["lr"]), g["betas"][0], g["betas"][1], max(self._steps, 1), self._scale(), row.data_ptr())
        else:
            ops.optim_hyper(row, max(self._steps, 1), g["betas"][0], g["betas"][1], self._scale(), 0.0,
                            [float(q["lr"]) for q in self.param_groups], [float(q["weight_decay"]) for q in self.param_groups])

    @torch.no_grad()
    def step(self, closure=None):
        fp = self.model.flat()
        state = self._state(fp)
        m, v = state[0], state[1]
        g = self.param_groups[0]
        grad = self._grad(fp)
        if self._plain():
            if self._hyper_dev is not None:
                # device-scalar form (graph.GraphedTrainStep): a launch recorded into a hipGraph reads {lr, bias corrections, gradient scale}
                # from device memory; outside a capture this call advances the step and uploads them itself
                if not torch.cuda.is_current_stream_capturing():
                    self._steps += 1
                    self.upload_hyper()
                ops.adam_step_dev(fp.flat, grad, m, v, self._hyper_dev, g["betas"][0], g["betas"][1], g["eps"])
            else:
                self._steps += 1
                ops.adam_step(fp.flat, grad, m, v, float(g["lr"]), self._steps, g["betas"][0], g["betas"][1], g["eps"],
                              self._scale())
            self._average()
            self._close_window(fp)
            return
        hyper = self._advance()
        clip = self._clip(grad, hyper)
        wd_mode = ops.WD_NONE
        if any(q["weight_decay"] for q in self.param_groups):
            wd_mode = ops.WD_DECOUPLED if g.get("decoupled_weight_decay", False) else ops.WD_COUPLED
        ops.adam_step_ex(fp.flat, grad, m, v, hyper, G=len(self.param_groups), group_map=self._group_map(fp),
                         vmax=state[2] if len(state) > 2 else None, beta1=g["betas"][0], beta2=g["betas"][1], eps=g["eps"], wd_mode=wd_mode,
                         clip=clip)
        self._average()
        self._close_window(fp)

    def _state_entry(self, views):
        return dict({"step": torch.tensor(float(self._steps))}, **views)

    def load_state_dict(self, sd):
        if "state" not in sd or "param_groups" not in sd:
            if {"steps", "m", "v"} <= set(sd):     # round-1 flat format of this package
                self._steps, self._m, self._v = sd["steps"], sd["m"], sd["v"]
                for g, s in zip(self.param_groups, sd.get("param_groups", [])):
                    g.update({k: v for k, v in s.items() if k != "params"})
                return
            raise ValueError("unrecognised optimiser state: expected torch.optim.Adam's {'state', 'param_groups'} dictionary")
        fp, order = self._load_groups(sd)
        bufs = dict(zip(self._live(), self._state(fp)))
        for b in bufs.values():
            b.zero_()
        keys = [(a, key) for a, key in self._STATE if a in bufs]
        steps = set()
        for p, idx in zip(self._ordered(), order):
            st = sd["state"].get(idx)
            if st is None:
                continue
            if tuple(st["exp_avg"].shape) != tuple(p.shape):
                raise ValueError("optimiser state %d has shape %s, parameter has %s" % (idx, tuple(st["exp_avg"].shape), tuple(p.shape)))
            o = fp.offsets[id(p)]
            for a, key in keys:
                if key not in st:
                    raise ValueError("optimiser state %d lacks %r (amsgrad is on)" % (idx, key))
                FlatParams._view(bufs[a], o, p).copy_(st[key])
            steps.add(int(st["step"]))
        if len(steps) > 1:
            raise ValueError("per-parameter step counts differ (%s): not representable by the fused single-step kernel" % sorted(steps))
        self._steps = steps.pop() if steps else 0


class FusedAdamW(FusedAdam):
    """``torch.optim.AdamW``: FusedAdam with decoupled weight decay and torch's default weight_decay = 1e-2"""

    def __init__(self, model, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=1e-2, amsgrad=False, groups=None, max_grad_norm=None,
                 grad_scale=1.0):
        super().__init__(model, lr=lr, betas=betas, eps=eps, grad_scale=grad_scale, weight_decay=weight_decay, amsgrad=amsgrad, decoupled=True,
                         groups=groups, max_grad_norm=max_grad_norm)


class FusedSGD(FusedOptimizer):
    """Drop-in for ``torch.optim.SGD`` on an EngineNet: momentum, dampening, (coupled) weight decay, nesterov, parameter groups, the
    gradient-norm clip.  The momentum buffer starts at zero and the first step runs with dampening 0, which is torch's "buf = g" of
    the first step without a branch a graph replay would freeze.  ``state_dict()`` / ``load_state_dict()`` speak ``torch.optim.SGD``'s
    format (``momentum_buffer`` per parameter; none with momentum 0)."""
    _STATE = (("_buf", "momentum_buffer"),)

    def __init__(self, model, lr=1e-3, momentum=0, dampening=0, weight_decay=0, nesterov=False, groups=None, max_grad_norm=None, grad_scale=1.0):
        defaults = _stock_defaults(torch.optim.SGD, lr=lr, momentum=momentum, dampening=dampening, weight_decay=weight_decay, nesterov=nesterov)
        super().__init__(model, defaults, groups, grad_scale, max_grad_norm)

    def _live(self):
        return ["_buf"] if self.param_groups[0]["momentum"] else []

    def _fill_hyper(self, row):
        g = self.param_groups[0]
        ops.optim_hyper(row, max(self._steps, 1), 0.0, 0.0, self._scale(), float(g["dampening"]),
                        [float(q["lr"]) for q in self.param_groups], [float(q["weight_decay"]) for q in self.param_groups])

    @torch.no_grad()
    def step(self, closure=None):
        fp = self.model.flat()
        state = self._state(fp)
        g = self.param_groups[0]
        grad = self._grad(fp)
        hyper = self._advance()
        clip = self._clip(grad, hyper)
        ops.sgd_step(fp.flat, grad, state[0] if state else None, hyper, G=len(self.param_groups), group_map=self._group_map(fp),
                     momentum=float(g["momentum"]), nesterov=bool(g["nesterov"]), use_wd=any(q["weight_decay"] for q in self.param_groups),
                     clip=clip)
        self._average()
        self._close_window(fp)

    def _state_entry(self, views):
        return views if views else None

    def load_state_dict(self, sd):
        if "state" not in sd or "param_groups" not in sd:
            raise ValueError("unrecognised optimiser state: expected torch.optim.SGD's {'state', 'param_groups'} dictionary")
        fp, order = self._load_groups(sd)
        state = self._state(fp)
        for b in state:
            b.zero_()
        have = []
        for p, idx in zip(self._ordered(), order):
            st = sd["state"].get(idx)
            buf = None if st is None else st.get("momentum_buffer")
            have.append(buf is not None)
            if buf is None:
                continue
            if not state:
                raise ValueError("optimiser state %d holds a momentum buffer, momentum is 0" % idx)
            if tuple(buf.shape) != tuple(p.shape):
                raise ValueError("optimiser state %d has shape %s, parameter has %s" % (idx, tuple(buf.shape), tuple(p.shape)))
            FlatParams._view(state[0], fp.offsets[id(p)], p).copy_(buf)
        if any(have) and not all(have):
            raise ValueError("momentum buffers for %d of %d parameters: the fused kernel keeps one first-step flag for the whole network"
                             % (sum(have), len(have)))
        # torch.optim.SGD stores no step count: what matters is whether the first step (dampening off) is still ahead
        self._steps = 1 if any(have) else 0


# ---------------------------------------------------------------------- config['train']['optimiser']
_COMMON_KEYS = {"name", "weight_decay", "no_decay", "lr_mult", "clip_grad_norm"}
_KEYS = {"Adam": _COMMON_KEYS | {"amsgrad", "betas", "eps"}, "AdamW": _COMMON_KEYS | {"amsgrad", "betas", "eps"},
         "SGD": _COMMON_KEYS | {"momentum", "nesterov", "dampening"}}


def build_optimiser(model, cfg, lr, grad_scale=1.0):
    """the optimiser of config['train']['optimiser'] (a build-side key; the reference builds Adam(lr) only):
    {"name": "Adam" | "AdamW" | "SGD", "weight_decay", "amsgrad", "betas", "eps", "momentum", "nesterov", "dampening",
     "no_decay": ["norm", "bias"], "lr_mult": {"backbone": 0.1}, "clip_grad_norm": 1.0}.  cfg None: FusedAdam(lr) as ever."""
    if cfg is None:
        return FusedAdam(model, lr=lr, grad_scale=grad_scale)
    if not isinstance(cfg, dict) or "name" not in cfg:
        raise ValueError("config['train']['optimiser'] is a dictionary with a 'name'")
    name = cfg["name"]
    if name not in _KEYS:
        raise ValueError("unknown optimiser %r: one of %s" % (name, sorted(_KEYS)))
    unknown = sorted(set(cfg) - _KEYS[name])
    if unknown:
        raise ValueError("unknown key(s) %s in config['train']['optimiser'] for %s: it takes %s" % (unknown, name, sorted(_KEYS[name])))
    kw = {k: cfg[k] for k in ("amsgrad", "eps", "momentum", "nesterov", "dampening") if k in cfg}
    if "betas" in cfg:
        kw["betas"] = tuple(cfg["betas"])
    if "weight_decay" in cfg:
        kw["weight_decay"] = cfg["weight_decay"]
    wd = kw.get("weight_decay", 1e-2 if name == "AdamW" else 0)
    groups = None
    if cfg.get("lr_mult") or (wd and cfg.get("no_decay")):
        groups = param_groups(model, wd, no_decay=tuple(cfg.get("no_decay") or ()), lr_mult=cfg.get("lr_mult"))
    cls = {"Adam": FusedAdam, "AdamW": FusedAdamW, "SGD": FusedSGD}[name]
    return cls(model, lr=lr, groups=groups, max_grad_norm=cfg.get("clip_grad_norm"), grad_scale=grad_scale, **kw)


# ---------------------------------------------------------------------- config['train']['accumulate']
def accumulate_config(n, world=1):
    """config['train']['accumulate'] (a build-side key; the reference steps on every batch): the micro-steps per optimiser step, an
    int >= 1.  None (no key) is 1.  A window over data-parallel ranks is refused."""
    if n is None:
        return 1
    if isinstance(n, bool) or not isinstance(n, int) or n < 1:
        raise ValueError("config['train']['accumulate'] is an int >= 1, got %r" % (n,))
    if n > 1 and world > 1:
        raise ValueError("config['train']['accumulate'] = %d with WORLD_SIZE = %d: the exchange of an accumulated window (once per window, "
                         "behind its last backward pass) is not built" % (n, world))
    return n


# ---------------------------------------------------------------------- the running average of the weights (EMA / SWA)
AVERAGE_MODES = ("ema", "swa")


def average_weight(n, mode="ema", decay=0.999, warmup=False):
    """the weight w of update number n + 1 (n = updates already done, AveragedModel's n_averaged in front of the update) in
    avg = lerp(avg, p, w), in double: 1 for the first update (a copy); 'ema': 1 - decay as torch.optim.swa_utils.get_ema_multi_avg_fn,
    with warmup 1 - min(decay, (1 + n) / (10 + n)); 'swa': 1 / (n + 1), AveragedModel's default (the equal-weight average)."""
    n = int(n)
    if n < 0:
        raise ValueError("average_weight: n counts the updates already done")
    if mode not in AVERAGE_MODES:
        raise ValueError("average_weight: mode is one of %s, got %r" % (list(AVERAGE_MODES), mode))
    if n == 0:
        return 1.0
    if mode == "swa":
        return 1.0 / (n + 1.0)
    d = float(decay)
    if warmup:
        d = min(d, (1.0 + n) / (10.0 + n))
    return 1.0 - d


class WeightAverage:
    """A running average of a network's weights, kept beside the live ones: torch.optim.swa_utils.AveragedModel's arithmetic
    (get_ema_multi_avg_fn(decay) for mode 'ema', the default equal-weight average for 'swa', use_buffers = `buffers`) without a second
    network.  It owns a zero-initialised shadow of model.flat().flat and, with buffers=True, one packed shadow of the running_mean /
    running_var of every BatchNorm module with the device table catseg_ema_table walks; num_batches_tracked is not averaged and the
    generator states of Dropout2d / PointSampler are never touched.

    optimiser.attach_average(avg): every step() launches avg = lerp(avg, p, w) behind the parameter update.  The count of updates is
    derived from the optimiser's step count (n_averaged = steps since the attachment - start_step, never below 0), so whatever saves
    and restores the optimiser's `_steps` and state_buffers() -- graph.GraphedTrainStep's warm-up -- covers the average too.  Steps up
    to start_step run with w = 1: the shadow tracks the weights.

    applied(): swaps the averaged weights (and statistics) into the live model in place for the duration of a `with` block: the flat
    buffer, the weight-image bank and captured graphs keep their pointers; an eval pass builds its weight images in line from what the
    flat buffer holds, the next training pass refreshes its images as every step does."""
    META = "_average"           # state_dict(): the key of the averaging record beside the model's own keys

    def __init__(self, model, decay=0.999, mode="ema", warmup=False, start_step=0, buffers=True):
        if mode not in AVERAGE_MODES:
            raise ValueError("WeightAverage: mode is one of %s, got %r" % (list(AVERAGE_MODES), mode))
        if isinstance(decay, bool) or not isinstance(decay, (int, float)) or not 0.0 <= decay < 1.0:
            raise ValueError("WeightAverage: decay is a number in [0, 1), got %r" % (decay,))
        if isinstance(start_step, bool) or not isinstance(start_step, int) or start_step < 0:
            raise ValueError("WeightAverage: start_step is a non-negative integer, got %r" % (start_step,))
        self.model, self.mode, self.decay, self.warmup = model, mode, float(decay), bool(warmup)
        self.start_step, self.use_buffers = start_step, bool(buffers)
        self.optimiser = None
        self._origin = 0            # the optimiser's step count at this average's step 0
        self._loaded_steps = 0      # steps a loaded state had behind it (applied at the attachment)
        self.shadow = self.buf_shadow = self._table = None
        self._count, self._key, self._slices, self._bns = 0, None, [], None
        self._swapped = False

    # ------------------------------------------------------------------ the count and the weight
    def _attach(self, optimiser):
        self.optimiser = optimiser
        self._origin = optimiser._steps - self._loaded_steps

    @property
    def steps(self):
        """optimiser steps this average has seen (those of the tracking phase included)"""
        return 0 if self.optimiser is None else self.optimiser._steps - self._origin

    @property
    def n_averaged(self):
        return max(0, self.steps - self.start_step)

    @property
    def ready(self):
        """the shadows hold weights (at least one update ran, or a state was loaded)"""
        return self.steps > 0

    def weight(self):
        """the weight of the update behind the optimiser step that `steps` counts (float: the kernels take it as float32)"""
        return average_weight(max(0, self.steps - 1 - self.start_step), self.mode, self.decay, self.warmup)

    def reset(self):
        """forget the average: zero shadows, the count starts at the optimiser's current step"""
        for b in self.buffers():
            b.zero_()
        self._loaded_steps = 0
        if self.optimiser is not None:
            self._origin = self.optimiser._steps

    # ------------------------------------------------------------------ the shadows
    def _bn_modules(self):
        if self._bns is None:       # (the selection of dist.sync_bn_stats)
            self._bns = [(name, m) for name, m in self.model.named_modules()
                         if isinstance(m, torch.nn.modules.batchnorm._BatchNorm) and m.running_mean is not None] if self.use_buffers else []
        return self._bns

    def _ensure(self):
        """the flat parameters; (re)builds the shadows and the table when the flat buffer or a statistics buffer is another tensor
        (the values are carried along where the sizes still match)"""
        fp = self.model.flat()
        if self.shadow is None or self.shadow.numel() != fp.flat.numel() or self.shadow.device != fp.flat.device:
            new = torch.zeros_like(fp.flat)
            if self.shadow is not None and self.shadow.numel() == new.numel():
                new.copy_(self.shadow)
            self.shadow = new
        bns = self._bn_modules()
        if bns:
            key = (fp.flat.device,) + tuple(t.data_ptr() for _, m in bns for t in (m.running_mean, m.running_var))
            if key != self._key:
                rec, slices, off = [], [], 0
                for name, m in bns:
                    for attr in ("running_mean", "running_var"):
                        t = getattr(m, attr)
                        if t.dtype != torch.float32 or not t.is_contiguous():
                            raise ValueError("WeightAverage: %s.%s is not a contiguous float32 buffer" % (name, attr))
                        rec.append((t.data_ptr(), off, t.numel(), 0))
                        slices.append((name + "." + attr if name else attr, off, t.numel()))
                        off += t.numel()
                new = torch.zeros(off, dtype=torch.float32, device=fp.flat.device)
                if self.buf_shadow is not None and self.buf_shadow.numel() == off:
                    new.copy_(self.buf_shadow)
                table = np.array(rec, dtype=ops.EMA_ENTRY)
                self._table = torch.from_numpy(table.view(np.uint8).copy()).to(fp.flat.device)
                self.buf_shadow, self._count, self._slices, self._key = new, len(rec), slices, key
        return fp

    def buffers(self):
        """the shadows (what a snapshot of the training state has to hold; part of the optimiser's state_buffers())"""
        self._ensure()
        return [self.shadow] + ([self.buf_shadow] if self._count else [])

    def update(self):
        """avg = lerp(avg, live, w) on the current stream: one launch over the flat buffer, one over the statistics table.  The weight
        goes by value, or -- the optimiser in its device-scalar form -- is read from the row uploaded with the step scalars."""
        opt = self.optimiser
        if opt is None:
            raise RuntimeError("WeightAverage.update(): attach the average to a fused optimiser first (optimiser.attach_average)")
        if self._swapped:
            raise RuntimeError("WeightAverage.update() inside applied(): the live model holds the averaged weights")
        fp = self._ensure()
        w = opt._hyper_dev[AVERAGE_SLOT:AVERAGE_SLOT + 1] if opt._hyper_dev is not None else self.weight()
        ops.ema_update(fp.flat, self.shadow, w)
        if self._count:
            ops.ema_table(self._table, self._count, self.buf_shadow, ops.EMA_LERP, w)

    # ------------------------------------------------------------------ scoring the average
    def _swap(self):
        fp = self._ensure()
        ops.ema_swap(fp.flat, self.shadow)
        if self._count:
            ops.ema_table(self._table, self._count, self.buf_shadow, ops.EMA_SWAP)
        self._swapped = not self._swapped

    @contextlib.contextmanager
    def applied(self):
        """the averaged weights and statistics in the live model, in place, until the block ends (also by an exception)"""
        if self._swapped:
            raise RuntimeError("WeightAverage.applied() is not re-entrant")
        if not self.ready:
            raise RuntimeError("WeightAverage.applied(): the average holds no weights yet (no optimiser step since it was attached)")
        fp = self.model.flat()
        if fp.flat.is_cuda and torch.cuda.is_current_stream_capturing():
            raise RuntimeError("WeightAverage.applied() inside a stream capture: the swap would become part of the captured graph")
        state = self.model._open_state() if getattr(self.model, "_open_state", None) is not None else None
        if getattr(self.model, "_last_pass", None) is not None or (state is not None and (state.kept or state.refreshed or state.inline)):
            raise RuntimeError("WeightAverage.applied() while a recorded forward pass awaits its backward: that pass would read the "
                               "averaged weights")
        self._swap()
        try:
            yield self
        finally:
            self._swap()

    # ------------------------------------------------------------------ (de)serialisation
    def record(self):
        return {"n_averaged": self.n_averaged, "steps": self.steps, "mode": self.mode, "decay": self.decay, "warmup": self.warmup,
                "start_step": self.start_step}

    def state_dict(self):
        """the averaged network under the model's own state-dict keys (conv weights in their logical OIHW shape; what is not averaged --
        num_batches_tracked, other buffers -- as the live model holds it), and the averaging record under META"""
        fp = self._ensure()
        out = {k: v.detach().clone() for k, v in self.model.state_dict().items()}
        if not self._swapped:       # (inside applied() the live model IS the average)
            for name, p in self.model.named_parameters():
                if name in out:
                    out[name] = FlatParams._view(self.shadow, fp.offsets[id(p)], p).detach().clone().contiguous()
            for key, off, n in self._slices:
                if key in out:
                    out[key] = self.buf_shadow[off:off + n].clone().view(out[key].shape)
        out[self.META] = self.record()
        return out

    def load_state_dict(self, sd):
        """restores the shadows and continues the count: n_averaged (and the position inside the tracking phase) go on from the saved
        record, whatever step count the optimiser's own state format restored"""
        meta = sd.get(self.META)
        if not isinstance(meta, dict) or "n_averaged" not in meta:
            raise ValueError("WeightAverage.load_state_dict: the state lacks its averaging record (%r)" % self.META)
        for k in ("mode", "start_step"):        # (what the count means; decay and warmup may change on a resume)
            if k in meta and meta[k] != getattr(self, k):
                raise ValueError("WeightAverage.load_state_dict: the state was averaged with %s = %r, this average has %r" % (k, meta[k], getattr(self, k)))
        if self._swapped:
            raise RuntimeError("WeightAverage.load_state_dict() inside applied()")
        fp = self._ensure()
        with torch.no_grad():
            for name, p in self.model.named_parameters():
                if name not in sd:
                    raise ValueError("WeightAverage.load_state_dict: %r is missing" % name)
                if tuple(sd[name].shape) != tuple(p.shape):
                    raise ValueError("WeightAverage.load_state_dict: %r has shape %s, the parameter has %s" % (name, tuple(sd[name].shape), tuple(p.shape)))
                FlatParams._view(self.shadow, fp.offsets[id(p)], p).copy_(sd[name])
            for key, off, n in self._slices:
                if key not in sd:
                    raise ValueError("WeightAverage.load_state_dict: %r is missing" % key)
                self.buf_shadow[off:off + n].copy_(sd[key].reshape(-1))
        n_avg = int(meta["n_averaged"])
        self._loaded_steps = int(meta["steps"]) if "steps" in meta else (n_avg + self.start_step if n_avg > 0 else 0)
        if self.optimiser is not None:
            self._origin = self.optimiser._steps - self._loaded_steps


# ---------------------------------------------------------------------- config['train']['ema']
_AVERAGE_KEYS = {"decay": 0.999, "mode": "ema", "warmup": False, "start_step": 0, "buffers": True, "validate": "ema", "infer": True}
AVERAGE_VALIDATE = ("ema", "live", "both")


def average_config(cfg):
    """config['train']['ema'] (a build-side key; the reference has no weight averaging) with its defaults filled in:
    {"decay": 0.999, "mode": "ema" | "swa", "warmup": false, "start_step": 0, "buffers": true, "validate": "ema" | "live" | "both",
     "infer": true}.  None stays None; unknown keys and ill-typed entries are refused."""
    if cfg is None:
        return None
    if not isinstance(cfg, dict):
        raise ValueError("config['train']['ema'] is a dictionary")
    unknown = sorted(set(cfg) - set(_AVERAGE_KEYS))
    if unknown:
        raise ValueError("unknown key(s) %s in config['train']['ema']: it takes %s" % (unknown, sorted(_AVERAGE_KEYS)))
    out = dict(_AVERAGE_KEYS, **cfg)
    for k in ("warmup", "buffers", "infer"):
        if not isinstance(out[k], bool):
            raise ValueError("config['train']['ema'][%r] is true or false, got %r" % (k, out[k]))
    if isinstance(out["decay"], bool) or not isinstance(out["decay"], (int, float)) or not 0.0 <= out["decay"] < 1.0:
        raise ValueError("config['train']['ema']['decay'] is a number in [0, 1), got %r" % (out["decay"],))
    if isinstance(out["start_step"], bool) or not isinstance(out["start_step"], int) or out["start_step"] < 0:
        raise ValueError("config['train']['ema']['start_step'] is a non-negative integer, got %r" % (out["start_step"],))
    if out["mode"] not in AVERAGE_MODES:
        raise ValueError("config['train']['ema']['mode'] is one of %s, got %r" % (list(AVERAGE_MODES), out["mode"]))
    if out["validate"] not in AVERAGE_VALIDATE:
        raise ValueError("config['train']['ema']['validate'] is one of %s, got %r" % (list(AVERAGE_VALIDATE), out["validate"]))
    return out


def build_average(model, optimiser, cfg):
    """the WeightAverage of config['train']['ema'], attached to the optimiser; cfg None: nothing is built or attached"""
    cfg = average_config(cfg)
    if cfg is None:
        return None
    if not isinstance(optimiser, FusedOptimizer):
        raise TypeError("config['train']['ema'] needs a fused optimiser of optim.py")
    avg = WeightAverage(model, decay=cfg["decay"], mode=cfg["mode"], warmup=cfg["warmup"], start_step=cfg["start_step"], buffers=cfg["buffers"])
    return optimiser.attach_average(avg)
