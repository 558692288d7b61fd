"""Optimisers on the flat parameter buffer: one HIP kernel per step for the whole network.

FusedAdam with its constructor arguments of old is torch.optim.Adam(lr) as built at managers/BaseManager.py:441 of the reference and
launches catseg_adam_step / catseg_adam_step_dev (include/catseg.h).  Weight decay (coupled or decoupled), amsgrad, parameter groups,
momentum SGD and clipping by the global gradient norm run on the kernels of include/ext/optim/catseg_optim.h."""
import numpy as np
import torch

from . import ops
from .engine import FlatParams

MAX_GROUPS = ops.OPTIM_MAX_GROUPS


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

    def zero_grad(self, set_to_none=True):
        """The backward tape OVERWRITES each parameter's slice of the flat gradient buffer (it does not accumulate over
        several backward passes: a second backward() before zero_grad() raises); clearing the buffer here matters for
        parameters that receive no gradient in a step (one memset of the flat buffer, ~0.1 ms)."""
        self.model.zero_grad()
        return None

    # ------------------------------------------------------------------ state
    def _live(self):
        """the attributes of the state buffers the current options need"""
        return [a for a, _ in self._STATE]

    def _state(self, fp):
        """the flat state buffers (allocated zero on first use; carried along when the model moved), in _live() order"""
        out = []
        for a in self._live():
            cur = getattr(self, a)
            if cur is None or cur.numel() != fp.flat.numel() or cur.device != fp.flat.device:
                new = torch.zeros_like(fp.flat)
                if cur is not None and cur.numel() == fp.flat.numel():
                    new.copy_(cur)
                setattr(self, a, new)
            out.append(getattr(self, a))
        if self.max_grad_norm is not None and (self.last_grad_norm is None or self.last_grad_norm.device != fp.flat.device):
            self.last_grad_norm = torch.zeros(2, dtype=torch.float32, device=fp.flat.device)
            self._norm_ws = torch.zeros(max(ops.grad_norm_workspace(fp.flat.numel()), 8), dtype=torch.uint8, device=fp.flat.device)
        return out

    def state_buffers(self):
        """every flat state tensor of this optimiser (what a snapshot of the training state has to hold besides `_steps`)"""
        return self._state(self.model.flat())

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
            n = ops.OPTIM_HYPER_FLOATS
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

    def _clip(self, fp, hyper):
        """the two norm launches, right in front of the update; returns the update kernel's clip pointer"""
        if self.max_grad_norm is None:
            return None
        ops.grad_norm(fp.grad, self.last_grad_norm, self._norm_ws, self.max_grad_norm, self.grad_scale, hyper if hyper.is_cuda else None)
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
            ops.lib.catseg_adam_hyper(float(g["lr"]), g["betas"][0], g["betas"][1], max(self._steps, 1), self.grad_scale, row.data_ptr())
        else:
            ops.optim_hyper(row, max(self._steps, 1), g["betas"][0], g["betas"][1], self.grad_scale, 0.0,
                            [float(q["lr"]) for q in self.param_groups], [float(q["weight_decay"]) for q in self.param_groups])

    @torch.no_grad()
    def step(self, closure=None):
        fp = self.model.flat()
        state = self._state(fp)
        m, v = state[0], state[1]
        g = self.param_groups[0]
        if self._plain():
            if self._hyper_dev is not None:
                # device-scalar form (graph.GraphedTrainStep): a launch recorded into a hipGraph reads {lr, bias corrections, gradient scale}
                # from device memory; outside a capture this call advances the step and uploads them itself
                if not torch.cuda.is_current_stream_capturing():
                    self._steps += 1
                    self.upload_hyper()
                ops.adam_step_dev(fp.flat, fp.grad, m, v, self._hyper_dev, g["betas"][0], g["betas"][1], g["eps"])
                return
            self._steps += 1
            ops.adam_step(fp.flat, fp.grad, m, v, float(g["lr"]), self._steps, g["betas"][0], g["betas"][1], g["eps"],
                          self.grad_scale)
            return
        hyper = self._advance()
        clip = self._clip(fp, hyper)
        wd_mode = ops.WD_NONE
        if any(q["weight_decay"] for q in self.param_groups):
            wd_mode = ops.WD_DECOUPLED if g.get("decoupled_weight_decay", False) else ops.WD_COUPLED
        ops.adam_step_ex(fp.flat, fp.grad, m, v, hyper, G=len(self.param_groups), group_map=self._group_map(fp),
                         vmax=state[2] if len(state) > 2 else None, beta1=g["betas"][0], beta2=g["betas"][1], eps=g["eps"], wd_mode=wd_mode,
                         clip=clip)

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
        ops.optim_hyper(row, max(self._steps, 1), 0.0, 0.0, self.grad_scale, float(g["dampening"]),
                        [float(q["lr"]) for q in self.param_groups], [float(q["weight_decay"]) for q in self.param_groups])

    @torch.no_grad()
    def step(self, closure=None):
        fp = self.model.flat()
        state = self._state(fp)
        g = self.param_groups[0]
        hyper = self._advance()
        clip = self._clip(fp, hyper)
        ops.sgd_step(fp.flat, fp.grad, state[0] if state else None, hyper, G=len(self.param_groups), group_map=self._group_map(fp),
                     momentum=float(g["momentum"]), nesterov=bool(g["nesterov"]), use_wd=any(q["weight_decay"] for q in self.param_groups),
                     clip=clip)

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
