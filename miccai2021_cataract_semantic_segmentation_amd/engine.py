"""Execution engine: explicit tape of native kernels (no tracing compiler, no torch ops in the
hot path).  A forward pass records one backward closure per fused layer; the backward pass
walks the tape in reverse, writing parameter gradients straight into one flat fp32 buffer
(so the optimiser is a single kernel and data-parallel all-reduce works on contiguous buckets).

torch.autograd sees exactly one node per network (``NetFunction``) and one per loss, which keeps
the reference's ``loss.backward(); optimiser.step()`` calling convention working.
"""
import collections
import weakref

import torch
from torch import nn

from . import ops
from . import plan as _plan
from .weight_images import WeightImages, network_layers


# --------------------------------------------------------------------------- parameter containers
class Conv2d(nn.Conv2d):
    """Parameter container with nn.Conv2d's init / state-dict behaviour; runs on the HIP engine."""
    stem = False
    exact_operands = False      # forward on the fp32 MFMA kernel whatever the split-precision kernels could take: ops.conv_fwd(exact=)

    def forward(self, x):  # pragma: no cover
        raise RuntimeError("engine Conv2d is executed by the owning network, not called directly")


class BatchNorm2d(nn.BatchNorm2d):
    # frozen: the layer normalises with its running statistics in every pass and never updates them, while its gamma / beta train
    # (bn.eval() inside a training model in stock torch; freeze_bn below).  Not a mode: model.train() / .eval() leave it alone.
    frozen = False

    def __init__(self, *a, **k):
        super().__init__(*a, **k)
        self._pending_batches = 0  # num_batches_tracked is flushed lazily (no per-step kernel)

    def forward(self, x):  # pragma: no cover
        raise RuntimeError("engine BatchNorm2d is executed by the owning network, not called directly")


class _DeviceRng:
    """What the modules that draw on the device share: 16 bytes of device state {seed lo, seed hi, layer | rank << 16, draw counter} as a
    NON-persistent buffer (the state-dict keys stay the reference's).  A draw reads the state on the device and the same launch advances the
    counter: eager steps and hipGraph replays run the same launches and draw the same numbers.  The seed is torch.initial_seed() at the
    first training forward (the managers seed after construction) unless reseed() was called; layer tells the drawing modules of one
    network apart, rank the data-parallel replicas (dist.attach)."""

    def _init_rng(self, layer):
        self.layer, self.rank = int(layer), 0
        self.register_buffer("state", torch.zeros(4, dtype=torch.int32), persistent=False)
        self._seeded = False

    def reseed(self, seed, rank=None):
        """(seed, rank) -> state, the draw counter back to 0"""
        if rank is not None:
            self.rank = int(rank)
        seed = int(seed) & 0xFFFFFFFFFFFFFFFF
        words = [seed & 0xFFFFFFFF, seed >> 32, (self.layer & 0xFFFF) | (self.rank & 0xFFFF) << 16, 0]
        host = torch.tensor([w - (1 << 32) if w >= 1 << 31 else w for w in words], dtype=torch.int32)
        with torch.no_grad():
            self.state.copy_(host)
        self._seeded = True

    def ensure_seeded(self):
        if not self._seeded:
            self.reseed(torch.initial_seed())


class Dropout2d(nn.Dropout2d, _DeviceRng):
    """nn.Dropout2d of a head (models/OCR.py:87, 311-316 of the reference), executed by conv_bn_act(drop=): no parameters; its draws come
    from the device state of _DeviceRng (ops.dropout2d_mask).
    fixed_mask: a test knob -- a [B, C] tensor of zeros and ones used instead of a draw (the state does not move)."""

    def __init__(self, p=0.0, layer=0):
        super().__init__(p)
        self._init_rng(layer)
        self.fixed_mask = None
        self.last = None            # the ops.DropMask of the last training forward

    def forward(self, x):  # pragma: no cover
        raise RuntimeError("engine Dropout2d is executed by the owning network, not called directly")

    def draws(self):
        """a training forward of this module reads its device state"""
        return self.p > 0.0 and self.fixed_mask is None

    def active(self, cx):
        return self.p > 0.0 and cx.train

    def draw(self, B, C, device):
        if self.fixed_mask is not None:
            keep01 = self.fixed_mask.to(device=device, dtype=torch.float32).contiguous()
            if tuple(keep01.shape) != (B, C):
                raise ValueError("Dropout2d.fixed_mask must be [%d, %d], got %s" % (B, C, tuple(keep01.shape)))
            self.last = ops.dropout2d_mask_fixed(keep01, self.p)
        else:
            self.ensure_seeded()
            self.last = ops.dropout2d_mask(self.state, self.p, B, C)
        return self.last


class PointSampler(nn.Module, _DeviceRng):
    """The random points of PointRend's training forward (utils/pointrend_utils.py:65-116 of the reference, whose torch.rand calls are the
    device generator's draws here: ops.pointrend_draw, counter word 2 = 1 where the Dropout2d masks have 0).  No parameters.
    fixed_points: a test knob -- a [N, P, 2] tensor of (x, y) in [0, 1]^2 used instead of the whole sampling (the state does not move)."""

    def __init__(self, layer=0):
        super().__init__()
        self._init_rng(layer)
        self.fixed_points = None

    def forward(self, x):  # pragma: no cover
        raise RuntimeError("engine PointSampler is executed by the owning network, not called directly")

    def draws(self):
        return self.fixed_points is None


class AnchorSampler(nn.Module, _DeviceRng):
    """The draws of the dense contrastive loss's anchor pick (ops.contrast_pick, counter word 2 = 2).  No parameters.  Owned by
    models.Projector, so that what holds for a model's buffers holds for it: graph.GraphedTrainStep seeds it before the capture and restores
    it around the warm-up, dist.attach gives it the rank.  The managers bind it to the loss (loss.sampler = model.projector_model.sampler).
    fixed_u: a test knob -- an int32 tensor of K * M values in [0, 2^24) used instead of the draws (the state does not move)."""

    def __init__(self, layer=0):
        super().__init__()
        self._init_rng(layer)
        self.fixed_u = None

    def forward(self, x):  # pragma: no cover
        raise RuntimeError("engine AnchorSampler is read by losses.DenseContrastiveLoss, not called directly")

    def draws(self):
        return self.fixed_u is None


def rng_modules(module):
    """the modules of a network that own a device generator state"""
    return [m for m in module.modules() if isinstance(m, _DeviceRng)]


def dropout_layers(module):
    return [m for m in module.modules() if isinstance(m, Dropout2d)]


def bn_frozen(bn):
    return bool(getattr(bn, "frozen", False))


def freeze_bn(model, select):
    """sets BatchNorm2d.frozen on the BatchNorm modules `select` names and returns the names of the modules it froze.
    select: True / "all" -- every BatchNorm; "backbone" -- those under backbone. (under the model's `backbone_modules`); a list or tuple of named_modules() prefixes -- those under
    one of them (a prefix names a module: "backbone.layer1" takes backbone.layer1.0.bn1, not backbone.layer10); False / None -- none.
    Anything else, and a selection that matches no BatchNorm module, is a ValueError that quotes the value."""
    if select is None or select is False:
        return []
    if select is True or (isinstance(select, str) and select == "all"):
        prefixes = [""]
    elif isinstance(select, str) and select == "backbone":
        prefixes = list(getattr(model, "backbone_modules", ("backbone",)))      # (EncDec names its trunk enc_model)
    elif isinstance(select, (list, tuple)) and all(isinstance(p, str) for p in select):
        prefixes = list(select)
    else:
        raise ValueError("freeze_bn: expected True, 'all', 'backbone', a list of module name prefixes, False or None, got %r" % (select,))
    frozen = []
    for name, m in model.named_modules():
        if isinstance(m, BatchNorm2d) and any(p == "" or name == p or name.startswith(p + ".") for p in prefixes):
            m.frozen = True
            frozen.append(name)
    if not frozen:
        raise ValueError("freeze_bn: %r matches no BatchNorm module of %s" % (select, type(model).__name__))
    return frozen


def frozen_bn_names(model):
    return [name for name, m in model.named_modules() if isinstance(m, BatchNorm2d) and bn_frozen(m)]


def flush_bn_counters(module):
    for m in module.modules():
        if isinstance(m, BatchNorm2d) and m._pending_batches:
            m.num_batches_tracked += m._pending_batches
            m._pending_batches = 0


# --------------------------------------------------------------------------- flat parameter storage
class FlatParams:
    """All parameters of a network as views into one flat buffer (conv weights physically OHWI),
    gradients likewise.  Rebuilt automatically if the module was moved (.to / .cuda)."""
    ALIGN = 64  # floats

    def __init__(self, module):
        self.module = module
        self.params = [p for p in module.parameters()]
        self.device = None
        self.flat = self.grad = None
        self.offsets = {}

    def _stale(self):
        if self.flat is None:
            return True
        p0, pn = self.params[0], self.params[-1]
        return (p0.device != self.flat.device or p0.data_ptr() != self.flat.data_ptr() + 4 * self.offsets[id(p0)]
                or pn.data_ptr() != self.flat.data_ptr() + 4 * self.offsets[id(pn)])

    def ensure(self):
        if not self._stale():
            return self
        dev = self.params[0].device
        off = 0
        offs = {}
        for p in self.params:
            offs[id(p)] = off
            off += (p.numel() + self.ALIGN - 1) // self.ALIGN * self.ALIGN
        flat = torch.zeros(off, dtype=torch.float32, device=dev)
        grad = torch.zeros(off, dtype=torch.float32, device=dev)
        for p in self.params:
            o, n = offs[id(p)], p.numel()
            pv, gv = self._view(flat, o, p), self._view(grad, o, p)
            pv.copy_(p.data)
            p.data = pv
            p.grad = gv
        self.flat, self.grad, self.offsets, self.device, self.numel = flat, grad, offs, dev, off
        return self

    @staticmethod
    def _view(buf, o, p):
        if p.dim() == 4:
            O, I, kh, kw = p.shape
            return buf[o:o + p.numel()].view(O, kh, kw, I).permute(0, 3, 1, 2)
        return buf[o:o + p.numel()].view(p.shape)

    def bind_grads(self):
        """(re)attach .grad views (optimizer.zero_grad(set_to_none=True) detaches them)"""
        for p in self.params:
            if p.grad is None or p.grad.data_ptr() != self.grad.data_ptr() + 4 * self.offsets[id(p)]:
                p.grad = self._view(self.grad, self.offsets[id(p)], p)


# --------------------------------------------------------------------------- tape
_side_streams = {}


def side_streams(device, n):
    """a small pool of HIP streams per device for the parallel-branch regions (HRNet's branches are independent)"""
    key = (device.type, device.index)
    pool = _side_streams.setdefault(key, [])
    while len(pool) < n:
        pool.append(torch.cuda.Stream(device=device))
    return pool[:n]


PREP_ASYNC = _plan.get("prep_async")
_prep_streams = {}


def prep_stream(device):
    key = (device.type, device.index)
    if key not in _prep_streams:
        _prep_streams[key] = torch.cuda.Stream(device=device)
    return _prep_streams[key]


PARALLEL_BRANCHES = True   # run independent branches (HRNet stages) on separate HIP streams, forward and backward
# streams a parallel region spreads its branches over (branch i runs on stream i % BRANCH_STREAMS): A/B knob, CATSEG_BRANCH_STREAMS
BRANCH_STREAMS = _plan.get("branch_streams")
LAST_BRANCH_ON_MAIN = _plan.get("last_branch_on_main")


class _Region:
    """tape marker of a parallel region: the streams its branches ran on"""
    def __init__(self, streams):
        self.streams = streams


class Ctx:
    def __init__(self, train, record, on_param_grad=None):
        self.train = train
        self.record = record
        self.tape = []
        self.grads = {}
        self.shared = set()
        self.nondiff = set()           # id(output) of the outputs that carry no gradient (PointRend's point coordinates)
        self.on_param_grad = on_param_grad
        self.on_quiet = None           # backward: called on the launch stream between two tape entries outside every parallel region
        self.claimed = set()
        self.branch_stream = None      # stream of the branch being recorded (None: the main stream)
        self.region = None
        self._region_depth = 0         # backward: parallel regions entered and not yet joined
        self._deferred = []            # backward: parameters whose 'gradient ready' signal waits for the join
        self.bn_src = {}               # id(z) -> (y, stats, gamma, beta) of a conv_bn_act output z = relu(bn(y))
        self.bn_pre = {}               # backward: id(z) -> per-tile sums of the already masked gradient of z (conv_bn_act private_in)
        self.pool_pending = {}         # backward: id(z) -> (dpool, idx) of maxpool2(record=True) for the junction backward of conv_act(record="pool")

    def claim(self, *params):
        """every parameter may feed exactly one recorded layer: the backward tape WRITES (does not accumulate) parameter
        gradients and the data-parallel reducer launches a bucket after one 'ready' signal per parameter, so a module
        applied twice in one forward would silently lose a gradient term"""
        if not self.record:
            return
        for p in params:
            if p is None:
                continue
            if id(p) in self.claimed:
                raise NotImplementedError("a parameterised layer is applied twice in one forward pass (shared module): "
                                          "not supported by the HIP engine's backward tape")
            self.claimed.add(id(p))

    def push(self, fn):
        if self.record:
            self.tape.append((fn, self.branch_stream))

    # ---- parallel regions: independent branches on separate HIP streams --------------------------------------------------
    # The kernels of a 192- or 384-channel HRNet branch fill a fraction of the 256 CUs; its three sibling branches are
    # independent until the fuse layer.  Forward: every branch runs on its own side stream (all of them wait for the main
    # stream at the region's start, the main stream waits for all of them at its end and launches nothing in between, so that
    # the caching allocator never hands a block that a side stream still reads to main-stream work).  The tape remembers each
    # closure's stream and the region's boundaries; the backward replay mirrors the same fork / join.
    def parallel(self, device, n):
        cx = self

        class _Par:
            def __enter__(self_):
                self_.on = PARALLEL_BRANCHES and n > 1 and device.type == "cuda"
                if not self_.on:
                    return self_
                self_.main = torch.cuda.current_stream(device)
                ops.images_ready()              # (the branch streams fork from here: they must not wait on the prep stream themselves)
                ns = max(1, min(n, BRANCH_STREAMS))
                if LAST_BRANCH_ON_MAIN and ns >= 4 and cx.record:
                    # The runtime spreads streams over FOUR hardware queues: the main stream holds one, so of four side streams two share a
                    # queue and run one after the other (rocprofv3 kernel trace: streams 3 and 4 on queue 4; per-branch stream times of a
                    # stage-4 module 4.4 / 4.1 / 5.4 / 5.4 ms backward).  The main stream idles during a region: the last branch runs on it.
                    # Only for a RECORDED pass: its tape keeps every tensor a side stream reads alive until the backward has used it, so that
                    # main-stream allocations inside the region cannot be handed a block a side stream still reads (an inference pass frees
                    # a module's inputs as it goes: there the main stream launches nothing between fork and join, as before).
                    self_.streams = side_streams(device, ns - 1) + [self_.main]
                else:
                    self_.streams = side_streams(device, ns)
                ev = torch.cuda.Event(enable_timing=MARKS is not None)
                ev.record(self_.main)
                self_.t0 = ev
                for st in self_.streams:
                    st.wait_event(ev)
                cx.region = _Region(self_.streams)
                if cx.record:
                    cx.tape.append(("region_begin", cx.region))
                return self_

            def branch(self_, i):
                return _Branch(self_, i)

            def __exit__(self_, *exc):
                if not self_.on:
                    return False
                ends = []
                for st in self_.streams:
                    ev = torch.cuda.Event(enable_timing=MARKS is not None)
                    ev.record(st)
                    self_.main.wait_event(ev)
                    ends.append(ev)
                if MARKS is not None:
                    MARKS.append(("region_fwd", self_.t0, ends))
                if cx.record:
                    cx.tape.append(("region_end", cx.region))
                cx.region = None
                return False

        class _Branch:
            def __init__(self_, par, i):
                self_.par, self_.i = par, i

            def __enter__(self_):
                if self_.par.on:
                    st = self_.par.streams[self_.i % len(self_.par.streams)]
                    self_.ctxm = torch.cuda.stream(st)
                    self_.ctxm.__enter__()
                    cx.branch_stream = st
                return self_

            def __exit__(self_, *exc):
                if self_.par.on:
                    cx.branch_stream = None
                    self_.ctxm.__exit__(*exc)
                return False

        return _Par()

    def take(self, t):
        self.shared.discard(id(t))
        return self.grads.pop(id(t), None)

    def _own(self, t):
        """a gradient buffer that several activations share (fan-out of an add) is copied before
        anything is accumulated into it"""
        k = id(t)
        if k in self.shared:
            self.shared.discard(k)
            src = self.grads[k]
            own = torch.empty(src.shape, dtype=torch.float32, device=src.device)
            ops.axpy(src, own, 1.0, False)
            self.grads[k] = own
        return ops.drop_amax(self.grads[k])     # (the caller accumulates into it: a producer's amax record no longer bounds it)

    def give(self, t, g, shared=False):
        assert id(t) not in self.bn_pre, "conv_bn_act(private_in=True): the input has a second consumer"
        if id(t) not in self.grads:
            self.grads[id(t)] = g
            if shared:
                self.shared.add(id(t))
        else:
            ops.axpy(g, self._own(t), 1.0, True)

    def dest(self, t):
        """buffer the gradient of activation t must be written to: (buffer, accumulate?)"""
        assert id(t) not in self.bn_pre, "conv_bn_act(private_in=True): the input has a second consumer"
        if id(t) in self.grads:
            return self._own(t), True
        C = t.shape[-1]
        ld = ops.ld_of(t) if t.dim() == 4 else C
        if t.dim() == 4 and ld != C and ld <= 64:   # small padded rows (class logits): keep the zero pad
            buf = ops.new_act(t.shape[0], t.shape[1], t.shape[2], C, t.device, ld=ld, zero=True)
        else:
            buf = torch.empty(t.shape, dtype=torch.float32, device=t.device)
        self.grads[id(t)] = buf
        return buf, False

    def pgrad(self, p):
        """where the gradient of parameter p is written (None for an absent bias)"""
        return None if p is None else p.grad

    def done(self, *params):
        """gradient of these parameters has been enqueued.  Inside a parallel region the signal is held back until the region
        has joined: the data-parallel reducer launches a bucket's all-reduce behind the CURRENT stream only, and the other
        members of the bucket may have been written on sibling streams."""
        if self.on_param_grad is not None:
            for p in params:
                if p is not None:
                    if self._region_depth > 0:
                        self._deferred.append(p)
                    else:
                        self.on_param_grad(p)

    def backward(self):
        tape = self.tape
        main = None
        region_t0 = None
        while tape:
            fn, tag = tape.pop()
            if isinstance(fn, str):
                region = tag
                if main is None:
                    main = torch.cuda.current_stream(region.streams[0].device)
                if fn == "region_end":          # (reverse order) entering the region: the side streams wait for the main stream
                    ev = torch.cuda.Event(enable_timing=MARKS is not None)
                    ev.record(main)
                    for st in region.streams:
                        st.wait_event(ev)
                    self._region_depth += 1
                    region_t0 = ev
                else:                           # leaving it: the main stream waits for every branch
                    ends = []
                    for st in region.streams:
                        ev = torch.cuda.Event(enable_timing=MARKS is not None)
                        ev.record(st)
                        main.wait_event(ev)
                        ends.append(ev)
                    if MARKS is not None:       # (tools/stage_times.py: how long each branch stream of this region's backward ran)
                        MARKS.append(("region_bwd", region_t0, ends))
                    self._region_depth -= 1
                    if self._region_depth == 0 and self._deferred:
                        ready, self._deferred = self._deferred, []
                        for p in ready:         # (on the main stream, which now follows every branch of the region)
                            self.on_param_grad(p)
                    if self._region_depth == 0 and self.on_quiet is not None and tape:
                        self.on_quiet()
                continue
            if tag is None:
                fn()
                if self._region_depth == 0 and self.on_quiet is not None and tape:
                    self.on_quiet()             # (graph.GraphedTrainStep cuts its capture here when enough buckets are complete)
            else:
                with torch.cuda.stream(tag):
                    fn()
        self.grads.clear()
        self.shared.clear()
        self.bn_src.clear()
        self.bn_pre.clear()
        self.pool_pending.clear()


# --------------------------------------------------------------------------- fused layers
def is_nhwc4(x):
    """network input already in the stem layout [B, H, W, 4] (utils.GpuIngest(..., nhwc4=True)) instead of NCHW [B, 3, H, W]"""
    return x.dim() == 4 and x.shape[-1] == 4 and x.shape[1] != 3


def image_hw(x):
    return tuple(x.shape[1:3]) if is_nhwc4(x) else tuple(x.shape[-2:])


TAPS = None   # diagnostic hook (tools/error_growth.py): a dict collects named intermediate activations (CPU copies, NCHW)


MARKS = None   # diagnostic hook (tools/stage_times.py): a list collects (direction, name, HIP event) at every tap of a pass and of its backward
_cur_cx = None  # the Ctx of the forward pass being recorded (EngineNet._run)


def tap(name, t):
    if MARKS is not None and t.is_cuda:
        ev = torch.cuda.Event(enable_timing=True)
        ev.record()
        MARKS.append(("fwd", name, ev))
        if _cur_cx is not None and _cur_cx.record:
            def mark():
                e2 = torch.cuda.Event(enable_timing=True)
                e2.record()
                MARKS.append(("bwd", name, e2))
            _cur_cx.push(mark)
    if TAPS is not None:
        if getattr(t, "_planes_only", False):       # (exists as fp16 x 2 planes only: h + l, rescaled)
            pl = t._planes
            B, H, W, C = pl.shape
            hl = pl.buf.view(torch.float16).view(2, C // 8, B * H * W, 8).float()
            v = (hl[0] + hl[1]).permute(1, 0, 2).reshape(B, H, W, C) * 2.0 ** (-int(pl.rec[1]))
            TAPS[name] = v.permute(0, 3, 1, 2).contiguous().cpu()
        else:
            TAPS[name] = t.detach().permute(0, 3, 1, 2).contiguous().cpu()
    return t


FUSE_BN_STATS = True  # training forward: BatchNorm batch statistics from the convolution epilogue (False: separate statistics pass)
FUSE_EVAL_BN = True   # eval-mode forward: fold BatchNorm into the conv and fuse bias/residual/ReLU into its epilogue


# ---- the path of one conv_bn_act layer: decided ONCE, in its forward, and written down as a Path ------------------------------------------
# input form -- how the convolution reads x:
#   stem7 / stem3   the image as it is through a direct stem kernel (csrc/stem7.hip: ResNet 7x7/2; csrc/stem3.hip: HRNet 3x3/2), training forward
#                   (also behind a frozen BatchNorm, which then asks the kernel for no statistics)
#   stem4           the implicit GEMM's packed 4-channel stem (image as NHWC-4, weights as ops.stem_pack_weight)
#   pad3            a 3-channel image into a generic convolution: image and weights padded to 4 channels
#   plain           an NHWC activation
STEM7, STEM3, STEM4, PAD3, PLAIN = "stem7", "stem3", "stem4", "pad3", "plain"
# forward form: eval-mode BatchNorm folded into the convolution / training (batch statistics) / eval-mode BatchNorm as a kernel of its own
# (a frozen BatchNorm in a training or recorded pass: running statistics, and a backward of its own -- ops.bn_backward_frozen)
FOLDED, TRAIN, EVAL = "folded", "train", "eval"
# backward form (recorded training passes only, else None) -- in which form the gradient of the convolution's output exists:
#   planes   fp16 x 2 planes that the trunk's plane kernels stream (_bwd_planes)
#   h2       blocked f16x2 planes that both GEMMs of a head layer read (_bwd_h2)
#   head     as h2, behind the fused BatchNorm + ReLU + classifier (_fused_head / _bwd_fused_head)
#   generic  an fp32 tensor (_bwd_generic); the only form of a frozen BatchNorm
BWD_PLANES, BWD_H2, BWD_HEAD, BWD_GENERIC = "planes", "h2", "head", "generic"
Path = collections.namedtuple("Path", "input forward backward")

# what a recorded layer keeps for its backward (z: the tensor whose cotangent starts it -- the fused head's logits on that form)
# (stats: the batch statistics of a TRAIN layer; a frozen layer has None there and keeps `scale`, the row its forward normalised with)
_Saved = collections.namedtuple("_Saved", "cx path c bn x x_in wk y stats yrec z relu residual need_dx private_in scale")

# the first pass of a BatchNorm's backward as its private_in consumer's backward-data epilogue left it: sums = what ops.bn_backward_pre /
# bn_backward_pre_planes take, planes = it came from the plane kernel (ops.conv_bwd_data_pl) and carries max|g|
_Pre = collections.namedtuple("_Pre", "sums planes")


def _input_form(cx, x, conv, c, need_dx, out):
    w3 = (not conv.stem) and c.weight.shape[1] == 3       # 3-channel image into a generic conv (HRNet 3x3/2 stem)
    direct = cx.train and c.bias is None and not need_dx and out is None
    if (conv.stem and direct and c.weight.data.is_contiguous(memory_format=torch.channels_last)
            and ops.stem7_ok(x, c.weight.data, c.kh, c.kw, c.stride, c.pad, c.dil, c.groups)):
        # the ResNet stem's first convolution, training forward: the direct fp64-accumulating kernel on the image as it is (csrc/stem7.hip);
        # the backward-weight pass packs its operands for the implicit GEMM itself
        return STEM7
    if conv.stem:
        return STEM4
    if w3 and direct and ops.stem3_ok(x, c.weight.data, c.kh, c.kw, c.stride, c.pad, c.dil, c.groups):
        # the HRNet stem's first convolution: HBM-bound direct kernels on the image as it is (NCHW or NHWC-4), no repack, no channel padding
        return STEM3
    return PAD3 if w3 else PLAIN


def _conv_input(inp, x, c):
    """(x_in, wk): input and weights as the forward kernel of input form `inp` reads them"""
    if inp == STEM4:
        return (x if is_nhwc4(x) else ops.nchw3_to_nhwc4(x)), ops.stem_pack_weight(c.weight.data, c.Cout)
    if inp == PAD3:
        return (x if is_nhwc4(x) else ops.nchw3_to_nhwc4(x)), ops.weight_pad_cin(c.weight.data, c.Cout, c.kh * c.kw, 3, 4)
    return x, c.weight.data


def _conv_weight_grad(cx, inp, c, x_in, wk, dy):
    """weight (and bias) gradient of a convolution of input form `inp` from its fp32 output gradient"""
    dw, dbias = cx.pgrad(c.weight), cx.pgrad(c.bias)
    if inp in (STEM7, STEM4):
        x4 = x_in if is_nhwc4(x_in) else ops.nchw3_to_nhwc4(x_in)      # (stem7: the forward read the image as it was)
        dpk = torch.empty((c.Cout, 7, 8, 4), dtype=torch.float32, device=dy.device)     # the packed layout of ops.stem_pack_weight
        ops.conv_bwd_weight(x4, dy, dpk, dbias, c.kh, c.kw, c.stride, c.pad, c.dil, stem4=True)
        ops.stem_unpack_grad(dpk, dw, c.Cout)
    elif inp == STEM3:
        ops.stem3_bwd_weight(x_in, dy, dw)
    elif inp == PAD3:
        dpk = torch.empty_like(wk)
        ops.conv_bwd_weight(x_in, dy, dpk, dbias, c.kh, c.kw, c.stride, c.pad, c.dil)
        ops.weight_unpad_cin(dpk, dw, c.Cout, c.kh * c.kw, 3, 4)
    else:
        ops.conv_bwd_weight(x_in, dy, dw, dbias, c.kh, c.kw, c.stride, c.pad, c.dil, groups=c.groups)


def _backward_form(inp, c, x_in, y, yrec, partials, relu, residual, out, need_dx, head):
    """the backward form of a recorded training layer, from what its forward knows.  Everything asked here holds until the layer's backward:
    the module switches behind ops.h2_dy_route are set before a pass, not inside one (and the forward of the fused head has already acted
    on the answer), shapes and modules do not change."""
    if yrec is not None:
        # The convolution ran the plane kernel (ops.fwd_route: D3P), which takes no bias and reads the planes of x -- its producer's, or the
        # ones ops.conv_fwd attached to x for this layer.  They are still there in the backward: `_planes` is an attribute of the tensor
        # OBJECT, and ops.drop_amax clears it only on the destination of a launch that overwrites that object.  A recorded pass writes an
        # activation before its first consumer reads it (every form's backward-weight reads x as the forward saw it), a tensor with planes
        # is never an `out=` view of a concatenation buffer (bn_apply writes planes only where out is None), and the destinations of the
        # backward pass are gradient buffers (Ctx.dest / Ctx._own).  (The fused head below needs no planes for z, i.e. zrec is None; with
        # its other conditions that means yrec is None: planes_ok held for this width a moment ago, inside ops.conv_fwd.)
        return BWD_PLANES
    if residual is None and inp == PLAIN and ops.h2_dy_route(x_in, y, c.weight.data, c.kh, c.kw, c.stride, c.pad, c.dil, c.groups, need_dx):
        # head layers on the f16x2 kernels: dy exists only as the blocked planes both of its consumers read
        if (head is not None and TAPS is None and relu and out is None and partials is not None and head.kernel_size == (1, 1)
                and head.stride == (1, 1) and head.padding == (0, 0) and head.groups == 1 and ops.head_fuse_ok(y, head.weight.shape[0])):
            return BWD_HEAD
        return BWD_H2
    return BWD_GENERIC


def _fused_head(L, scale, head, pad_to, dm=None):
    """BatchNorm + ReLU + the K-class 1 x 1 classifier `head` behind the head convolution whose output L.y (and batch statistics) exist:
    the normalised activation and its gradient are never written (ops.head_fwd / ops.head_backward, csrc/headfuse.h); the convolution's
    backward streams the blocked planes of dy as on the h2 form."""
    hw, K = head.weight, head.weight.shape[0]
    L.cx.claim(hw, head.bias)
    hb = head.bias.data if head.bias is not None else None
    logits = ops.head_fwd(L.y, L.stats[:L.c.Cout], scale, L.bn.bias.data, hw.data, hb, K, max(pad_to, (K + 3) // 4 * 4), drop=dm)
    L = L._replace(z=logits)
    L.cx.push(lambda: _bwd_fused_head(L, head, dm))
    return logits


def _bwd_fused_head(L, head, dm=None):
    cx, bn = L.cx, L.bn
    dl = cx.take(L.z)
    if dl is None:
        return
    dyp, dysc = ops.head_backward(dl, L.y, L.stats, bn.weight.data, bn.bias.data, head.weight.data, cx.pgrad(head.weight), cx.pgrad(head.bias),
                                  cx.pgrad(bn.weight), cx.pgrad(bn.bias), cx.pgrad(L.c.bias), drop=dm)
    del dl
    cx.done(head.weight, head.bias)
    _h2_tail(L, dyp, dysc)


def _h2_tail(L, dyp, dysc):
    """backward-weight and backward-data of a head convolution from the blocked planes of its output gradient"""
    cx, c, x = L.cx, L.c, L.x
    ops.conv_bwd_weight_h2(L.x_in, dyp, dysc, c.Cout, cx.pgrad(c.weight), c.kh, c.kw, c.stride, c.pad, c.dil)
    if L.need_dx:
        dx, accx = cx.dest(x)
        ops.conv_bwd_data_h2(dyp, dysc, c.weight.data, tuple(x.shape), c.Cout, c.kh, c.kw, c.pad, c.dil, dx, accx)
    cx.done(L.bn.weight, L.bn.bias, c.weight, c.bias)


def _conv_bn_act_backward(L):
    """tape entry of a conv_bn_act layer: its backward form, but for what only the backward knows -- whether z's private_in consumer ran
    the first pass of this BatchNorm's backward in its backward-data epilogue (`pre`), and in which kernel.  The planes form merges a
    pre of the plane kernel only, the h2 form none; the generic form takes either."""
    pre = L.cx.bn_pre.pop(id(L.z), None)
    L.cx.bn_src.pop(id(L.z), None)          # (its private_in consumer, if any, has run: y is not kept alive beyond this layer's backward)
    form = L.path.backward
    if form == BWD_PLANES and (pre is None or pre.planes):
        _bwd_planes(L, pre)
    elif form == BWD_H2 and pre is None:
        _bwd_h2(L)
    else:
        _bwd_generic(L, pre)


def _cotangent(L):
    """(dz, dres, accumulate): the gradient of the layer's output -- None when nothing reached it -- and where the residual branch's goes"""
    dz = L.cx.take(L.z)
    if dz is None or L.residual is None:
        return dz, None, False
    return (dz,) + L.cx.dest(L.residual)


def _input_grad(L, dgrad, planes):
    """dx through dgrad(dx, accumulate, bn_src) -> (dx, pre), one of ops.conv_bwd_data / conv_bwd_data_pl(with_pre=True).  private_in: x is
    relu(bn(.)) of the preceding conv_bn_act and has no other consumer; where this call is the first contribution to its gradient the
    kernel may run the first pass of that BatchNorm's backward in its epilogue, and that layer's backward finds `pre` under cx.bn_pre."""
    cx, x = L.cx, L.x
    dx, accx = cx.dest(x)
    src = cx.bn_src.get(id(x)) if (L.private_in and not accx) else None
    pre = dgrad(dx, accx, src)[1]
    if pre is not None:
        cx.bn_pre[id(x)] = _Pre(pre, planes)


def _bwd_planes(L, pre):
    """planes form: the gradient of the convolution's output exists as planes only; backward-weight and backward-data stream them"""
    cx, bn, w = L.cx, L.bn, L.c.weight
    dz, dres, acc = _cotangent(L)
    if dz is None:
        return
    if pre is not None:
        dyp = ops.bn_backward_pre_planes(dz, L.y, L.stats, bn.weight.data, pre.sums, L.yrec, cx.pgrad(bn.weight), cx.pgrad(bn.bias))
    else:
        z_mask = L.z if (L.residual is not None or not L.relu) else None
        dyp = ops.bn_backward_planes(dz, z_mask, L.y, L.stats, bn.weight.data, L.relu, cx.pgrad(bn.weight), cx.pgrad(bn.bias), dres, acc,
                                     bn.bias.data, L.yrec)
    del dz
    ops.dwgrad3_pl(ops.planes_of(L.x_in), dyp, cx.pgrad(w))
    if L.need_dx:
        _input_grad(L, lambda dx, accx, src: ops.conv_bwd_data_pl(dyp, w.data, dx, accumulate=accx, bn_src=src, with_pre=True), True)
    cx.done(bn.weight, bn.bias, w, L.c.bias)


def _bwd_h2(L):
    """h2 form: dy exists only as the blocked planes both of its consumers read (ops.bn_backward_h2)"""
    cx, bn = L.cx, L.bn
    dz = cx.take(L.z)
    if dz is None:
        return
    dyp, dysc = ops.bn_backward_h2(dz, L.y, L.stats, bn.weight.data, L.relu, cx.pgrad(bn.weight), cx.pgrad(bn.bias), bn.bias.data,
                                   cx.pgrad(L.c.bias))
    del dz
    _h2_tail(L, dyp, dysc)


def _bwd_generic(L, pre):
    """generic form: dy as an fp32 tensor through ops.conv_bwd_weight / conv_bwd_data"""
    cx, bn, c, x = L.cx, L.bn, L.c, L.x
    dz, dres, acc = _cotangent(L)
    if dz is None:
        return
    # without a residual branch the ReLU mask is recomputed from y (z is not read: 1 of 3 tensor reads saved)
    z_mask = L.z if (L.residual is not None or not L.relu) else None
    if L.path.forward == EVAL:
        # frozen statistics: one pass, dy = g * scale (the layer registered no bn_src: no consumer has run a first pass for it)
        assert pre is None
        dy = ops.bn_backward_frozen(dz, z_mask, L.y, bn.running_mean, bn.running_var, bn.eps, L.scale, L.relu, cx.pgrad(bn.weight),
                                    cx.pgrad(bn.bias), dres, acc, beta=bn.bias.data)
    elif pre is not None:
        # dz is already masked and its per-tile sums exist (the consumer's backward-data epilogue): merge + apply only
        dy = ops.bn_backward_pre(dz, L.y, L.stats, bn.weight.data, pre.sums, cx.pgrad(bn.weight), cx.pgrad(bn.bias))
    else:
        dy = ops.bn_backward(dz, z_mask, L.y, L.stats, bn.weight.data, L.relu, cx.pgrad(bn.weight), cx.pgrad(bn.bias), dres, acc,
                             beta=bn.bias.data)
    del dz
    _conv_weight_grad(cx, L.path.input, c, L.x_in, L.wk, dy)
    if L.path.input == PLAIN and L.need_dx:         # (every other input form reads the image)
        _input_grad(L, lambda dx, accx, src: ops.conv_bwd_data(dy, c.weight.data, tuple(x.shape), c.kh, c.kw, c.stride, c.pad, c.dil, out=dx,
                                                               accumulate=accx, groups=c.groups, bn_src=src, with_pre=True), False)
    cx.done(bn.weight, bn.bias, c.weight, c.bias)


def _dropout_pass(cx, z, dm):
    """Dropout2d as a pass of its own behind bn_apply (every form but the fused head): z_d = m z, and the tape entry dz = m dz_d"""
    zd = ops.dropout2d_apply(z, dm)
    if cx.record:
        def bwd():
            dzd = cx.take(zd)
            if dzd is None:
                return
            dz, acc = cx.dest(z)
            assert not acc, "Dropout2d is the only consumer of the activation in front of it"
            ops.dropout2d_apply(dzd, dm, out=dz)
        cx.push(bwd)
    return zd


def conv_bn_act(cx, x, conv, bn, relu=True, residual=None, out=None, need_dx=True, private_in=False, sole_conv_out=False, head=None, z_tap=None,
                drop=None):
    """conv -> BatchNorm (batch stats in training) -> (+residual) -> (ReLU).  x NHWC (or the raw
    NCHW image for the stem).  Returns z (NHWC).
    head: a 1 x 1 classifier convolution that is the ONLY consumer of z -- the call then returns conv_bias(z, head), and in a recorded training
    pass on the head layers' route BatchNorm, ReLU and classifier run fused (_fused_head: z is never written); z_tap names z for the diagnostic
    taps where it exists.
    drop: an engine.Dropout2d behind the ReLU (in front of `head`).  In a training forward with p > 0 it draws one mask; the fused head takes it
    into its kernels, every other form applies it as a pass between bn_apply and what follows (z_tap then names the dropped activation, as the
    reference's ocr_representation).  In eval mode and with p = 0 it launches nothing and its state does not move.
    private_in: the caller states that x is the output of the preceding conv_bn_act (ReLU, no residual) and has NO other consumer
    (the first half of a BasicBlock).  The backward-data kernel of this layer may then run the first pass of that BatchNorm's
    backward in its epilogue (ops.conv_bwd_data(bn_src=...)).
    sole_conv_out: the caller states that the OUTPUT of this layer feeds nothing but one conv_bn_act(private_in=True) (the same first half
    of a BasicBlock, seen from the producer): on the planes route (ops.planes_ok) it then exists as fp16 x 2 planes only."""
    c = ops.conv_args(conv)
    Cout = c.Cout
    inp = _input_form(cx, x, conv, c, need_dx, out)
    x_in, wk = _conv_input(inp, x, c)
    bias = c.bias.data if c.bias is not None else None
    cx.claim(c.weight, c.bias, bn.weight, bn.bias)
    frozen = bn_frozen(bn)
    fwd = FOLDED if (not cx.train and not cx.record and FUSE_EVAL_BN) else TRAIN if (cx.train and not frozen) else EVAL
    if fwd == FOLDED:
        # inference fast path: eval-mode BatchNorm folded into the weights, bias + residual + ReLU applied in
        # the convolution epilogue — one kernel per layer, no separate normalisation pass over HBM
        per_out = wk.numel() // Cout
        wf, bf = ops.fold_bn(wk, bias, bn.weight.data, bn.bias.data, bn.running_mean, bn.running_var, bn.eps, Cout, per_out)
        zf = ops.conv_fwd_fused(x_in, wf, bf, residual, relu, Cout, c.kh, c.kw, c.stride, c.pad, c.dil, out=out, stem4=inp == STEM4, groups=c.groups)
        if z_tap is not None:
            tap(z_tap, zf)
        return zf if head is None else conv_bias(cx, zf, head)
    partials = yrec = zrec = None
    dropping = drop is not None and drop.active(cx)        # (Dropout2d follows the pass's mode, not the BatchNorm's: active() asks cx.train)
    if dropping and (not relu or residual is not None or out is not None):
        raise NotImplementedError("conv_bn_act(drop=): Dropout2d follows BatchNorm + ReLU of a layer without residual branch or out= view")
    if fwd == TRAIN:
        # batch statistics: per-tile partial sums come out of the convolution's epilogue (no separate pass over y)
        if inp == STEM3:
            res = ops.stem3_fwd(x_in, wk, None, bn_stats=FUSE_BN_STATS)
        elif inp == STEM7:
            res = ops.stem7_fwd(x_in, wk, None, bn_stats=FUSE_BN_STATS)
        else:
            res, yrec = ops.conv_fwd(x_in, wk, bias, Cout, c.kh, c.kw, c.stride, c.pad, c.dil, stem4=inp == STEM4, groups=c.groups,
                                     bn_stats=FUSE_BN_STATS, train=cx.record, exact=conv.exact_operands, with_yrec=True)
        y, partials = res if FUSE_BN_STATS else (res, None)
        # planes route: the convolution streamed planes and left max|y| (yrec); then the BatchNorm's output gets planes too (exponent from a bound)
        if (yrec is not None and partials is not None and out is None and not dropping and ops.planes_ok(Cout, ops.rows_of(y))
                and (residual is None or ops.amax_of(residual) is not None)):
            zrec = ops.new_amax(y.device)
        if partials is not None:
            stats, scale = ops.bn_finalize(partials, ops.rows_of(y), Cout, bn.weight.data, bn.eps, bn.momentum, bn.running_mean, bn.running_var,
                                           bound=(bn.bias.data, yrec, zrec) if zrec is not None else None)
        else:
            stats, scale = ops.bn_train_stats(y, bn.weight.data, bn.eps, bn.momentum, bn.running_mean, bn.running_var)
        bn._pending_batches += 1
        mean = stats[:Cout]
    else:
        if inp == STEM3:        # (the direct stem forms are chosen for a training pass: here behind a frozen BatchNorm, without statistics)
            y = ops.stem3_fwd(x_in, wk, None)
        elif inp == STEM7:
            y = ops.stem7_fwd(x_in, wk, None)
        else:
            # (exact: the rule of the trunk's first layers holds for a training pass whatever the BatchNorm behind them does)
            y = ops.conv_fwd(x_in, wk, bias, Cout, c.kh, c.kw, c.stride, c.pad, c.dil, stem4=inp == STEM4, groups=c.groups, train=cx.record,
                             exact=cx.train and conv.exact_operands)
        stats = None
        mean = bn.running_mean
        scale = ops.bn_eval_scale(bn.weight.data, bn.running_var, bn.eps)
    if cx.record and fwd != TRAIN and not frozen:
        raise NotImplementedError("backward through eval-mode BatchNorm is not on the training path")
    path = Path(inp, fwd, None if not cx.record else BWD_GENERIC if frozen else
                _backward_form(inp, c, x_in, y, yrec, partials, relu, residual, out, need_dx, head))
    dm = drop.draw(y.shape[0], Cout, y.device) if dropping else None
    if path.backward == BWD_HEAD:
        return _fused_head(_Saved(cx, path, c, bn, x, x_in, wk, y, stats, yrec, None, relu, residual, need_dx, private_in, None), scale, head, 32, dm)
    z = ops.bn_apply(y, mean, scale, bn.bias.data, residual, relu, out=out, planes_rec=zrec,
                     planes_only=zrec is not None and sole_conv_out and relu and residual is None,
                     want_mask=cx.record and cx.train,       # (a residual block's output: its ReLU mask as bits for the backward pass)
                     want_record=not frozen)
    # (no amax record behind a frozen BatchNorm: the kernels that split their input in registers scale it by max|z| and keep their 2^-22
    #  only for elements within 2^-17 of it (csrc/planes.h) -- a range batch statistics guarantee and running statistics that need not fit
    #  the batch do not.  Its consumers take the three-plane kernels, which have fp32's exponent range)
    if cx.record:
        if fwd == TRAIN and relu and residual is None and out is None and dm is None:
            # for a private_in consumer of z (not behind a frozen BatchNorm: that pass belongs to a batch-statistics backward)
            cx.bn_src[id(z)] = (y, stats, bn.weight.data, bn.bias.data)
        L = _Saved(cx, path, c, bn, x, x_in, wk, y, stats, yrec, z, relu, residual, need_dx, private_in, scale if frozen else None)
        cx.push(lambda: _conv_bn_act_backward(L))
    if dm is not None:
        z = _dropout_pass(cx, z, dm)
    if z_tap is not None:
        tap(z_tap, z)
    return z if head is None else conv_bias(cx, z, head)


def conv_bias(cx, x, conv, pad_to=32):
    """plain conv (+bias), used for the K-class classifier heads.  The output keeps a zero-padded
    row stride (pad_to floats) so that it can feed 16-byte-granular kernels."""
    w, Cout, kh, kw, s, p, d, _, b = ops.conv_args(conv)
    ld = max(pad_to, (Cout + 3) // 4 * 4)
    y = ops.conv_fwd(x, w.data, b.data if b is not None else None, Cout, kh, kw, s, p, d, zero_to=ld, train=cx.record)
    cx.claim(w, b)
    if cx.record:
        def bwd():
            dy = cx.take(y)
            if dy is None:
                return
            if ops.ld_of(dy) % 4:   # the layer is the network's output (models/UNet.py) and the loss hands its gradient over as a dense
                #                     [B, H, W, K] tensor: re-pitch it (a copy), as conv_transpose_bwd does
                padded = ops.new_act(dy.shape[0], dy.shape[1], dy.shape[2], Cout, dy.device, ld=ld, zero=True)
                padded.copy_(dy)
                dy = padded
            ops.conv_bwd_weight(x, dy, cx.pgrad(w), cx.pgrad(b), kh, kw, s, p, d)
            dx, acc = cx.dest(x)
            ops.conv_bwd_data(dy, w.data, tuple(x.shape), kh, kw, s, p, d, out=dx, accumulate=acc)
            cx.done(w, b)
        cx.push(bwd)
    return y


def conv_act(cx, x, conv, relu=True, record=False):
    """conv + bias (+ ReLU) without normalisation -- the VGG-style layers of models/FCN.py:42-55 of the reference: bias and ReLU run in
    the convolution's epilogue.  x NHWC (or the raw NCHW image for a 3-channel first layer).
    record (models/UNet.py; needs relu; a no-op unless ops.bnfree_records()): the layer works on amax records -- its forward takes the
    route the planner gives an input with a record, its output z carries one, and its backward masks dz with ops.relu_bwd_rec, so that
    backward-data and backward-weight see the record of dy.  record=True: z's record comes from a pass of its own (ops.amax_record) unless
    the ReLU pass behind a direct / gather kernel has left it; record="pool": z is read by maxpool2(record=True) and upcat alone -- the pool
    leaves z's record, and the layer's backward adds the pooled gradient to the concatenation's slice in the same pass (junction form)."""
    c = ops.conv_args(conv)
    inp = PAD3 if c.weight.shape[1] == 3 else PLAIN
    x_in, wk = _conv_input(inp, x, c)
    cx.claim(c.weight, c.bias)
    rec = bool(record) and relu and ops.bnfree_records()
    bias = c.bias.data if c.bias is not None else None
    direct = rec and inp == PLAIN and ops.fwd_route(ops.Layer(x_in.shape, c.Cout, c.kh, c.kw, c.stride, c.pad, c.dil, ldx=ops.ld_of(x_in), bias=bias is not None,
                                                              x_amax=ops.amax_of(x_in) is not None)).kind in ("d3h", "d3", "p1", "s2p")
    if direct:
        # the direct / pointwise / gather kernels add the bias but have no ReLU epilogue: the ReLU pass that follows leaves z's record
        z = ops.conv_fwd(x_in, wk, bias, c.Cout, c.kh, c.kw, c.stride, c.pad, c.dil, train=cx.record)
        ops.add_n_act([z], True, out=z)
    else:
        z = ops.conv_fwd_fused(x_in, wk, bias, None, relu, c.Cout, c.kh, c.kw, c.stride, c.pad, c.dil)
        if rec and record != "pool":
            ops.amax_record(z)
    if rec and record == "pool":
        z._junction = True
    if cx.record:
        def bwd():
            dz = cx.take(z)
            pend = cx.pool_pending.pop(id(z), None)
            if dz is None and pend is not None:     # (only the pool consumed z)
                dz = torch.empty(z.shape, dtype=torch.float32, device=z.device)
                ops.maxpool2_bwd(pend[0], pend[1], dz)
                pend = None
            if dz is None:
                return
            if rec:
                dy = ops.relu_bwd_rec(dz, z, pool=pend)
            else:
                dy = ops.relu_bwd(dz, z) if relu else dz
            del dz, pend
            _conv_weight_grad(cx, inp, c, x_in, wk, dy)
            if inp == PLAIN:
                dx, acc = cx.dest(x)
                ops.conv_bwd_data(dy, c.weight.data, tuple(x.shape), c.kh, c.kw, c.stride, c.pad, c.dil, out=dx, accumulate=acc)
            cx.done(c.weight, c.bias)
        cx.push(bwd)
    return z


def maxpool2(cx, x, record=False):
    """F.max_pool2d(x, 2) (models/FCN.py:44-53 of the reference).  record (a no-op unless ops.bnfree_records()): the pass also leaves the
    amax records of x and of the result (ops.maxpool2_fwd_rec); where x is the output of conv_act(record="pool") the pooled gradient is
    not scattered here but handed to that layer's backward (Ctx.pool_pending)."""
    rec = record and ops.bnfree_records()
    y, idx = ops.maxpool2_fwd_rec(x) if rec else ops.maxpool2_fwd(x)
    if cx.record:
        junction = rec and getattr(x, "_junction", False)

        def bwd():
            dy = cx.take(y)
            if dy is None:
                return
            if junction:
                cx.pool_pending[id(x)] = (dy, idx)
                return
            dx, acc = cx.dest(x)
            ops.maxpool2_bwd(dy, idx, dx, acc)
        cx.push(bwd)
    return y


def upcat(cx, x, skip):
    """torch.cat([Upsample(2, bilinear, align_corners=True)(x), skip], 1) (models/UNet.py:48-57 of the reference).  With ops.bnfree_records()
    one launch that also leaves the concatenation's amax record (ops.upcat2x_fwd); otherwise composed of bilinear(out=slice), copy_into
    and concat_views.  Either way the gradient of the resized half goes back through bilinear_bwd on its slice and skip receives its slice."""
    B, h, w, Cx = x.shape
    Cs = skip.shape[-1]
    if not ops.bnfree_records():
        cat = torch.empty((B, 2 * h, 2 * w, Cx + Cs), dtype=torch.float32, device=x.device)
        up = bilinear(cx, x, 2 * h, 2 * w, True, out=cat[..., :Cx])
        sk = copy_into(cx, skip, cat[..., Cx:])
        return concat_views(cx, cat, [(up, 0, Cx), (sk, Cx, Cx + Cs)])
    cat = ops.upcat2x_fwd(x, skip)
    if cx.record:
        def bwd():
            dcat = cx.take(cat)
            if dcat is None:
                return
            dx, acc = cx.dest(x)
            ops.bilinear_bwd(dcat[..., :Cx], tuple(x.shape), True, out=dx, accumulate=acc)
            cx.give(skip, dcat[..., Cx:])
        cx.push(bwd)
    return cat


class ConvTranspose2d(nn.ConvTranspose2d):
    """Parameter container with nn.ConvTranspose2d's init / state-dict behaviour (weight [Cin, Cout, k, k]); runs on the HIP engine."""

    def forward(self, x, output_size=None):  # pragma: no cover
        raise RuntimeError("engine ConvTranspose2d is executed by the owning network, not called directly")


def conv_transpose(cx, x, deconv):
    """nn.ConvTranspose2d on a class-logit tensor (rows zero padded to 32 floats: conv_bias's output).  The transposed convolution IS the
    backward-data pass of the convolution with the same weight tensor; its own backward is that convolution's forward / backward-weight."""
    w, Cout, k, kw, s, p, d, groups, b = ops.conv_args(deconv)
    assert k == kw and deconv.output_padding[0] == 0 and d == 1 and groups == 1
    cx.claim(w, b)
    y, wp = ops.conv_transpose_fwd(x, w.data, b.data if b is not None else None, Cout, k, s, p)
    if cx.record:
        def bwd():
            dy = cx.take(y)
            if dy is None:
                return
            dx, acc = cx.dest(x)
            ops.conv_transpose_bwd(dy, x, wp, cx.pgrad(w), cx.pgrad(b), k, s, p, dx, acc)
            cx.done(w, b)
        cx.push(bwd)
    return y


def add_classes(cx, a, b):
    """a + b of two class-logit tensors (models/FCN.py:57,60 of the reference); rows zero padded to the same stride"""
    K = a.shape[-1]
    yw = ops.add_n_act([ops.widen(a), ops.widen(b)], False)
    y = yw[..., :K]
    if cx.record:
        def bwd():
            dy = cx.take(y)
            if dy is not None:
                cx.give(a, dy, shared=True)
                cx.give(b, dy, shared=True)
        cx.push(bwd)
    return y


def add_n(cx, terms, relu=True):
    """y = act(sum(terms)) — the HRNet fuse (models/HRNetv2.py:237-261); terms share one shape"""
    y = ops.add_n_act(terms, relu)
    if cx.record:
        def bwd():
            dy = cx.take(y)
            if dy is None:
                return
            g = ops.relu_bwd(dy, y) if relu else dy
            for t in terms:
                cx.give(t, g, shared=len(terms) > 1)
        cx.push(bwd)
    return y


def maxpool(cx, x):
    y, idx = ops.maxpool_fwd(x)
    if cx.record:
        def bwd():
            dy = cx.take(y)
            if dy is not None:
                cx.give(x, ops.maxpool_bwd(dy, idx, tuple(x.shape)))
        cx.push(bwd)
    return y


def bilinear_backward_of(cx, x, y, align_corners):
    """tape entry of y = bilinear(x): the gradient of y, resized back, goes to x"""
    if cx.record:
        def bwd():
            dy = cx.take(y)
            if dy is None:
                return
            dx, acc = cx.dest(x)
            C = x.shape[-1]
            ops.bilinear_bwd(dy, tuple(x.shape), align_corners, out=dx, zero_to=(ops.ld_of(dx) if ops.ld_of(dx) != C else 0),
                             accumulate=acc)
        cx.push(bwd)


def bilinear(cx, x, Ho, Wo, align_corners, out=None):
    y = ops.bilinear_fwd(x, Ho, Wo, align_corners, out=out)
    bilinear_backward_of(cx, x, y, align_corners)
    return y


def adaptive_avgpool(cx, x, S):
    """nn.AdaptiveAvgPool2d(S) -> [B, S, S, C]"""
    y = ops.adaptive_avgpool_fwd(x, S)
    if cx.record:
        def bwd():
            dy = cx.take(y)
            if dy is None:
                return
            dx, acc = cx.dest(x)
            ops.adaptive_avgpool_bwd(dy, dx, S, acc)
        cx.push(bwd)
    return y


def copy_into(cx, src, dst):
    """dst (a channel slice of a concat buffer) = src; the gradient of dst flows back to src"""
    rec = ops.amax_of(src)
    ops.axpy(src, dst, 1.0, False)
    if rec is not None:
        dst._amax = rec                 # (a copy: the source's record bounds it)
    if cx.record:
        def bwd():
            g = cx.take(dst)
            if g is not None:
                cx.give(src, g)
        cx.push(bwd)
    return dst


def global_avgpool(cx, x):
    y = ops.global_avgpool_fwd(x)
    if cx.record:
        def bwd():
            dy = cx.take(y)
            if dy is None:
                return
            dx, acc = cx.dest(x)
            ops.global_avgpool_bwd(dy, dx, acc)
        cx.push(bwd)
    return y


def concat_views(cx, cat, parts):
    """parts: [(tensor written as a channel slice of `cat`, c0, c1)] — backward hands out slices."""
    recs = [ops.amax_of(t) for t, _, _ in parts]
    if recs and all(r is not None for r in recs) and sum(c1 - c0 for _, c0, c1 in parts) == cat.shape[-1]:
        cat._amax_parts = recs          # every channel of the buffer has a producer that left max|.|: the f16x2 split pass needs no amax pass
    if cx.record:
        def bwd():
            dcat = cx.take(cat)
            if dcat is None:
                return
            for t, c0, c1 in parts:
                cx.give(t, dcat[..., c0:c1])
        cx.push(bwd)
    return cat


def pointrend_refine(cx, seg, feats, head, k0, steps):
    """models/PointRend.py:74-90 of the reference, the eval-mode refinement loop (ops.pointrend_refine).  Forward only: nothing differentiates
    through the point branch, so a training or recorded pass is refused"""
    if cx.train or cx.record:
        raise NotImplementedError("the PointRend refinement runs in eval mode only: its train-mode forward (random point sampling, point loss) "
                                  "and the backward of the point gather are not on the accelerated path")
    return ops.pointrend_refine(seg, feats, head, k0, steps)


def pointrend_sample_points(coarse, sampler, P, ratio, beta, h, w):
    """utils/pointrend_utils.py:86-116 and models/PointRend.py:54-57 of the reference on the device: M = int(P ratio) uniform candidates,
    the uncertainty of the coarse logits sampled there, the int(beta P) most uncertain of them, P - int(beta P) fresh uniform points; per
    point its pixel of the h x w map.  -> (coords [N, P, 2], pix int32 [N, P]).  Nothing differentiates through this."""
    if not (ratio >= 1 and 0 <= beta <= 1):
        raise ValueError("PointRend: pr_oversample_ratio >= 1 and 0 <= pr_importance_sample_ratio <= 1 (got %s, %s)" % (ratio, beta))
    N = coarse.shape[0]
    if sampler.fixed_points is not None:
        pts = sampler.fixed_points.to(device=coarse.device, dtype=torch.float32).contiguous()
        if tuple(pts.shape) != (N, P, 2):
            raise ValueError("PointSampler.fixed_points must be [%d, %d, 2], got %s" % (N, P, tuple(pts.shape)))
        coords, pix, _ = ops.pointrend_compose(None, None, ops.pointrend_draw(None, N, P, fixed=pts), h, w)
        return coords, pix
    sampler.ensure_seeded()
    M, kb = int(P * ratio), int(beta * P)
    cand = sel = rest = None
    if kb > 0:
        cand = ops.pointrend_draw(sampler.state, N, M)
        sel = ops.pointrend_topk(ops.pointrend_point_uncertainty(coarse, cand), kb)
    if P - kb > 0:
        rest = ops.pointrend_draw(sampler.state, N, P - kb)
    coords, pix, _ = ops.pointrend_compose(cand, sel, rest, h, w)
    return coords, pix


def pointrend_train(cx, coarse, feats, head, sampler, P, ratio, beta, scale):
    """models/PointRend.py:43-73 of the reference, the train-mode forward.  coarse: UPerNet's logits NHWC [N, h, w, K] (padded rows); feats:
    the encoder stages NHWC, shallow to deep; head: the StandardPointHead module; sampler: an engine.PointSampler.
    -> (coords [N, P, 1, 2], point_logits [N, P, 1, K] (a view of rows K rounded up to 4 floats wide), pred [N, s h, s w, K]): pred IS the
    interpolated coarse logits with the point logits scattered in place (seg_logits and pred of the reference are one memory; among points
    on one pixel the last writes).
    Backward (one tape entry): the scatter (every point, duplicates too, receives its pixel's gradient; the interpolation receives zero
    there), the interpolation, the predictor and the fc layers with their ReLUs as GEMMs over the N P point rows (weight gradients straight
    into p.grad [O, I, 1]: the zero pad columns of the weight images never leave this function; the coarse block's gradient summed over
    every layer that concatenates it), and the deterministic adjoint of the point gather into the four stages and the coarse logits."""
    N, hc, wc, K = coarse.shape
    if K < 2:
        raise ValueError("PointRend's uncertainty is the difference of the two largest logits: it needs at least 2 classes (got %d)" % K)
    Kq = (K + 3) // 4 * 4
    srcs = list(feats[::-1])
    if any(f.shape[-1] % 4 for f in srcs):
        raise ValueError("PointRend: the encoder stages' channel counts must be multiples of 4 (got %s)" % [f.shape[-1] for f in feats])
    Cf = sum(f.shape[-1] for f in srcs)
    layers = list(head.fc_layers) + [head.predictor]
    widths = [m.out_channels for m in head.fc_layers]
    if any(o % 4 for o in widths):
        raise ValueError("PointRend: ph_fc_dim must be a multiple of 4 (got %s)" % widths)
    each = bool(head.coarse_pred_each_layer)
    for m in layers:
        cx.claim(m.weight, m.bias)
    h, w = hc * scale, wc * scale
    dev = coarse.device
    with torch.no_grad():
        coords, pix = pointrend_sample_points(coarse, sampler, P, ratio, beta, h, w)
    rows = N * P
    # the inputs of the layers: [c5 | c4 | c3 | c2 | coarse] for fc1, [relu(fc_i) | coarse] (or relu(fc_i) alone) behind it
    mains = [Cf] + widths                                  # width of each layer's input in front of its coarse block
    blocks = [Kq] + [Kq if each else 0] * len(widths)      # ... and of the coarse block
    xs = [torch.empty((rows, m + b), dtype=torch.float32, device=dev) for m, b in zip(mains, blocks)]
    ops.pointrend_gather_at(srcs + [coarse], coords, out=xs[0], extras=[(x, m) for x, m, b in zip(xs[1:], mains[1:], blocks[1:]) if b])
    # (weight images with the coarse block's columns padded to Kq, rebuilt every step: the optimiser writes the parameters in place)
    imgs = [ops._pointrend_weight(m.weight.data, mn, K if b else 0) for m, mn, b in zip(layers, mains, blocks)]
    for li, o in enumerate(widths):
        ops.conv_fwd_fused(xs[li].view(1, 1, rows, -1), imgs[li], layers[li].bias.data, None, True, o, 1, 1, out=xs[li + 1].view(1, 1, rows, -1)[..., :o])
    pl = ops.conv_fwd(xs[-1].view(1, 1, rows, -1), imgs[-1], head.predictor.bias.data, K, 1, 1, zero_to=Kq)      # (rows Kq floats apart)
    prow = torch.as_strided(pl, (rows, K), (Kq, 1))
    pl = torch.as_strided(pl, (N, P, 1, K), (P * Kq, Kq, Kq, 1))
    pred = ops.bilinear_fwd(coarse, h, w, False)
    ops.pointrend_scatter_last(prow, pix, pred)
    coords4 = coords.view(N, P, 1, 2)
    cx.nondiff.add(id(coords4))
    if cx.record:
        def bwd():
            dpl, dpred = cx.take(pl), cx.take(pred)
            cx.take(coords4)
            if dpl is None and dpred is None:
                return
            dp = torch.zeros((rows, Kq), dtype=torch.float32, device=dev)      # (the pad columns stay zero: they meet the images' zero columns)
            if dpl is not None:
                dp[:, :K].copy_(dpl.reshape(rows, K))
            if dpred is not None:
                ops.pointrend_scatter_bwd(dpred, pix, dp, True)                # dpred is zero at the scattered pixels from here on
                dc, acc = cx.dest(coarse)
                ops.bilinear_bwd(dpred, tuple(coarse.shape), False, out=dc, zero_to=(ops.ld_of(dc) if ops.ld_of(dc) != K else 0), accumulate=acc)
            dy, dx0, coarse_terms = dp, None, []
            for li in range(len(layers) - 1, -1, -1):
                m, x, mn, b = layers[li], xs[li], mains[li], blocks[li]
                O, real = m.out_channels, mn + (K if b else 0)                 # the parameter's input width: no pad column
                ops.gemm(ops.TN, 1, O, real, rows, dy, dy.stride(0), 0, x, x.stride(0), 0, cx.pgrad(m.weight).view(O, real), real, 0)
                ops.bias_grad(dy, O, cx.pgrad(m.bias))
                dx = torch.empty_like(x)
                ops.gemm(ops.NN, 1, rows, mn + b, O, dy, dy.stride(0), 0, imgs[li], imgs[li].stride(0), 0, dx, dx.stride(0), 0)
                cx.done(m.weight, m.bias)
                if li == 0:
                    dx0 = dx
                else:
                    if b:
                        coarse_terms.append(dx[:, mn:])
                    dy = ops.relu_bwd(dx[:, :mn], x[:, :mn])
            for t in coarse_terms:
                ops.axpy(t, dx0[:, Cf:], 1.0, True)
            ops.pointrend_gather_bwd(dx0, coords, [cx.dest(t) for t in srcs + [coarse]])
        cx.push(bwd)
    return coords4, pl, pred


def spatial_gather(cx, feats, logits, K):
    """models/OCR.py:158-170: proxy[b, k, :] = sum_n softmax_n(logits[b, n, k]) * feats[b, n, :]"""
    B, H, W, C = feats.shape
    N = H * W
    ldl = ops.ld_of(logits)
    lbuf = torch.as_strided(logits, (B, N, ldl), (N * ldl, ldl, 1))
    probs = ops.softmax_spatial_fwd(lbuf, K)
    proxy = torch.empty((B, K, 1, C), dtype=torch.float32, device=feats.device)
    ldf = ops.ld_of(feats)
    ops.gemm_tn_split(B, K, C, N, probs, ldl, feats, ldf, proxy)
    if cx.record:
        def bwd():
            dproxy = cx.take(proxy)
            if dproxy is None:
                return
            dfe, acc = cx.dest(feats)
            ops.gemm(ops.NN, B, N, C, K, probs, ldl, N * ldl, dproxy, C, K * C, dfe, ops.ld_of(dfe), N * ops.ld_of(dfe),
                     accumulate=acc)
            dprobs = torch.empty_like(probs)
            ops.gemm(ops.NT, B, N, K, C, feats, ldf, N * ldf, dproxy, C, K * C, dprobs, ldl, N * ldl, zero_to=ldl)
            dlg, accl = cx.dest(logits)
            dbuf = torch.as_strided(dlg, (B, N, ldl), (N * ldl, ldl, 1))
            ops.softmax_spatial_bwd(probs, dprobs, dbuf, K, accumulate=accl)
        cx.push(bwd)
    return proxy


def object_attention_core(cx, q, key, val, K, key_channels):
    """models/OCR.py:266-274: softmax_k(C^-0.5 q.key) . val   (q [B,H,W,Ck]; key, val [B,K,1,Ck])"""
    B, H, W, Ck = q.shape
    N = H * W
    ld = 32 if K <= 32 else 64
    scale = float(key_channels) ** -0.5
    sim = torch.empty((B, N, ld), dtype=torch.float32, device=q.device)
    ops.gemm(ops.NT, B, N, K, Ck, q, Ck, N * Ck, key, Ck, K * Ck, sim, ld, N * ld, zero_to=ld)
    p = ops.softmax_rows_fwd(sim.view(B * N, ld), K, scale)
    del sim
    ctx = torch.empty((B, H, W, Ck), dtype=torch.float32, device=q.device)
    ops.gemm(ops.NN, B, N, Ck, K, p, ld, N * ld, val, Ck, K * Ck, ctx, Ck, N * Ck)
    if ops.amax_of(val) is not None:
        ctx._amax = ops.amax_of(val)    # every row of ctx is a convex combination of val's rows (softmax weights): max|ctx| <= max|val|
    if cx.record:
        def bwd():
            dctx = cx.take(ctx)
            if dctx is None:
                return
            dp = torch.empty_like(p)
            ops.gemm(ops.NT, B, N, K, Ck, dctx, Ck, N * Ck, val, Ck, K * Ck, dp, ld, N * ld, zero_to=ld)
            dv, accv = cx.dest(val)
            ops.gemm_tn_split(B, K, Ck, N, p, ld, dctx, Ck, dv, accumulate=accv)
            dsim = ops.softmax_rows_bwd(p, dp, K, scale)
            dq, accq = cx.dest(q)
            ops.gemm(ops.NN, B, N, Ck, K, dsim, ld, N * ld, key, Ck, K * Ck, dq, Ck, N * Ck, accumulate=accq)
            dk, acck = cx.dest(key)
            ops.gemm_tn_split(B, K, Ck, N, dsim, ld, q, Ck, dk, accumulate=acck)
        cx.push(bwd)
    return ctx


# --------------------------------------------------------------------------- autograd bridge
class NetFunction(torch.autograd.Function):
    """One autograd node for a whole network.  Parameter gradients are written directly into the
    flat gradient buffer by the tape; autograd only carries the output gradients in."""

    @staticmethod
    def forward(ctx, net, x, anchor):
        cx, outs = net._run(x, record=True)
        ctx.cx = cx
        ctx.net = net
        ctx.outs_nhwc = outs
        if net._keep_pass:
            net._last_pass = (cx, outs)
        res = tuple(o.permute(0, 3, 1, 2) for o in outs)
        ctx.mark_non_differentiable(*[r for o, r in zip(outs, res) if id(o) in cx.nondiff])
        return res if len(res) > 1 else res[0]

    @staticmethod
    def backward(ctx, *gouts):
        ctx.net._tape_backward(ctx.cx, ctx.outs_nhwc, gouts)
        return None, None, None


class EngineNet(nn.Module):
    """Base class of the HIP-engine networks (keeps the reference's ``Model(config, experiment)``
    / ``model(x)`` surface).  Subclasses implement ``_body(cx, x_nchw) -> [NHWC outputs]``."""

    def __init__(self):
        super().__init__()
        self._flatp = None
        self._grad_sync = None  # optional data-parallel gradient reducer
        self._grads_pending = False
        self._keep_pass = False  # graph.GraphedTrainStep (segmented capture): keep the recorded pass for backward_from()
        self._last_pass = self._last_outputs = None
        self._open_state = None  # weak reference to the state of the last recorded pass (dead once its Ctx is gone)

    def apply_freeze_bn(self, config):
        """config['freeze_bn'] (build-side key of the graph section; the values of freeze_bn's `select`), applied at the end of construction"""
        self.frozen_bn = freeze_bn(self, config.get("freeze_bn"))

    def flat(self):
        if self._flatp is None:
            self._flatp = FlatParams(self)
        return self._flatp.ensure()

    def state_dict(self, *a, **k):
        flush_bn_counters(self)
        return super().state_dict(*a, **k)

    def weight_images(self):
        """the network's bank of weight images (weight_images.WeightImages): every direct 3x3, pointwise and gather layer behind the stem"""
        fp = self.flat()
        bank = getattr(self, "_wimages", None)
        if bank is None or bank.stale(fp.flat):
            convs = [m for m in self.modules() if isinstance(m, Conv2d) and not m.stem]
            bank = self._wimages = WeightImages(fp.flat, network_layers(fp, convs))
        return bank

    def _run(self, x, record):
        stale = self._open_state() if self._open_state is not None else None
        if stale is not None:
            stale.release()             # (planes left over from this network's last recorded forward if it never saw its backward)
        # what the pass caches between its launches -- split planes, weight images made in line, which images of the network's bank are its
        # own (the bank's buffers stay: a captured step replays into them) -- is the pass's own: its Ctx holds it, current while the pass runs
        cx = Ctx(self.training, record, None)
        bank = self.weight_images()
        cx.state = ops.PassState(bank)
        self._open_state = weakref.ref(cx.state) if record else None
        ops.set_state(cx.state)
        # The per-step weight images (direct 3x3 kernels: 459 MB written for OCRNet-HRNet-W48, 0.43 ms; pointwise / gather kernels) are not
        # needed before stage 2: their launches run on a side stream beside the stem and stage 1; the launch stream waits for them at the
        # first lookup of an image or in front of the first parallel region (ops.images_ready).  Only while the step is being RECORDED into a
        # hipGraph (replay: 109.1 / 109.2 / 109.7 -> 108.5 / 109.2 / 109.0 ms): in the eager launch loop one more live stream shifts the runtime's
        # round-robin of streams over its four hardware queues, two branch streams of the parallel regions then share a queue and the step
        # LOSES 3 - 5 ms (116.4 / 119.5 against 113.5 / 114.3 ms; per-branch region times 1.9 / 2.7 / 2.7 / 2.7 instead of 2.2 / 2.3 / 2.0 / 2.3 ms).
        # PREP_ASYNC = False: in line everywhere.  (The head layers' images join on the side stream only, else they are made at their GEMMs.)
        aside = bool(PREP_ASYNC and x.is_cuda and torch.cuda.is_current_stream_capturing())
        due = bank.due(self.training, with_heads=aside)
        if due and aside:
            main = torch.cuda.current_stream(x.device)
            side = prep_stream(x.device)
            side.wait_stream(main)          # (behind the optimiser's update of the weights and the last readers of the old images)
            with torch.cuda.stream(side):
                bank.refresh(due)
                ev = torch.cuda.Event()
                ev.record(side)
            ops.images_pending(ev, main)
        elif due:
            bank.refresh(due)
        if ops._trunk_h2() and self.training:
            # the per-tensor amax records of this forward pass and of its backward: ONE chunk, zeroed here on the main stream, sized from
            # the previous pass of this network (+25 %: a rollover inside a parallel region would have to be ordered against its siblings)
            cx.amax_scope = ops.AmaxScope(x.device, max(ops.AMAX_SCOPE_RECORDS, int(1.25 * getattr(self, "_amax_records", 0)) + 64))
            cx.state.amax_scope = cx.amax_scope
        global _cur_cx
        _cur_cx = cx
        try:
            outs = self._body(cx, x)
        finally:
            _cur_cx = None
            ops.images_ready()          # (a pass that looked no image up -- small maps stay on the fp32 kernels -- still joins the prep stream)
            ops.set_state(None)
        if not record:
            cx.state.release()          # a recorded forward keeps its split planes for the backward-weight pass (_end_backward frees them)
        return cx, outs

    def zero_grad(self, set_to_none=True):
        """clears the flat gradient buffer (one memset; the .grad views stay bound to it)"""
        fp = self.flat()
        if fp.grad is not None:
            fp.grad.zero_()
        self._grads_pending = False

    def _begin_backward(self, cx):
        fp = self.flat()
        if self._grads_pending:
            detached = sum(1 for p in fp.params if p.grad is None)
            if detached == len(fp.params) or detached > 0:
                # optimiser.zero_grad(set_to_none=True) of a stock torch optimiser (torch.optim.Adam(model.parameters()) in the reference's
                # loop, managers/OCRNet_Manager.py:80-90) detached every .grad: that IS the zero_grad between two backward passes.  An
                # optimiser over a SUBSET of the parameters detaches only its own: the others' gradients are read by nobody (torch would
                # accumulate them unseen; the tape overwrites them), so a partly detached set counts as cleared as well.
                fp.grad.zero_()
                self._grads_pending = False
            elif not bool(fp.grad.any()):
                # zero_grad(set_to_none=False): the .grad views were zeroed in place, i.e. the flat buffer is all zero (checked on this
                # rare path only: one reduction + a host synchronisation)
                self._grads_pending = False
            else:
                raise RuntimeError("second backward() before zero_grad(): the HIP engine's tape overwrites parameter gradients "
                                   "(no accumulation over several backward passes); call optimiser.zero_grad() / model.zero_grad() "
                                   "between backward passes")
        fp.bind_grads()
        ops.set_state(cx.state)         # (another forward pass may have run since this one: planes, images and amax records are this pass's own)
        if self._grad_sync is not None:
            cx.on_param_grad = self._grad_sync.param_ready
            cx.on_quiet = getattr(self._grad_sync, "quiet_point", None)
            self._grad_sync.begin(fp)

    def _tape_backward(self, cx, outs_nhwc, gouts):
        """the backward pass of a recorded forward: hands the output gradients (NCHW, as autograd carries them) to the tape and pops it"""
        for o, g in zip(outs_nhwc, gouts):
            if g is None or id(o) in cx.nondiff:
                continue
            gn = g.permute(0, 2, 3, 1)
            if not gn.is_contiguous():
                gn = gn.contiguous()
            cx.give(o, gn)
        self._begin_backward(cx)
        cx.backward()
        self._end_backward(cx)

    def backward_from(self, gouts):
        """runs the tape of the last recorded forward pass ON THE CALLING THREAD from the gradients of its outputs (one per output of
        forward(), None allowed) -- what NetFunction.backward does inside autograd's device thread.  graph.GraphedTrainStep drives the
        backward pass this way when it cuts the captured step into segments: a stream capture has to end on the thread that began it.
        Needs `_keep_pass` set before the forward."""
        if self._last_pass is None:
            raise RuntimeError("backward_from(): no recorded forward pass is kept (set model._keep_pass = True before the forward)")
        (cx, outs), self._last_pass, self._last_outputs = self._last_pass, None, None
        self._tape_backward(cx, outs, gouts)

    def _end_backward(self, cx):
        if getattr(cx, "amax_scope", None) is not None:
            self._amax_records = max(getattr(self, "_amax_records", 0), cx.amax_scope.used)
        cx.state.release()
        ops.set_state(None)
        self._grads_pending = True
        if self._grad_sync is not None:
            self._grad_sync.finish()

    def forward(self, x):
        if not x.is_cuda:
            raise RuntimeError("the HIP engine only runs on an MI355X device tensor (no CPU fallback)")
        fp = self.flat()
        x = x.contiguous().float()
        if torch.is_grad_enabled() and self.training and any(p.requires_grad for p in fp.params):
            res = NetFunction.apply(self, x, fp.params[0])
            if self._keep_pass:
                self._last_outputs = res if isinstance(res, tuple) else (res,)
            return res
        _, outs = self._run(x, record=False)
        res = tuple(o.permute(0, 3, 1, 2) for o in outs)
        return res if len(res) > 1 else res[0]
