"""Tensor-level wrappers over the C ABI (include/catseg.h).

Activations are NHWC fp32 torch tensors of shape [B, H, W, C] whose last dim is
contiguous and whose pixel stride ``ld = t.stride(2)`` may exceed C (a view into
a wider concat buffer).  Conv weights are [O, I, kh, kw] tensors in
channels_last memory format (physical OHWI).  Nothing here touches autograd.
"""
import collections
import ctypes

import numpy as np
import torch

from . import _lib
from . import plan as _plan
from . import weight_images as _wi
from ._lib import (BnApplyDesc, BnBackwardDesc, ConvBwdDataDesc, ConvBwdWeightDesc, ConvDesc, ConvFwdDesc, OPERANDS_BF16X3, OPERANDS_BF16X3_BLOCKED,
                   OPERANDS_F16X2, OPERANDS_F16X2_BLOCKED, OPERANDS_F32, check, lib, ptr, stream)

_ws = {}


def workspace(nbytes, device):
    """Grow-only scratch buffer per (device, stream): launches on one stream are ordered; parallel-branch regions
    (engine.Ctx.parallel) run on side streams, each with its own scratch"""
    key = (device.type, device.index, torch.cuda.current_stream(device).cuda_stream if device.type == "cuda" else 0)
    buf = _ws.get(key)
    if buf is None or buf.numel() < nbytes:
        buf = torch.empty(max(int(nbytes), 1 << 20), dtype=torch.uint8, device=device)
        _ws[key] = buf
    return buf


def release_workspaces():
    _ws.clear()


def new_act(B, H, W, C, device, ld=None, zero=False):
    """NHWC activation; ld (pixel stride) defaults to C rounded up to 4."""
    ld = ld or ((C + 3) // 4 * 4)
    buf = (torch.zeros if zero else torch.empty)((B, H, W, ld), dtype=torch.float32, device=device)
    return buf[..., :C] if ld != C else buf


def ld_of(t):
    """pixel stride of an NHWC tensor; the stride torch reports for a size-1 dimension is arbitrary, so it is
    taken from the innermost pixel dimension that has more than one entry"""
    if t.dim() < 2:
        return t.shape[-1]
    inner = 1
    for dim in range(t.dim() - 2, -1, -1):
        if t.shape[dim] > 1:
            return t.stride(dim) // inner
        inner *= t.shape[dim]
    return (t.shape[-1] + 3) // 4 * 4


def rows_of(t):
    n = 1
    for s in t.shape[:-1]:
        n *= s
    return n


def conv_out_size(n, k, s, p, d):
    return (n + 2 * p - d * (k - 1) - 1) // s + 1


def make_desc(xshape, ldx, Cout, ldy, kh, kw, stride, pad, dil, stem4=False, groups=1):
    B, H, W, Cin = xshape
    return ConvDesc(B, H, W, Cin, conv_out_size(H, kh, stride, pad, dil), conv_out_size(W, kw, stride, pad, dil), Cout,
                    kh, kw, stride, pad, dil, ldx, ldy, 1 if stem4 else 0, groups)


PROFILE = None  # bench.py sets this to a list: every implicit-GEMM launch is bracketed by HIP events

# roctx ranges: CATSEG_ROCTX=1 brackets every timed C-ABI call with roctxRangePush(kind) / roctxRangePop(), so that a
# `rocprofv3 --marker-trace --kernel-trace` timeline shows which layer operation a kernel belongs to.  Off by default (two ctypes calls per launch).
_roctx = None
if __import__("os").environ.get("CATSEG_ROCTX", "0") == "1":      # (a profiling aid, not a route: roctx ranges around every C-ABI call)
    for _name in ("librocprofiler-sdk-roctx.so", "libroctx64.so"):
        try:
            _roctx = ctypes.CDLL(_name)
            _roctx.roctxRangePushA.argtypes = [ctypes.c_char_p]
            break
        except (OSError, AttributeError):
            _roctx = None


class _Timed:
    """HIP events on the launch stream around one C-ABI call (algorithmic FLOPs = 2*M*N*K)."""

    def __init__(self, kind, flops):
        self.kind, self.flops = kind, flops

    def __enter__(self):
        if _roctx is not None:
            _roctx.roctxRangePushA(self.kind.encode())
        if PROFILE is not None:
            self.e0 = torch.cuda.Event(enable_timing=True)
            self.e1 = torch.cuda.Event(enable_timing=True)
            self.e0.record()

    def __exit__(self, *a):
        if PROFILE is not None:
            self.e1.record()
            PROFILE.append((self.kind, self.flops, self.e0, self.e1))
        if _roctx is not None:
            _roctx.roctxRangePop()


# Arithmetic of the large convolutions: "fp32" = v_mfma_f32_32x32x2_f32 (an exact fp32 FMA chain), "bf16x3" = every fp32
# operand split exactly into three bf16 planes, six bf16 MFMA partial products per block, fp32 accumulate (csrc/igemm_bf16x3.hip:
# error vs an fp64 reference equal to or below the fp32 kernel's, 1.45-1.6x its speed on the layers it takes).  Which kernel family
# runs a layer is decided in ONE place, the route planner below (fwd_route / dgrad_route / wgrad_route); the thresholds it reads are the
# module attributes of this file.  CATSEG_PRECISION=fp32 selects the exact fp32 path everywhere.
PRECISION = _plan.get("precision")
# thresholds of the layer selection (tests lower them to push small layers through the split-precision kernels)
B3_MIN_TAPS, B3_MIN_K, B3_MIN_N, B3_MIN_TILES = 2, 2048, 192, 192
B3_OPS = ("fwd", "dgrad", "wgrad")
B3_MIN_WGRAD_ROWS = 32768


# wide 1x1 layers (the 1024 -> 512 bottleneck of the OCR head at stride 4): both GEMM extents >= 512, their product >= 512 * 1024,
# >= 131072 pixels -- there the split pass (one read + 1.5 writes of the activation) is paid back (tools/bench_b3.py: forward
# 2.38 -> 1.54 + 0.57 ms, backward-data 2.42 -> 1.80 + 0.30 ms at 8 x 136 x 240); smaller 1x1 layers stay on the fp32 kernels
# Round 3, with two fp16 planes and three products: the 1x1 layers of a ResNet50's layer 4 at stride 8 (2048 <-> 512 on 8 x 68 x 120 = 65 280
# pixels) pay as well -- OCRNet-R50 step 98.8 -> 87.5 ms (tools/ab_1x1_rows.py); smaller extents (256) still do not (87.6 -> 88.5 ms)
B3_1X1_MIN_DIM = _plan.get("wide_1x1_min_dim")
B3_1X1_MIN_PROD, B3_1X1_MIN_ROWS = B3_1X1_MIN_DIM * 1024, _plan.get("wide_1x1_min_rows")


def _b3_wide_1x1(rows, ncols, taps, cred):
    return taps == 1 and min(cred, ncols) >= B3_1X1_MIN_DIM and cred * ncols >= B3_1X1_MIN_PROD and rows >= B3_1X1_MIN_ROWS


B3_INDEX_LIMIT = 1 << 31     # the planar bf16x3 kernels index their operand planes with 32-bit element offsets


def _b3_eligible(rows, ncols, taps, cred, stride_ok=True):
    if not (PRECISION == "bf16x3" and stride_ok and taps <= 32 and cred % 8 == 0):
        return False
    if rows * cred >= B3_INDEX_LIMIT or ncols * taps * cred >= B3_INDEX_LIMIT:      # oversized operands: the fp32 kernels (64-bit addressing)
        return False
    if (B3_MIN_TAPS <= taps and taps * cred >= B3_MIN_K and ncols >= B3_MIN_N
            and ((rows + 255) // 256) * ((ncols + 255) // 256) >= B3_MIN_TILES):
        return True
    return _b3_wide_1x1(rows, ncols, taps, cred)


# Layers that run the 256 x 256 register-pipelined kernel (> 192 output columns) read BLOCKED planes in forward / backward-data
# (csrc/igemm_bf16x3.hip: whole cache lines per LDS-DMA instruction, 190 -> 248 TFLOP/s-equivalent on the 3x3 720 -> 512 layer);
# the backward-weight kernel keeps the planar planes, written by the same split pass when a backward will follow.
B3_BLOCKED = True
B3_PLANE_LIMIT = (1 << 32) - 64     # bytes of the three blocked planes of one operand (one 32-bit-offset buffer resource); tests lower it


def _b3_blocked_shape(ncols, cred):
    """the layer's extents suit the 256 x 256 kernel on blocked planes; cred: channels of the gathered operand (a multiple of 16)"""
    return B3_BLOCKED and ncols > 192 and cred % 16 == 0


def _b3_blocked_ok(ncols, cred, a_rows, w_rows, taps):
    """... and the three planes of an operand stay below 4 GB (the kernel addresses them through one 32-bit-offset buffer resource)"""
    return (_b3_blocked_shape(ncols, cred) and 6 * a_rows * cred < B3_PLANE_LIMIT
            and 6 * w_rows * taps * cred < B3_PLANE_LIMIT)


# Arithmetic of the layers on the blocked 256 x 256 path (forward / backward-data of the head convolutions): "f16x2" = two fp16 planes
# per operand after a per-tensor power-of-two prescale, three MFMA products (csrc/igemm_f16x2.hip: 22 significant bits per operand,
# half the matrix work of bf16x3); "bf16x3" = three exact bf16 planes, six products.  CATSEG_HEADS selects.
HEADS = _plan.get("heads")


def _h2():
    return HEADS == "f16x2"


# Backward-weight of the f16x2 layers from the BLOCKED planes its forward / backward-data read (csrc/igemm_f16x2.hip: igemm_h2t_kernel's
# blocked mode): one plane set per tensor, the split passes write half as much.  CATSEG_H2T=planar: the separate planar set of round 3.
H2T_BLOCKED = _plan.get("h2t") != "planar"


# launch-shape knobs of the library's debug interface (include/catseg_debug.h) as plan fields, so that a whole bench process can run under
# another setting (tools/ab_env_bench.sh).  0 = the library's default.
for _field, _setter in _plan.LIBRARY_KNOBS.items():
    if _plan.get(_field):
        getattr(lib, _setter)(int(_plan.get(_field)))


def plan():
    """the active execution plan: every route / threshold switch of the host layer with its live value (plan.FIELDS documents them);
    bench.py prints it as `config.plan`"""
    return _plan.active()


def _split3_any(x, want, both):
    """(planar, blocked) planes of x, at least the wanted one; `both`: produce the two layouts in ONE pass over x"""
    if want == "blk" or both:
        blk, planar = split3_blocked(x, with_planar=(want == "planar" or both))
        return planar, blk
    return split3(x), None


def _cached(cache, x, key, want, both):
    """want: "planar" / "blk" (bf16 x 3 planes), or "h2" / "h2p" ((fp16 x 2 planes in the blocked / planar layout, device scale record));
    both: on a miss produce the sibling layout in the same pass over x"""
    hit = cache["key"] == key and cache["x"] is x
    if not hit:
        cache.update(key=key, x=x, planar=None, blk=None, h2=None, h2p=None)
    if cache.get(want) is None:
        _refuse_h2_only(x, "a split pass (%s planes)" % want)
        if want in ("h2", "h2p"):
            blk, pl, sc = split2h(x, blocked=(want == "h2" or both), planar=(want == "h2p" or both))
            if blk is not None:
                cache["h2"] = (blk, sc)
            if pl is not None:
                cache["h2p"] = (pl, sc)
        else:
            planar, blk = _split3_any(x, want, both and not hit)
            if planar is not None:
                cache["planar"] = planar
            if blk is not None:
                cache["blk"] = blk
    return cache[want]


def _no_planes():
    return {"key": None, "x": None, "planar": None, "blk": None, "h2": None, "h2p": None}


class PassState:
    """what ONE pass (a forward and its backward) caches between its launches: the split planes of its activations and the images of its
    weights.  engine.EngineNet._run creates one per pass, keeps it on the pass's Ctx and makes it current (set_state) for the forward and
    again for the backward, so that passes of several networks in flight never see, overwrite or release each other's operands; callers
    outside the engine (tests, tools) work on the module's default instance."""

    def __init__(self, bank=None):
        self.last, self.last_dy = _no_planes(), _no_planes()    # planes of the last split activation / output gradient
        self.kept = {}          # recorded forward: planes of every split input, kept for the layer's backward-weight pass
        self.inline = {}        # weight images made in line during the pass (weight_images.weight_image: key -> image)
        self.bank = bank        # the network's bank of weight images (weight_images.WeightImages: its buffers outlive the pass), or None
        self.refreshed = {}     # family -> entries of the bank its refresh wrote for THIS pass (only those are this pass's images)
        self.images_event = None    # (event, origin stream): the pass's weight images are being written on a side stream
        self.amax_scope = None      # the AmaxScope new_amax() draws from

    def release(self):
        """drops the planes and images (the memory of a finished pass); the bank's images are no longer those of a running step"""
        self.last, self.last_dy = _no_planes(), _no_planes()
        self.kept.clear()
        self.inline.clear()
        self.refreshed = {}


_default_state = _state = PassState()


def set_state(st):
    """the state the cached operand functions below read and write; None: the default one"""
    global _state
    _state = _default_state if st is None else st


def _split3_cached(x, want="planar", both=False, keep=False):
    """three-plane split of an activation.  The last one is always kept (the two 720-channel head convolutions of OCRNet-HRNet and
    the ASPP branches read one tensor); keep=True (a recorded training forward) holds on to the planes until the pass's state is released,
    so that the layer's backward-weight pass reads what its forward produced instead of splitting x again (the planes of all
    bf16x3 layers of a step: 5.5 GB for OCRNet-HRNet-W48 at bs 8, of 288 GB)"""
    # (per stream: since round 5 a branch output may be read by fuse chains on SEVERAL branch streams -- each splits for itself; planes made
    #  on one stream are never read on another without an ordering event)
    hp = getattr(x, "_h2_planes", None)
    if hp is not None:          # a tensor that exists only as blocked f16x2 planes (register_h2_planes): they travel with it
        if want == "h2":
            return hp
        _refuse_h2_only(x, "a split pass (%s planes)" % want)
    key = (x.data_ptr(), x._version, tuple(x.shape), ld_of(x), torch.cuda.current_stream(x.device).cuda_stream if x.is_cuda else 0)
    ent = _state.kept.get(key)
    if ent is not None and ent["x"] is x:
        return _cached(ent, x, key, want, both)
    if keep:
        ent = _state.kept[key] = _no_planes()
        return _cached(ent, x, key, want, both)
    return _cached(_state.last, x, key, want, both)


def _split3_cached_dy(dy, want="planar", both=False):
    """the dy planes of a layer are used twice in its backward (backward-weight, then backward-data)"""
    return _cached(_state.last_dy, dy, (dy.data_ptr(), tuple(dy.shape), ld_of(dy)), want, both)


def release_b3_cache():
    """releases the current state and the default one (never the state of another pass in flight)"""
    _state.release()
    _default_state.release()


# Direct 3x3 / stride 1 / pad 1 convolution of the HRNet trunk widths in split precision (csrc/dconv3_b3.hip): the fp32 activation is
# split into bf16 planes inside the kernel, a block reads the halo tile of its pixel tile once.  DCONV3_MIN_ROWS: below that many
# pixels the launch cannot fill the chip with its 128-pixel tiles and the fp32 implicit GEMM is as good (tests lower it).
DCONV3 = True
DCONV3_MIN_ROWS = 2048


def d3_layer(Cin, Cout, kh, kw, stride, pad, dil, groups):
    """a layer of the direct 3x3 kernels by geometry and library support, whatever its map size and the plan (the planner's _d3_ok and the
    engine's weight-image bank share it)"""
    return bool(kh == 3 and kw == 3 and stride == 1 and pad == 1 and dil == 1 and groups == 1 and Cin == Cout and lib.catseg_dconv3_supported(Cin))


def _d3_ok(rows, Cin, Cout, kh, kw, stride, pad, dil, groups):
    return DCONV3 and PRECISION == "bf16x3" and rows >= DCONV3_MIN_ROWS and d3_layer(Cin, Cout, kh, kw, stride, pad, dil, groups)


# Arithmetic of the direct trunk kernels' forward / backward-data: "f16x2" = two fp16 planes, three products (csrc/dconv3_f16x2.hip) for
# every launch whose input carries an amax record (left by its producer: bn_apply, add_n_act, bn_backward), "bf16x3" = three bf16 planes,
# six products.  CATSEG_TRUNK selects; inputs without a record always take the bf16x3 kernel.
TRUNK = _plan.get("trunk")


def _trunk_h2():
    return TRUNK == "f16x2" and PRECISION == "bf16x3"


# The trunk on PRODUCER-WRITTEN planes (round 4; csrc/planes.h, dconv3_pl.hip, dwgrad3_pl.hip): BatchNorm apply / the HRNet fuse sum / BatchNorm
# backward write the fp16 x 2 operand planes of what they produce, the direct kernels stream them by LDS-DMA.  CATSEG_TRUNK_PLANES=0: the
# round-3 route (fp32 tensors + amax records, split inside the convolution kernels).
PLANES = _plan.get("trunk_planes")


def _trunk_planes():
    return PLANES and _trunk_h2() and DCONV3


# Widths that take the planes route.  Measured within one run on the HRNet-W48 step (tools/ab_planes.py, min / median of 4 rounds, ms): fp32
# tensors + in-kernel split 118.9 / 128.9, planes for all four widths 118.4 / 118.6, planes for 96 / 192 / 384 only 117.1 / 117.5, planes for 48
# only 120.8 / 121.0.  The 48-channel layers stay on the round-3 kernel: standalone the planes kernel is 5 us faster there too (47.8 against
# 52.7 us), but it owns its CUs (eight waves of 128 registers per block, two blocks: every register of the SIMDs), whereas the uniform
# four-wave kernel leaves room for the BatchNorm / reduction kernels of the other branch streams to run beside it.
PLANES_WIDTHS = _plan.get("planes_widths")


def planes_ok(C, rows):
    """a trunk tensor of C channels and `rows` pixels takes the planes route: both plane kernels support the width"""
    return bool(_trunk_planes() and C in PLANES_WIDTHS and rows >= DCONV3_MIN_ROWS and lib.catseg_dconv3_pl_supported(C)
                and lib.catseg_dwgrad3_pl_supported(C))


AMAX_SCOPE_RECORDS = 1024
AMAX_WORDS = 512        # int32 words per record (include/catseg.h: CATSEG_AMAX_RECORD_BYTES): 16 slots 128 bytes apart


class AmaxScope:
    """the amax records of ONE forward pass and its backward: zeroed chunks of records, handed out in order.  A record lives as long as a
    tensor (or this scope) refers to its chunk -- a second forward pass (another network, a second micro-batch before the first backward)
    gets its own scope and cannot clear records that are still waiting for their backward.
    A chunk is zero-filled on the stream that is current when it is created (the first one at the stem, on the main stream; `records` sizes
    it for the whole pass when the owner knows the count of its previous pass).  Records are handed out on other streams too (HRNet's
    branch regions): the first request from a stream that may not be ordered behind the fill waits for the fill's event, so that a late
    memset can never erase an amax a sibling stream has already accumulated."""

    def __init__(self, device, records=AMAX_SCOPE_RECORDS):
        self.device, self.chunk, self.n, self.i = device, None, max(int(records), 16), 0
        self.used = 0
        self.i = self.n        # (first new() allocates)
        self.event, self.ordered = None, set()

    def new(self):
        cur = torch.cuda.current_stream(self.device) if self.device.type == "cuda" else None
        if self.i >= self.n:
            self.chunk, self.i = torch.zeros(AMAX_WORDS * self.n, dtype=torch.int32, device=self.device), 0
            if cur is not None:
                self.event = torch.cuda.Event()
                self.event.record(cur)
                self.ordered = {cur.cuda_stream}
        elif cur is not None and cur.cuda_stream not in self.ordered:
            cur.wait_event(self.event)
            self.ordered.add(cur.cuda_stream)
        i = self.i
        self.i = i + 1
        self.used += 1
        return self.chunk[AMAX_WORDS * i:AMAX_WORDS * (i + 1)]


def set_amax_scope(scope):
    """the scope new_amax() draws from: the current state's (the engine gives every pass its own)"""
    _state.amax_scope = scope


def new_amax(device):
    """a zeroed amax record (int32[AMAX_WORDS]) from the current scope (a private scope per device outside the engine)"""
    if _state.amax_scope is None or _state.amax_scope.device != device:
        _state.amax_scope = AmaxScope(device)
    return _state.amax_scope.new()


def amax_of(t):
    """the record a producing kernel attached to t, or None"""
    return getattr(t, "_amax", None)


SPLIT_BOUND = _plan.get("split_bound")    # f16x2 split passes take max|x| from the producers' records when they exist


def amax_records_of(t):
    """the amax records that bound |t|: its own, or those of the channel slices of a concatenation buffer (engine.concat_views); None if
    unknown or more than four"""
    r = getattr(t, "_amax", None)
    if r is not None:
        return [r]
    parts = getattr(t, "_amax_parts", None)
    return parts if parts and len(parts) <= 4 else None


def drop_amax(t):
    """a tensor that is about to be modified IN PLACE (an accumulating launch) loses the amax record its producer attached: the record
    would underestimate the new contents, and an underestimate overflows the fp16 planes of the trunk kernels (their prescale leaves one
    bit of headroom).  Without a record the consumer takes the three-plane bf16 kernel, which needs none."""
    if t is not None and getattr(t, "_amax", None) is not None:
        t._amax = None
    if t is not None and getattr(t, "_planes", None) is not None:
        t._planes = None           # (planes describe the old contents)
    if t is not None and getattr(t, "_amax_parts", None) is not None:
        t._amax_parts = None
    return t


def images_pending(ev, origin):
    """the pass's weight images are being written on a side stream (engine.EngineNet._run): ev marks their end, origin is the launch stream"""
    _state.images_event = (ev, origin)


def images_ready():
    """the current stream waits for the weight-image launches of this step (once: every later stream forks from the origin stream)"""
    if _state.images_event is not None:
        ev, origin = _state.images_event
        cur = torch.cuda.current_stream(origin.device)
        cur.wait_event(ev)
        if cur.cuda_stream == origin.cuda_stream:
            _state.images_event = None


def dconv3_weight_image(w, backward_data=False, h2=False):
    """pre-split weight image of the direct kernel; h2: the two-plane fp16 image and its scale record, (image, record)"""
    return _wi.weight_image(w, "d3", backward_data, h2=h2)


# Pointwise (1 x 1, stride 1) convolutions in split precision with the split in registers (csrc/pconv1.hip): every dense 1 x 1 layer whose
# input carries an amax record and that is too small for the blocked-plane kernels (ops._b3_wide_1x1) -- the stage-1 bottlenecks, the
# object-attention block of the OCR head, the HRNet fuse layers.  CATSEG_P1=0: the fp32 MFMA kernels, as in round 4.
# Measured (tools/time_p1.py, four tensors in turn, fp32 MFMA kernel -> this route, us per launch at the bench size): stage-1 64 -> 256 forward
# 178 -> 138, backward-data 113 -> 85; 256 -> 64 129 -> 81 / 135 -> 119; f_pixel 512 -> 256 609 -> 264 / 597 -> 326; 256 -> 256 337 -> 191 / 308 -> 176;
# f_up 256 -> 512 643 -> 354 / 555 -> 252 (2.3 - 4.1 TB/s of algorithmic bytes).  The fuse layers of the low-resolution branches (8 160 ... 65 280
# pixels: 32 ... 255 blocks of 256 rows) are no faster or slower (0.55 - 1.2 x): P1_MIN_ROWS keeps them on the fp32 kernels.  Backward-weight
# (p1t_kernel: LDS-bound, both operands pass through the transposing reads) pays for the 256 / 512-channel layers only (619 -> 492, 343 -> 276 us;
# 64-channel layers 0.82 - 0.89 x): P1_WGRAD_MIN_DIM.  HRNet-W48 step (tools/ab_p1.sh, graph replay, two alternating rounds): 109.06 / 109.97 ms
# without, 108.24 / 108.09 with all three operations on every layer, 107.72 / 107.65 with forward + backward-data only.
P1 = _plan.get("p1")
P1_MIN_ROWS = _plan.get("p1_min_rows")
P1_WGRAD_MIN_DIM = _plan.get("p1_wgrad_min_dim")
P1_OPS = _plan.get("p1_ops")


def p1_geometry(kh, kw, stride, pad, groups):
    """a pointwise layer by geometry"""
    return kh == 1 and kw == 1 and stride == 1 and pad == 0 and groups == 1


def p1_layer(Cin, Cout, kh, kw, stride, pad, groups):
    """a layer of the pointwise kernel (forward: N = Cout columns from K = Cin; backward-data: the same question with the two exchanged) by
    geometry and library support (shared by the planner and the engine's weight-image bank)"""
    return bool(p1_geometry(kh, kw, stride, pad, groups) and lib.catseg_pconv1_supported(Cout, Cin))


def _p1_ok(rows, Cin, Cout, kh, kw, stride, pad, dil, groups):
    return P1 and _trunk_h2() and p1_geometry(kh, kw, stride, pad, groups) and rows >= P1_MIN_ROWS and not _b3_wide_1x1(rows, Cout, 1, Cin)


def p1_weight_image(w, transposed=False):
    """(image, record) of a pointwise layer's weights [O, I, 1, 1] (physical OHWI = [O][I])"""
    return _wi.weight_image(w, "p1", transposed)


# Gather launches of the same kernels (csrc/pconv1.hip: catseg_gconv_*): dense kh x kw convolutions with stride 1 / 2 whose input carries an
# amax record and that neither the direct 3x3 kernels nor the blocked-plane kernels take -- the stride-2 layers of the HRNet fuse chains and
# transitions, the 256 -> 48 transition, the stem's second convolution.  CATSEG_G1=0: the fp32 MFMA kernels.
# Measured (tools/time_g1.py, fp32 MFMA kernel -> gather launch, us): 256 -> 48 3x3 at 8 x 136 x 240: forward 585 -> 398, backward-data 495 -> 249,
# backward-weight 739 -> 651; 256 -> 96 / stride 2: 251 -> 129, 315 -> 200, 348 -> 230; stem 64 -> 64 / stride 2: 225 -> 143 forward; 48 -> 96 / stride 2:
# 72 -> 46 forward, 107 -> 73 backward-weight -- but its backward-data (four parity-class launches with N = 48 columns) 88 -> 95 and 48 -> 48: 59 -> 76:
# backward-data takes the route from G1_DGRAD_MIN_CIN input channels on.  HRNet-W48 step (graph replay, three alternating rounds): 108.1 - 108.8 ms
# without, 107.9 - 108.2 with.
G1 = _plan.get("g1")
G1_MIN_ROWS = _plan.get("g1_min_rows")
G1_DGRAD_MIN_CIN = _plan.get("g1_dgrad_min_cin")
G1_MIN_CIN = _plan.get("g1_min_cin")
G1_OPS = _plan.get("g1_ops")


def _g1_ok(rows, Cin, Cout, kh, kw, stride, pad, dil, groups):
    return (G1 and _trunk_h2() and groups == 1 and (kh * kw > 1 or stride > 1) and rows >= G1_MIN_ROWS and Cin % 8 == 0 and Cin >= G1_MIN_CIN
            and not _b3_eligible(rows, Cout, kh * kw, Cin, stride == 1))


def g1_dgrad_layer(desc, Cin, Cout, kh, kw, stride):
    """backward-data of a gather layer by library support: desc (the layer's descriptor, or weight_images.gather_desc's shape-independent one) is a gather
    launch, and its parity-class launches are pointwise GEMMs with N = Cin, K = (taps of a class) * Cout (shared by the planner and the
    engine's weight-image bank)"""
    return bool(lib.catseg_gconv_supported(ctypes.byref(desc))
                and lib.catseg_pconv1_supported(Cin, ((kh + stride - 1) // stride) * ((kw + stride - 1) // stride) * Cout))


def g1_weight_image(w, backward_data, stride, pad, dil):
    """(image(s), record) of a gather layer: the forward image, or the stride^2 class images of backward-data back to back"""
    return _wi.weight_image(w, "g1", backward_data, stride=stride, pad=pad, dil=dil)


def pconv1(x, wimg, bias, N, out, accumulate=False, bn_stats=False):
    """out[rows][N] (+)= x[rows][K] . B^T (+ bias) through csrc/pconv1.hip; x carries an amax record; wimg = p1_weight_image(...)"""
    rows, K = rows_of(x), x.shape[-1]
    part = tr = nt = None
    if bn_stats:
        part = _bn_part_buffer(3 * ((rows + 255) // 256) * N, x.device)
        tr, nt = ctypes.c_int(0), ctypes.c_int(0)
    check(lib.catseg_pconv1(rows, N, K, ptr(x), ld_of(x), ptr(amax_of(x)), ptr(wimg[0]), ptr(wimg[1]), ptr(bias), ptr(out), ld_of(out),
                            1 if accumulate else 0, ptr(part), part.numel() if part is not None else 0,
                            ctypes.byref(tr) if bn_stats else None, ctypes.byref(nt) if bn_stats else None, stream()))
    if bn_stats:
        return out, ((part, nt.value, tr.value) if tr.value > 0 else None)
    return out


def dconv3(x, wimg, bias=None, out=None, accumulate=False, bn_stats=False, x_amax=None):
    """y (+)= conv3x3(x) from a weight image; bn_stats: also returns (partials, n_tiles, 0, counts) for bn_finalize.
    x_amax: the input's amax record -> the two-plane fp16 kernel; wimg is then (image, record) of dconv3_weight_image(..., h2=True)"""
    B, H, W, C = x.shape
    if out is None:
        out = new_act(B, H, W, C, x.device)
        accumulate = False
    drop_amax(out)
    part = cnt = None
    nt = 0
    if bn_stats:
        nt = lib.catseg_dconv3_tiles(C, B, H, W, None, None)
        part = _bn_part_buffer(3 * nt * C + nt, x.device)
        cnt = part[3 * nt * C:3 * nt * C + nt].view(torch.int32)
    if x_amax is not None:
        check(lib.catseg_dconv3_f16x2(B, H, W, C, ptr(x), ld_of(x), ptr(x_amax), ptr(wimg[0]), ptr(wimg[1]), ptr(bias), ptr(out), ld_of(out),
                                      1 if accumulate else 0, ptr(part), 3 * nt * C, ptr(cnt), stream()))
    else:
        check(lib.catseg_dconv3(B, H, W, C, ptr(x), ld_of(x), ptr(wimg), ptr(bias), ptr(out), ld_of(out), 1 if accumulate else 0,
                                ptr(part), 3 * nt * C, ptr(cnt), stream()))
    if bn_stats:
        return out, (part, nt, 0, cnt)
    return out


class Planes:
    """the fp16 x 2 operand planes of an NHWC activation (csrc/planes.h) + its record (amax slots, word 1 = the planes' exponent)"""
    __slots__ = ("buf", "rec", "shape")

    def __init__(self, buf, rec, shape):
        self.buf, self.rec, self.shape = buf, rec, tuple(shape)


def planes_of(t):
    """the planes a producing kernel attached to t, or None"""
    return getattr(t, "_planes", None)


def planes_from_f32(x, rec=None):
    """standalone producer: planes of x with the exponent from max|x| (rec given: its amax slots are taken as they are)"""
    B, H, W, C = x.shape
    buf = torch.empty(lib.catseg_planes_bytes(B * H * W, C), dtype=torch.uint8, device=x.device)
    own = rec is None
    if own:
        rec = new_amax(x.device)
    check(lib.catseg_planes_from_f32(ptr(x), ld_of(x), B * H * W, C, ptr(rec), ptr(buf), 1 if own else 0, stream()))
    return Planes(buf, rec, x.shape)


def dconv3_pl(xp, wimg, bias=None, out=None, accumulate=False, bn_stats=False, out_rec=None):
    """y (+)= conv3x3(x) from the planes of x (Planes) and an f16x2 weight image (image, record); bn_stats: also returns
    (partials, n_rows, 0, counts) for bn_finalize -- per-WAVE rows"""
    B, H, W, C = xp.shape
    if out is None:
        out = new_act(B, H, W, C, xp.buf.device)
        accumulate = False
    drop_amax(out)
    part = cnt = None
    nr = 0
    if bn_stats:
        nr = lib.catseg_dconv3_pl_rows(C, B, H, W)
        part = _bn_part_buffer(3 * nr * C + nr, xp.buf.device)
        cnt = part[3 * nr * C:3 * nr * C + nr].view(torch.int32)
    check(lib.catseg_dconv3_pl(B, H, W, C, ptr(xp.buf), ptr(xp.rec), ptr(wimg[0]), ptr(wimg[1]), ptr(bias), ptr(out), ld_of(out),
                               1 if accumulate else 0, ptr(part), 3 * nr * C, ptr(cnt), ptr(out_rec), stream()))
    if bn_stats:
        return out, (part, nr, 0, cnt)
    return out


def dwgrad3_pl(xp, dyp, dw):
    """backward-weight of a 3x3 / stride 1 / pad 1 trunk convolution from the planes of x and dy (Planes)"""
    B, H, W, C = xp.shape
    need = lib.catseg_dwgrad3_pl_workspace(B, H, W, C)
    ws = workspace(need + 256, xp.buf.device)
    with _Timed("wgrad_d3p", 2.0 * B * H * W * C * C * 9):
        check(lib.catseg_dwgrad3_pl(B, H, W, C, ptr(xp.buf), ptr(xp.rec), ptr(dyp.buf), ptr(dyp.rec), ptr(dw), ptr(ws), need, stream()))
    return dw


_bn_part = {}


def _bn_part_buffer(nfloats, device):
    """grow-only buffer (per device and stream) for the per-tile BatchNorm partials a convolution epilogue writes (consumed by
    the next launch on the same stream)"""
    key = (device.type, device.index, torch.cuda.current_stream(device).cuda_stream if device.type == "cuda" else 0)
    buf = _bn_part.get(key)
    if buf is None or buf.numel() < nfloats:
        buf = torch.empty(max(int(nfloats), 1 << 18), dtype=torch.float32, device=device)
        _bn_part[key] = buf
    return buf


def _refuse_placeholder(t, what):
    """a planes-only activation (bn_apply(planes_only=True)) is an UNWRITTEN fp32 placeholder: only the plane-streaming kernels may consume
    it.  Every other route of the convolution wrappers refuses it instead of reading uninitialised memory (a consumer with
    exact_operands, a failed _d3_ok, a bias, or CATSEG_PLANES_WIDTHS / DCONV3 toggled between producer and consumer would get here)."""
    if getattr(t, "_planes_only", False):
        raise RuntimeError("a planes-only activation reached %s, which reads fp32: its fp32 tensor was never written "
                           "(engine.conv_bn_act(sole_conv_out=True) requires the planes route on the consumer)" % what)


# The first stem convolution of HRNet (3 -> 64, 3 x 3 / stride 2 / pad 1 on the image) as HBM-bound direct fp32 kernels (csrc/stem3.hip) instead of
# the implicit GEMM over 9 taps x 4 padded channels.  CATSEG_STEM3=0: the implicit-GEMM route.
STEM3 = _plan.get("stem3")


def _image_strides(x):
    """(B, H, W, sb, sc, sy, sx) of a 3-channel image given as NCHW [B, 3, H, W] or NHWC-4 [B, H, W, 4]"""
    if x.dim() == 4 and x.shape[-1] == 4 and x.shape[1] != 3:
        B, H, W, _ = x.shape
        return B, H, W, x.stride(0), 1, x.stride(1), x.stride(2)
    B, _, H, W = x.shape
    return B, H, W, x.stride(0), x.stride(1), x.stride(2), x.stride(3)


def stem3_ok(x, w, kh, kw, stride, pad, dil, groups):
    if not (STEM3 and x.is_cuda and x.dtype == torch.float32 and w.dim() == 4 and w.shape[1] == 3 and (kh, kw, stride, pad, dil, groups) == (3, 3, 2, 1, 1, 1)):
        return False
    B, H, W = _image_strides(x)[:3]
    return bool(lib.catseg_stem3_supported(H, W, w.shape[0]))


def stem3_fwd(x, w, bias, bn_stats=False):
    """x: the image (NCHW or NHWC-4, any strides); w: [64, 3, 3, 3] in channels_last memory (physical OHWI).  Returns y NHWC [B, Ho, Wo, 64]
    (+ the BatchNorm partials (part, rows, 0, counts) for bn_finalize)"""
    B, H, W, sb, sc, sy, sx = _image_strides(x)
    Cout = w.shape[0]
    Ho, Wo = conv_out_size(H, 3, 2, 1, 1), conv_out_size(W, 3, 2, 1, 1)
    out = new_act(B, Ho, Wo, Cout, x.device)
    part = cnt = None
    nt = 0
    if bn_stats:
        nt = lib.catseg_stem3_partial_rows(B, H, W)
        part = _bn_part_buffer(3 * nt * Cout + nt, x.device)
        cnt = part[3 * nt * Cout:3 * nt * Cout + nt].view(torch.int32)
    with _Timed("hbm:stem3", 4.0 * (B * 3 * H * W + out.numel())):
        check(lib.catseg_stem3_fwd(ptr(x), sb, sc, sy, sx, B, H, W, ptr(w), ptr(bias), ptr(out), ld_of(out), ptr(part), ptr(cnt), stream()))
    return (out, (part, nt, 0, cnt)) if bn_stats else out


def stem3_bwd_weight(x, dy, dw):
    B, H, W, sb, sc, sy, sx = _image_strides(x)
    need = lib.catseg_stem3_wgrad_workspace()
    ws = workspace(need, x.device)
    with _Timed("hbm:stem3", 4.0 * (B * 3 * H * W + dy.numel())):
        check(lib.catseg_stem3_bwd_weight(ptr(x), sb, sc, sy, sx, B, H, W, ptr(dy), ld_of(dy), ptr(dw), ptr(ws), need, stream()))
    return dw


# The first convolution of the torchvision ResNet stem (3 -> 64, 7 x 7 / stride 2 / pad 3 on the image), training forward accumulated in fp64 and
# rounded once (csrc/stem7.hip): what csrc/stem3.hip did for the HRNet models' literal-1e-3 distance to the CPU path, for OCRNet-R50 / DeepLabv3+.
# The layer's backward-weight stays on the implicit GEMM (stem4 layout).  CATSEG_STEM7=0: the implicit-GEMM forward.
STEM7 = _plan.get("stem7")


def stem7_ok(x, w, kh, kw, stride, pad, dil, groups):
    if not (STEM7 and x.is_cuda and x.dtype == torch.float32 and w.dim() == 4 and w.shape[1] == 3 and (kh, kw, stride, pad, dil, groups) == (7, 7, 2, 3, 1, 1)):
        return False
    B, H, W = _image_strides(x)[:3]
    return bool(lib.catseg_stem7_supported(H, W, w.shape[0]))


def stem7_fwd(x, w, bias, bn_stats=False):
    """x: the image (NCHW or NHWC-4, any strides); w: [64, 3, 7, 7] in channels_last memory (physical OHWI).  Returns y NHWC [B, Ho, Wo, 64]
    (+ the BatchNorm partials (part, rows, 0, counts) for bn_finalize)"""
    B, H, W, sb, sc, sy, sx = _image_strides(x)
    Cout = w.shape[0]
    Ho, Wo = conv_out_size(H, 7, 2, 3, 1), conv_out_size(W, 7, 2, 3, 1)
    out = new_act(B, Ho, Wo, Cout, x.device)
    part = cnt = None
    nt = 0
    if bn_stats:
        nt = lib.catseg_stem7_partial_rows(B, H, W)
        part = _bn_part_buffer(3 * nt * Cout + nt, x.device)
        cnt = part[3 * nt * Cout:3 * nt * Cout + nt].view(torch.int32)
    with _Timed("hbm:stem7", 4.0 * (B * 3 * H * W + out.numel())):
        check(lib.catseg_stem7_fwd(ptr(x), sb, sc, sy, sx, B, H, W, ptr(w), ptr(bias), ptr(out), ld_of(out), ptr(part), ptr(cnt), stream()))
    return (out, (part, nt, 0, cnt)) if bn_stats else out


def _refuse_h2_only(t, what):
    """a tensor that exists ONLY as blocked f16x2 planes (concat_bilinear_h2: the HRNet head input) is an unwritten fp32 placeholder too: only
    the f16x2 kernels, through the planes registered for it, may consume it"""
    if getattr(t, "_h2_only", False):
        raise RuntimeError("a tensor that exists only as blocked f16x2 planes reached %s, which reads fp32 (its fp32 tensor was never written)" % what)


# ---------------------------------------------------------------------------------------------- the route planner
# Which kernel family runs a convolution, per direction: fwd_route / dgrad_route / wgrad_route map a Layer (shapes, the flags of the call and
# facts about the operands -- no tensor data, nothing is launched) to a Route.  Every rung's condition is written here and nowhere else;
# the rungs are tried in the order they are written.  conv_fwd / conv_bwd_data / conv_bwd_weight plan, then launch; the predictors
# (h2_dy_route, concat_planes_route, conv_fwd_fused, the h2-only guards) ask the same functions with the operand facts they assume.
#   d3p  direct 3x3 trunk kernel on producer-written fp16 x 2 planes (dconv3_pl.hip)         s2p  gather launches of pconv1.hip
#   d3h  direct 3x3 trunk kernel, f16x2, split in the kernel from an amax record             h2   blocked-plane GEMM, f16x2 (igemm_f16x2.hip)
#   d3   direct 3x3 trunk kernel, bf16x3 (no record needed)                                  b3   bf16x3 GEMM, blocked or planar planes
#   p1   pointwise kernel (pconv1.hip)                                                       f32  fp32 implicit GEMM (igemm.hip)
# The thresholds are read from this module's attributes at call time (tests, bench.py and the A/B tools assign to them after import).
Route = collections.namedtuple("Route", "kind blocked")     # blocked: the GEMM reads blocked planes (h2 / b3 only)
D3P, D3H, D3, P1R, S2P, F32 = (Route(k, False) for k in ("d3p", "d3h", "d3", "p1", "s2p", "f32"))
H2_BLOCKED = Route("h2", True)      # the one route that can read planes registered for a tensor (register_h2_planes)


class Layer:
    """what the planner knows of one convolution call.  xshape = (B, H, W, Cin) of the input side, ldx / ldy the pixel strides of the tensors
    on the input side (x, dx) and the output side (y, dy); yshape: dy's shape where the caller holds one (default: what the geometry gives).
    Flags: stem4, exact, zero_to, bias (present), w4d (the weight / its gradient is a 4-D tensor).  Operand facts: x_amax / dy_amax (the
    tensor carries an amax record), x_planes (producer-written planes)."""
    __slots__ = ("xshape", "B", "H", "W", "Cin", "Cout", "kh", "kw", "stride", "pad", "dil", "groups", "ldx", "ldy", "yshape", "rows_i", "rows_o",
                 "stem4", "exact", "zero_to", "bias", "w4d", "x_amax", "x_planes", "dy_amax")

    def __init__(self, xshape, Cout, kh, kw, stride=1, pad=0, dil=1, groups=1, ldx=None, ldy=None, yshape=None, stem4=False, exact=False,
                 zero_to=0, bias=False, w4d=True, x_amax=False, x_planes=False, dy_amax=False):
        self.xshape = tuple(xshape)
        self.B, self.H, self.W, self.Cin = B, H, W, Cin = self.xshape
        self.Cout, self.kh, self.kw, self.stride, self.pad, self.dil, self.groups = Cout, kh, kw, stride, pad, dil, groups
        self.ldx, self.ldy = ldx or (Cin + 3) // 4 * 4, ldy or (Cout + 3) // 4 * 4
        self.yshape = tuple(yshape) if yshape is not None else (B, conv_out_size(H, kh, stride, pad, dil), conv_out_size(W, kw, stride, pad, dil), Cout)
        self.rows_i, self.rows_o = B * H * W, 1
        for n in self.yshape[:-1]:
            self.rows_o *= n
        self.stem4, self.exact, self.zero_to, self.bias, self.w4d = stem4, exact, zero_to, bias, w4d
        self.x_amax, self.x_planes, self.dy_amax = x_amax, x_planes, dy_amax

    def geom(self, transposed=False):
        """the argument tail of the _d3_ok / _p1_ok / _g1_ok predicates; transposed: input and output channels exchanged (backward-data as a forward)"""
        cc = (self.Cout, self.Cin) if transposed else (self.Cin, self.Cout)
        return cc + (self.kh, self.kw, self.stride, self.pad, self.dil, self.groups)

    def desc(self):
        return make_desc(self.xshape, self.ldx, self.Cout, self.ldy, self.kh, self.kw, self.stride, self.pad, self.dil)

    def y_fits(self):
        """the output-side tensor has the size the geometry gives (a caller may hand backward a cropped or padded dy)"""
        d = self.desc()
        return d.Ho == self.yshape[1] and d.Wo == self.yshape[2]


def _small(rows, ld):
    """a tensor the pointwise / gather kernels can address (32-bit byte offsets)"""
    return rows * ld * 4 < B3_PLANE_LIMIT


def _fwd_gemm_ok(L):
    return (not L.exact and "fwd" in B3_OPS and not L.stem4 and L.groups == 1 and L.w4d
            and _b3_eligible(L.rows_o, L.Cout, L.kh * L.kw, L.Cin))


def fwd_route(L):
    taps = L.kh * L.kw
    dense = not L.exact and not L.stem4 and L.zero_to == 0 and L.w4d      # the direct / pointwise / gather kernels: no exact operands, no padded output
    if dense and _d3_ok(L.rows_o, *L.geom()):
        if not L.bias and planes_ok(L.Cin, L.rows_o) and (L.x_planes or L.x_amax):
            return D3P
        return D3H if L.x_amax and _trunk_h2() else D3
    if (dense and "fwd" in P1_OPS and L.x_amax and _p1_ok(L.rows_o, *L.geom()) and lib.catseg_pconv1_supported(L.Cout, L.Cin)
            and _small(L.rows_o, L.ldx)):
        return P1R
    if (dense and "fwd" in G1_OPS and L.x_amax and _g1_ok(L.rows_o, *L.geom()) and _small(L.rows_i, L.ldx)
            and lib.catseg_gconv_supported(ctypes.byref(L.desc()))):
        return S2P
    if _fwd_gemm_ok(L):
        blk = _b3_blocked_ok(max(L.zero_to, L.Cout), L.Cin, L.rows_i, L.Cout, taps)
        return Route("h2" if blk and _h2() else "b3", blk)
    return F32


def dgrad_route(L):
    taps, cred = L.kh * L.kw, (L.Cout + 7) // 8 * 8
    if L.w4d and _d3_ok(L.rows_i, *L.geom()):
        return D3H if L.dy_amax and _trunk_h2() else D3
    if (L.w4d and "dgrad" in P1_OPS and L.dy_amax and _p1_ok(L.rows_i, *L.geom(transposed=True)) and lib.catseg_pconv1_supported(L.Cin, L.Cout)
            and _small(L.rows_o, L.ldy)):
        return P1R
    elig = _b3_eligible(L.rows_i, L.Cin, taps, cred, L.stride == 1)      # (the gather rung leaves these layers to the GEMM rung)
    if (L.w4d and "dgrad" in G1_OPS and L.dy_amax and L.Cout % 8 == 0 and L.Cin >= G1_DGRAD_MIN_CIN and _g1_ok(L.rows_o, *L.geom())
            and not elig and _small(L.rows_o, L.ldy) and g1_dgrad_layer(L.desc(), L.Cin, L.Cout, L.kh, L.kw, L.stride) and L.y_fits()):
        return S2P
    if L.groups == 1 and "dgrad" in B3_OPS and elig:
        blk = _b3_blocked_ok(L.Cin, (L.Cout + 15) // 16 * 16, L.rows_o, L.Cin, taps)
        return Route("h2" if blk and _h2() else "b3", blk)
    return F32


def _wgrad_gemm_ok(L):
    """backward-weight runs the split-precision implicit GEMM (igemm_h2t / igemm_b3t) on planes of x and dy"""
    taps = L.kh * L.kw
    return bool(L.groups == 1 and "wgrad" in B3_OPS and not L.stem4 and PRECISION == "bf16x3" and L.Cin % 8 == 0 and
                L.rows_i * L.Cin < B3_INDEX_LIMIT and L.rows_o * ((L.Cout + 7) // 8 * 8) < B3_INDEX_LIMIT and
                ((B3_MIN_TAPS <= taps and taps * L.Cin >= B3_MIN_K and L.Cout >= B3_MIN_N and L.rows_o >= B3_MIN_WGRAD_ROWS)
                 or (L.stride == 1 and _b3_wide_1x1(L.rows_o, L.Cout, taps, L.Cin))))


def _wgrad_h2_ok(L):
    """... on two fp16 planes per operand, each operand's planes behind one 32-bit-offset buffer resource"""
    pad = 16 if H2T_BLOCKED else 8
    return bool(_h2() and 4 * L.rows_i * ((L.Cin + pad - 1) // pad * pad) < B3_PLANE_LIMIT
                and 4 * L.rows_o * ((L.Cout + pad - 1) // pad * pad) < B3_PLANE_LIMIT)


def wgrad_route(L):
    if not L.stem4 and _d3_ok(L.rows_o, *L.geom()) and lib.catseg_dwgrad3_supported(L.Cin):
        return D3H if L.x_amax and L.dy_amax and _trunk_h2() else D3
    recs = not L.stem4 and L.w4d and L.x_amax and L.dy_amax and _small(L.rows_i, L.ldx) and _small(L.rows_o, L.ldy)
    if (recs and "wgrad" in P1_OPS and min(L.Cout, L.Cin) >= P1_WGRAD_MIN_DIM and _p1_ok(L.rows_o, *L.geom())
            and lib.catseg_pconv1_wgrad_supported(L.Cout, L.Cin)):
        return P1R
    gemm = _wgrad_gemm_ok(L)
    if (recs and "wgrad" in G1_OPS and _g1_ok(L.rows_o, *L.geom()) and not gemm and lib.catseg_gconv_wgrad_supported(ctypes.byref(L.desc()))
            and L.y_fits()):
        return S2P
    if gemm:
        return Route("h2", H2T_BLOCKED) if _wgrad_h2_ok(L) else Route("b3", False)
    return F32


ConvArgs = collections.namedtuple("ConvArgs", "weight Cout kh kw stride pad dil groups bias")


def conv_args(conv):
    """THE unpacking of a convolution module (nn.Conv2d / nn.ConvTranspose2d; stride, padding and dilation are square in every model here).
    weight and bias are the parameters themselves; a shape-only stand-in for a module (the planner's predictors) has no weight"""
    kh, kw = conv.kernel_size
    return ConvArgs(getattr(conv, "weight", None), conv.out_channels, kh, kw, conv.stride[0], conv.padding[0], conv.dilation[0], conv.groups,
                    conv.bias)


def _h2_only_guard(x, route, what):
    """a tensor that exists only as blocked f16x2 planes may only take the route that reads them"""
    if getattr(x, "_h2_only", False) and route != H2_BLOCKED:
        _refuse_h2_only(x, what)


def conv_fwd(x, w_ptr_tensor, bias, Cout, kh, kw, stride=1, pad=0, dil=1, out=None, zero_to=0, stem4=False, groups=1, bn_stats=False, train=False,
             exact=False, with_yrec=False):
    """train=True (the engine's recorded forward): a backward pass will follow -- the split planes of x are written in both layouts
    and kept for it (in the current state, until that is released).
    exact=True (the first layers of a trunk, whose rounding error the rest of the network amplifies most: tools/error_growth.py): the
    layer runs the fp32 MFMA kernel (exact operands, two-level accumulation: csrc/igemm.hip TWO_LEVEL) whatever the split-precision
    kernels could take.  (Measured at 2 x 3 x 544 x 960, relative RMS error of layer1's output against fp64: fp32 CPU 1.22e-6, this 0.89e-6,
    two fp16 planes 1.12e-6, three bf16 planes / six products 1.25e-6 -- 84 accumulator roundings per output instead of 42.)
    bn_stats=True: returns (out, partials) where partials = (buffer, n_tiles, tile_rows) are the per-(M-tile, channel)
    BatchNorm partial sums written by the convolution's epilogue (for bn_finalize), or None if this layer's kernel has none
    with_yrec=True: returns (result, record) -- result as without it, record the max|y| record the planes kernel left (None on every
    other route)"""
    B, H, W, Cin = x.shape
    Ho, Wo = conv_out_size(H, kh, stride, pad, dil), conv_out_size(W, kw, stride, pad, dil)
    if out is None:
        out = new_act(B, Ho, Wo, Cout, x.device, ld=max(zero_to, (Cout + 3) // 4 * 4))
    flops = 2.0 * B * Ho * Wo * Cout * (3 if stem4 else Cin // groups) * kh * kw
    rows = B * Ho * Wo
    part = tr = nt = None
    if bn_stats:
        part = _bn_part_buffer(3 * ((rows + 63) // 64) * Cout, x.device)
        tr, nt = ctypes.c_int(0), ctypes.c_int(0)
    route = fwd_route(Layer(x.shape, Cout, kh, kw, stride, pad, dil, groups, ld_of(x), ld_of(out), stem4=stem4, exact=exact, zero_to=zero_to,
                            bias=bias is not None, w4d=w_ptr_tensor.dim() == 4, x_amax=amax_of(x) is not None, x_planes=planes_of(x) is not None))
    _h2_only_guard(x, route, "a convolution forward outside the blocked f16x2 route")
    if route == D3P:
        xp = planes_of(x)
        if xp is None:      # a tensor whose producer wrote no planes (the first block behind a transition): one split pass, kept for backward
            xp = planes_from_f32(x, rec=amax_of(x))
            x._planes = xp
        yrec = new_amax(x.device)
        with _Timed("fwd_d3p", flops):
            res = dconv3_pl(xp, _wi.weight_image(w_ptr_tensor, "d3", h2=True), None, out=out, bn_stats=bn_stats, out_rec=yrec)
        return (res, yrec) if with_yrec else res
    if route in (D3H, D3):
        _refuse_placeholder(x, "the in-kernel-split direct 3x3 kernel")
        rec = amax_of(x) if route == D3H else None
        wimg = _wi.weight_image(w_ptr_tensor, "d3", h2=rec is not None)
        with _Timed("fwd_d3h" if rec is not None else "fwd_d3", flops):
            res = dconv3(x, wimg, bias, out=out, bn_stats=bn_stats, x_amax=rec)
        return (res, None) if with_yrec else res
    _refuse_placeholder(x, "a convolution forward outside the planes route")
    if route == P1R:
        with _Timed("fwd_p1", flops):
            res = pconv1(x, _wi.weight_image(w_ptr_tensor, "p1"), bias, Cout, out, bn_stats=bn_stats)
        drop_amax(out)
        return (res, None) if with_yrec else res
    if route == S2P:
        d = make_desc(x.shape, ld_of(x), Cout, ld_of(out), kh, kw, stride, pad, dil)
        if bn_stats:
            part = _bn_part_buffer(3 * ((rows + 255) // 256) * Cout, x.device)
        wimg = _wi.weight_image(w_ptr_tensor, "g1", stride=stride, pad=pad, dil=dil)
        with _Timed("fwd_s2p", flops):
            check(lib.catseg_gconv_fwd(ctypes.byref(d), ptr(x), ptr(amax_of(x)), ptr(wimg[0]), ptr(wimg[1]), ptr(bias), ptr(out), ptr(part),
                                       part.numel() if part is not None else 0, ctypes.byref(tr) if bn_stats else None,
                                       ctypes.byref(nt) if bn_stats else None, stream()))
        drop_amax(out)
    else:
        if route.kind == "h2":
            kind, operands = "fwd_h2", OPERANDS_F16X2_BLOCKED
            with _Timed("split3", 0.0):
                xp, xsc = _split3_cached(x, "h2", both=train and not H2T_BLOCKED, keep=train)
                wp, wsc = _wi.weight_image(w_ptr_tensor, "h2")
        elif route.kind == "b3":
            blk = route.blocked
            kind, operands, xsc, wsc = "fwd_b3", OPERANDS_BF16X3_BLOCKED if blk else OPERANDS_BF16X3, None, None
            with _Timed("split3", 0.0):
                xp = _split3_cached(x, "blk" if blk else "planar", both=blk and train, keep=train)
                wp = _wi.weight_image(w_ptr_tensor, "b3", blocked=blk)
        else:
            kind, operands, xp, xsc, wp, wsc = "fwd", OPERANDS_F32, x, None, w_ptr_tensor, None
        if operands == OPERANDS_F32:
            d = make_desc(x.shape, ld_of(x), Cout, ld_of(out), kh, kw, stride, pad, dil, stem4, groups)
        else:
            d = make_desc(x.shape, Cin, Cout, ld_of(out), kh, kw, stride, pad, dil)
        stats = dict(bn_part=part, bn_part_floats=part.numel(), tile_rows=ctypes.addressof(tr), n_tiles=ctypes.addressof(nt)) if bn_stats else {}
        with _Timed(kind, flops):
            _conv_call(ConvFwdDesc, d, operands, x=xp, x_scale=xsc, w=wp, w_scale=wsc, bias=bias, y=out, zero_to=zero_to, **stats)
    res = (out, (part, nt.value, tr.value) if tr.value > 0 else None) if bn_stats else out
    return (res, None) if with_yrec else res


def bn_finalize(partials, rows, C, gamma, eps, momentum, running_mean, running_var, bound=None):
    """batch statistics from the convolution epilogue's per-tile partials: (stats [mean(C), invstd(C)], scale).
    bound = (beta, y_record, z_record): also leaves the bound of the normalised output in z_record (csrc/norm.hip: the exponent of z's planes)"""
    part, n_tiles, tile_rows = partials[:3]
    stats = torch.empty(2 * C, dtype=torch.float32, device=part.device)
    scale = torch.empty(C, dtype=torch.float32, device=part.device)
    if bound is not None:
        beta, yrec, zrec = bound
        check(lib.catseg_bn_finalize_counts_bound(ptr(part), n_tiles, ptr(partials[3]), rows, C, ptr(gamma), ptr(beta), eps, momentum,
                                                  ptr(running_mean), ptr(running_var), ptr(stats), ptr(scale), ptr(yrec), ptr(zrec), stream()))
        return stats, scale
    if len(partials) > 3:       # tiles with individual pixel counts (the direct 3x3 kernel's 2-D tiles)
        check(lib.catseg_bn_finalize_counts(ptr(part), n_tiles, ptr(partials[3]), rows, C, ptr(gamma), eps, momentum, ptr(running_mean),
                                            ptr(running_var), ptr(stats), ptr(scale), stream()))
        return stats, scale
    check(lib.catseg_bn_finalize(ptr(part), n_tiles, tile_rows, rows, C, ptr(gamma), eps, momentum, ptr(running_mean), ptr(running_var),
                                 ptr(stats), ptr(scale), stream()))
    return stats, scale


BN_BWD_FUSE = True    # first pass of the backward of relu(bn1(.)) in the epilogue of the backward-data kernel that produces its dz


def conv_bwd_data(dy, w, xshape, kh, kw, stride=1, pad=0, dil=1, out=None, accumulate=False, groups=1, bn_src=None, with_pre=False):
    """bn_src = (q, stats, gamma, beta): the convolution's input was relu(bn(q)) and this call is the ONLY contribution to its
    gradient.  When the direct kernel takes the layer, the result is then already masked (g = dx where relu(bn(q)) > 0) and the
    call returns (g, (partials, n_tiles)) for bn_backward_pre; otherwise it returns dx alone, as without bn_src.
    with_pre=True: always returns the pair, (dx, None) where the epilogue did not run that pass."""
    B, H, W, Cin = xshape
    Cout = dy.shape[-1]
    _refuse_placeholder(dy, "conv_bwd_data (fp32 output gradient)")
    if out is None:
        out = new_act(B, H, W, Cin, dy.device)
        accumulate = False
    drop_amax(out)
    flops = 2.0 * rows_of(dy) * Cout * (Cin // groups) * kh * kw
    route = dgrad_route(Layer(xshape, Cout, kh, kw, stride, pad, dil, groups, ld_of(out), ld_of(dy), yshape=dy.shape, w4d=w.dim() == 4,
                              dy_amax=amax_of(dy) is not None))
    if route in (D3H, D3):
        rec = amax_of(dy) if route == D3H else None
        wimg = _wi.weight_image(w, "d3", True, h2=rec is not None)
        kind = "dgrad_d3h" if rec is not None else "dgrad_d3"
        if bn_src is not None and BN_BWD_FUSE and not accumulate:
            q, stats, gamma, beta = bn_src
            nt = lib.catseg_dconv3_tiles(Cin, B, H, W, None, None)
            part = torch.empty(2 * nt * Cin, dtype=torch.float32, device=dy.device)
            with _Timed(kind, flops):
                if rec is not None:
                    check(lib.catseg_dconv3_bnbwd_f16x2(B, H, W, Cin, ptr(dy), ld_of(dy), ptr(rec), ptr(wimg[0]), ptr(wimg[1]), ptr(out), ld_of(out),
                                                        ptr(q), ld_of(q), ptr(stats), ptr(gamma), ptr(beta), ptr(part), part.numel(), stream()))
                else:
                    check(lib.catseg_dconv3_bnbwd(B, H, W, Cin, ptr(dy), ld_of(dy), ptr(wimg), ptr(out), ld_of(out), ptr(q), ld_of(q),
                                                  ptr(stats), ptr(gamma), ptr(beta), ptr(part), part.numel(), stream()))
            return out, (part, nt)
        with _Timed(kind, flops):
            dconv3(dy, wimg, None, out=out, accumulate=accumulate, x_amax=rec)
    elif route == P1R:
        with _Timed("dgrad_p1", flops):
            pconv1(dy, _wi.weight_image(w, "p1", True), None, Cin, out, accumulate=accumulate)
    elif route == S2P:
        d = make_desc(xshape, ld_of(out), Cout, ld_of(dy), kh, kw, stride, pad, dil)
        wimg = _wi.weight_image(w, "g1", True, stride=stride, pad=pad, dil=dil)
        with _Timed("dgrad_s2p", flops):
            check(lib.catseg_gconv_bwd_data(ctypes.byref(d), ptr(dy), ptr(amax_of(dy)), ptr(wimg[0]), ptr(wimg[1]), ptr(out),
                                            1 if accumulate else 0, stream()))
    else:
        if route.kind == "h2":
            kind, operands = "dgrad_h2", OPERANDS_F16X2_BLOCKED
            with _Timed("split3", 0.0):
                dyp, dysc = _split3_cached_dy(dy, "h2")
                wtp, wtsc = _wi.weight_image(w, "h2", True)
        elif route.kind == "b3":
            blk = route.blocked
            kind, operands, dysc, wtsc = "dgrad_b3", OPERANDS_BF16X3_BLOCKED if blk else OPERANDS_BF16X3, None, None
            with _Timed("split3", 0.0):
                dyp = _split3_cached_dy(dy, "blk" if blk else "planar")
                wtp = _wi.weight_image(w, "b3", True, blocked=blk)
        else:
            kind, operands, dyp, dysc, wtp, wtsc = "dgrad", OPERANDS_F32, dy, None, w, None
        if operands == OPERANDS_F32:
            d = make_desc(xshape, ld_of(out), Cout, ld_of(dy), kh, kw, stride, pad, dil, False, groups)
        else:
            d = make_desc(xshape, ld_of(out), Cout, (Cout + 7) // 8 * 8, kh, kw, stride, pad, dil)
        with _Timed(kind, flops):
            _conv_call(ConvBwdDataDesc, d, operands, dy=dyp, dy_scale=dysc, w=wtp, w_scale=wtsc, dx=out, accumulate=1 if accumulate else 0)
    return (out, None) if with_pre else out


def _wgrad_h2_planes(x, dy, dgrad_blk):
    """(x planes, x scale, dy planes, dy scale) of the f16x2 backward-weight kernel"""
    if H2T_BLOCKED:
        xp, xsc = _split3_cached(x, "h2")
        dyp, dysc = _split3_cached_dy(dy, "h2")
    else:
        xp, xsc = _split3_cached(x, "h2p")
        dyp, dysc = _split3_cached_dy(dy, "h2p", both=dgrad_blk)
    return xp, xsc, dyp, dysc


def conv_bwd_weight(x, dy, dw, dbias, kh, kw, stride=1, pad=0, dil=1, stem4=False, groups=1):
    """dw: destination tensor (physical OHWI, or packed [O][7][8][4] for the stem)."""
    Cout, Cin = dy.shape[-1], x.shape[-1]
    _refuse_placeholder(x, "conv_bwd_weight (fp32 input)")
    _refuse_placeholder(dy, "conv_bwd_weight (fp32 output gradient)")
    L = Layer(x.shape, Cout, kh, kw, stride, pad, dil, groups, ld_of(x), ld_of(dy), yshape=dy.shape, stem4=stem4, w4d=dw.dim() == 4,
              x_amax=amax_of(x) is not None, dy_amax=amax_of(dy) is not None)
    route = wgrad_route(L)
    _h2_only_guard(x, route, "conv_bwd_weight outside the blocked f16x2 route")
    flops = 2.0 * rows_of(dy) * Cout * (3 if stem4 else Cin // groups) * kh * kw
    if route in (D3H, D3):
        dwgrad3(x, dy, dw, dbias, flops)
        return dw
    if route == P1R:
        need = lib.catseg_pconv1_wgrad_workspace(rows_of(dy), Cout, Cin)
        ws = workspace(need + 256 * Cout * 4, x.device)
        with _Timed("wgrad_p1", flops):
            check(lib.catseg_pconv1_wgrad(rows_of(dy), Cout, Cin, ptr(dy), ld_of(dy), ptr(amax_of(dy)), ptr(x), ld_of(x), ptr(amax_of(x)), ptr(dw),
                                          ptr(ws), need, stream()))
    elif route == S2P:
        d = make_desc(x.shape, ld_of(x), Cout, ld_of(dy), kh, kw, stride, pad, dil)
        need = lib.catseg_gconv_wgrad_workspace(ctypes.byref(d))
        ws = workspace(need + 256 * Cout * 4, x.device)
        with _Timed("wgrad_s2p", flops):
            check(lib.catseg_gconv_bwd_weight(ctypes.byref(d), ptr(dy), ptr(amax_of(dy)), ptr(x), ptr(amax_of(x)), ptr(dw), ptr(ws), need, stream()))
    elif route.kind in ("h2", "b3"):
        d = make_desc(x.shape, Cin, Cout, (Cout + 7) // 8 * 8, kh, kw, stride, pad, dil)
        dgrad_blk = dgrad_route(L).blocked     # the layer's backward-data will read BLOCKED planes of dy: this split pass writes them as well
        if route.kind == "h2":
            # two fp16 planes per operand (csrc/igemm_f16x2.hip; each operand's planes behind one 32-bit-offset buffer resource); dy's
            # blocked planes for this layer's backward-data from the same pass
            kind, operands = "wgrad_h2", OPERANDS_F16X2_BLOCKED if H2T_BLOCKED else OPERANDS_F16X2
            ws = _wgrad_workspace(d, operands, 256 * Cout * 4, x.device)
            with _Timed("split3", 0.0):
                xp, xsc, dyp, dysc = _wgrad_h2_planes(x, dy, dgrad_blk)
        else:
            kind, operands, xsc, dysc = "wgrad_b3", OPERANDS_BF16X3, None, None
            ws = _wgrad_workspace(d, operands, 256 * Cout * 4, x.device)
            with _Timed("split3", 0.0):
                xp = _split3_cached(x, "planar")
                dyp = _split3_cached_dy(dy, "planar", both=dgrad_blk)
        with _Timed(kind, flops):
            _conv_call(ConvBwdWeightDesc, d, operands, x=xp, x_scale=xsc, dy=dyp, dy_scale=dysc, dw=dw, workspace=ws, workspace_bytes=ws.numel())
    else:
        d = make_desc(x.shape, ld_of(x), Cout, ld_of(dy), kh, kw, stride, pad, dil, stem4, groups)
        ws = _wgrad_workspace(d, OPERANDS_F32, 0, x.device)
        with _Timed("wgrad", flops):
            _conv_call(ConvBwdWeightDesc, d, OPERANDS_F32, x=x, dy=dy, dw=dw, dbias=dbias, workspace=ws, workspace_bytes=ws.numel())
        return dw
    if dbias is not None:
        check(lib.catseg_bias_grad(ptr(dy), ld_of(dy), rows_of(dy), Cout, ptr(dbias), ptr(ws), ws.numel(), stream()))
    return dw


def dwgrad3(x, dy, dw, dbias=None, flops=0.0):
    """backward-weight of a 3x3 / stride 1 / pad 1 trunk convolution through the direct split-precision kernel"""
    B, H, W, C = x.shape
    need = lib.catseg_dwgrad3_workspace(B, H, W, C)
    ws = workspace(need + 256 * C * 4, x.device)
    rx, rd = (amax_of(x), amax_of(dy)) if _trunk_h2() else (None, None)
    if rx is not None and rd is not None:      # both operands carry their producers' amax records: two fp16 planes, three products
        with _Timed("wgrad_d3h", flops or 2.0 * B * H * W * C * C * 9):
            check(lib.catseg_dwgrad3_f16x2(B, H, W, C, ptr(x), ld_of(x), ptr(rx), ptr(dy), ld_of(dy), ptr(rd), ptr(dw), ptr(ws), need, stream()))
    else:
        with _Timed("wgrad_d3", flops or 2.0 * B * H * W * C * C * 9):
            check(lib.catseg_dwgrad3(B, H, W, C, ptr(x), ld_of(x), ptr(dy), ld_of(dy), ptr(dw), ptr(ws), need, stream()))
    if dbias is not None:
        check(lib.catseg_bias_grad(ptr(dy), ld_of(dy), rows_of(dy), C, ptr(dbias), ptr(ws), ws.numel(), stream()))
    return dw


NT, NN, TN = 0, 1, 2


def gemm(layout, batch, M, N, K, A, lda, sA, Bm, ldb, sB, Cm, ldc, sC, zero_to=0, accumulate=False):
    check(lib.catseg_gemm_batched(layout, batch, M, N, K, ptr(A), lda, sA, ptr(Bm), ldb, sB, ptr(Cm), ldc, sC, zero_to,
                                  1 if accumulate else 0, stream()))
    return Cm


GEMM_TN_SPLIT = _plan.get("gemm_tn_split")


def tn_splits(M, N, K):
    """row chunks of a long reduction into a small M x N result: the largest divisor of K up to 32 that leaves chunks of >= 512 rows (a
    multiple of 4: the chunk's byte offset stays 16-byte aligned); 1 = do not split (short K, a large result, no suitable divisor)"""
    if K >= 4096 and M * N <= 64 * 1024:
        for s in (32, 24, 20, 16, 15, 12, 10, 8, 6, 5, 4, 3, 2):
            if K % s == 0 and K // s >= 512 and (K // s) % 4 == 0:
                return s
    return 1


def gemm_tn_split(batch, M, N, K, A, lda, Bm, ldb, Cm, accumulate=False):
    """C[b] (+)= A[b]^T B[b] for a LONG reduction K into a SMALL result M x N (the OCR head: all H * W pixels of an image into K_classes x C;
    models/OCR.py:158-170, and the value / key gradients of :266-274): with one block chain per (image, column tile) the 32 640-row
    reduction of the bench shape runs on 64 of the chip's 256 CUs for ~2 ms; the rows are cut into `splits` chunks that run as batch * splits
    independent GEMMs and are summed in a fixed order (catseg_sum_slabs).  A, Bm: [batch, K, ld] contiguous; Cm: [batch, M, N] contiguous."""
    splits = tn_splits(M, N, K) if GEMM_TN_SPLIT else 1
    if splits == 1:
        return gemm(TN, batch, M, N, K, A, lda, K * lda, Bm, ldb, K * ldb, Cm, N, M * N, accumulate=accumulate)
    kc = K // splits
    part = torch.empty((batch * splits, M, N), dtype=torch.float32, device=Cm.device)
    gemm(TN, batch * splits, M, N, kc, A, lda, kc * lda, Bm, ldb, kc * ldb, part, N, M * N)
    check(lib.catseg_sum_slabs(ptr(part), ptr(Cm), M * N, splits, batch, 1 if accumulate else 0, stream()))
    return Cm


def bn_train_stats(y, gamma, eps, momentum, running_mean, running_var):
    C = y.shape[-1]
    rows = rows_of(y)
    stats = torch.empty(2 * C, dtype=torch.float32, device=y.device)
    scale = torch.empty(C, dtype=torch.float32, device=y.device)
    ws = workspace(lib.catseg_bn_workspace(rows, C), y.device)
    check(lib.catseg_bn_train_stats(ptr(y), rows, C, ld_of(y), ptr(gamma), eps, momentum, ptr(running_mean),
                                    ptr(running_var), ptr(stats), ptr(scale), ptr(ws), ws.numel(), stream()))
    return stats, scale


def bn_eval_scale(gamma, running_var, eps):
    scale = torch.empty_like(gamma)
    check(lib.catseg_bn_eval_scale(gamma.numel(), ptr(gamma), ptr(running_var), eps, ptr(scale), stream()))
    return scale


# The ReLU mask of a residual block's output as bits (csrc/norm.hip: the mask field of catseg_bn_apply / catseg_bn_backward): the BatchNorm backward of
# z = relu(bn(y) + residual) reads 1 bit per element instead of z in both of its passes.  CATSEG_RELU_BITS=0: z is read, as before.
RELU_BITS = _plan.get("relu_bits")


def relu_bits_ok(y, residual, relu, out):
    return bool(RELU_BITS and relu and residual is not None and y.is_cuda and y.shape[-1] % 8 == 0 and ld_of(y) % 4 == 0
                and (out is None or ld_of(out) % 4 == 0))


def _ld(t):
    return 0 if t is None else ld_of(t)


def bn_apply(y, mean, scale, beta, residual, relu, out=None, planes_rec=None, planes_only=False, want_mask=False, want_record=True):
    """the output carries an amax record (out._amax: max|out| accumulated by the kernel) when the trunk runs the f16x2 kernels -- unless
    want_record is False (a frozen BatchNorm: engine.conv_bn_act).
    planes_rec (the record bn_finalize(bound=...) left the bound in): the kernel also writes the fp16 x 2 planes of the output (out._planes);
    planes_only: and NOT the fp32 output -- `out` is then an unwritten placeholder that only plane-streaming kernels may consume"""
    rows, C = rows_of(y), y.shape[-1]
    planes = planes_rec is not None
    if out is None:
        out = torch.empty(y.shape, dtype=torch.float32, device=y.device)
    buf = torch.empty(lib.catseg_planes_bytes(rows, C), dtype=torch.uint8, device=y.device) if planes else None
    mask = None
    if want_mask and not (planes and planes_only) and relu_bits_ok(y, residual, relu, out):
        mask = torch.empty(lib.catseg_bn_mask_bytes(rows, C), dtype=torch.uint8, device=y.device)
    rec = planes_rec if planes else new_amax(y.device) if (_trunk_h2() and want_record) else None
    d = BnApplyDesc(y=ptr(y), ldy=ld_of(y), mean=ptr(mean), scale=ptr(scale), beta=ptr(beta), residual=ptr(residual), ldr=_ld(residual),
                    residual_record=ptr(amax_of(residual)) if planes and residual is not None else None,
                    z=None if planes and planes_only else ptr(out), ldz=ld_of(out), z_planes=ptr(buf), rows=rows, C=C, relu=1 if relu else 0,
                    record=ptr(rec), mask=ptr(mask))
    # algorithmic bytes: y (+ residual) read, z written unless planes only, planes written (4 B / element, like fp32)
    with _Timed("hbm:bn_apply", 4.0 * y.numel() * ((3 if residual is not None else 2) + (1 if planes and not planes_only else 0))):
        check(lib.catseg_bn_apply(ctypes.byref(d), stream()))
    if rec is not None:
        out._amax = rec
    if planes:
        out._planes = Planes(buf, planes_rec, y.shape)
        out._planes_only = bool(planes_only)
    if mask is not None:
        out._relu_mask = mask
    return out


def _relu_source(z, relu, beta):
    """the ReLU fields of a catseg_bn_backward_desc: a z that carries its mask as bits (bn_apply(want_mask=True)) is not read, the bits are"""
    mask = getattr(z, "_relu_mask", None) if (z is not None and relu) else None
    if mask is not None:
        return dict(relu=1, mask=ptr(mask))
    return dict(relu=1 if relu else 0, z=ptr(z), ldz=_ld(z), beta=ptr(beta))


_CONV_ENTRY = {ConvFwdDesc: "catseg_conv2d_fwd", ConvBwdDataDesc: "catseg_conv2d_bwd_data", ConvBwdWeightDesc: "catseg_conv2d_bwd_weight"}


def _conv_call(Desc, geo, operands, **fields):
    """one catseg_conv2d_fwd / _bwd_data / _bwd_weight call (by the descriptor type): tensors in `fields` go in as their pointers, a field left
    out is NULL / 0"""
    d = Desc(geo=geo, operands=operands, **{k: v if isinstance(v, int) else ptr(v) for k, v in fields.items()})
    check(getattr(lib, _CONV_ENTRY[Desc])(ctypes.byref(d), stream()))


def _wgrad_workspace(geo, operands, extra, device):
    """the workspace of a backward-weight call + `extra` bytes (the bias-gradient partials of catseg_bias_grad behind a plane kernel)"""
    return workspace(lib.catseg_conv2d_bwd_weight_workspace(ctypes.byref(geo), operands) + extra, device)


def _bn_backward_call(dz, y, stats, gamma, dgamma, dbeta, passes, ws_bytes=None, **fields):
    """one catseg_bn_backward call: the fields every form fills and the workspace here, the ReLU source, the residual branch, the records and
    the output in `fields`.  passes: the algorithmic bytes, in tensors of y's size"""
    rows, C = rows_of(y), y.shape[-1]
    ws = workspace(ws_bytes or lib.catseg_bn_workspace(rows, C), y.device)
    d = BnBackwardDesc(dz=ptr(dz), lddz=ld_of(dz), y=ptr(y), ldy=ld_of(y), stats=ptr(stats), gamma=ptr(gamma), rows=rows, C=C, dgamma=ptr(dgamma),
                       dbeta=ptr(dbeta), workspace=ptr(ws), workspace_bytes=ws.numel(), **fields)
    with _Timed("hbm:bn_backward", 4.0 * y.numel() * passes):
        check(lib.catseg_bn_backward(ctypes.byref(d), stream()))


def bn_backward_planes(dz, z, y, stats, gamma, relu, dgamma, dbeta, dres, dres_accumulate, beta, y_rec):
    """bn_backward whose result exists as planes only (returned: Planes); y_rec: the forward convolution's max|y| record"""
    buf = torch.empty(lib.catseg_planes_bytes(rows_of(y), y.shape[-1]), dtype=torch.uint8, device=y.device)
    rec, grec = new_amax(y.device), new_amax(y.device)
    _bn_backward_call(dz, y, stats, gamma, dgamma, dbeta, 5 + (1 if dres is not None else 0), dy_planes=ptr(buf), dy_record=ptr(rec), g_record=ptr(grec),
                      y_record=ptr(y_rec), dres=ptr(dres), lddres=_ld(dres), dres_accumulate=1 if dres_accumulate else 0, **_relu_source(z, relu, beta))
    return Planes(buf, rec, y.shape)


def bn_backward_pre_planes(g, q, stats, gamma, pre, y_rec, dgamma, dbeta):
    """bn_backward_pre (g already masked, its per-wave sums and max|g| from catseg_dconv3_pl_bnbwd: pre = (partials, rows, g_record)) whose
    result exists as planes only"""
    part, nr, grec = pre
    buf = torch.empty(lib.catseg_planes_bytes(rows_of(q), q.shape[-1]), dtype=torch.uint8, device=q.device)
    rec = new_amax(q.device)
    _bn_backward_call(g, q, stats, gamma, dgamma, dbeta, 3, partials=ptr(part), n_blocks=nr, dy_planes=ptr(buf), dy_record=ptr(rec), g_record=ptr(grec),
                      y_record=ptr(y_rec))
    return Planes(buf, rec, q.shape)


def conv_bwd_data_pl(dyp, w, out, accumulate=False, bn_src=None, with_pre=False):
    """backward-data of a trunk 3x3 convolution from the planes of dy; bn_src as in conv_bwd_data: then returns
    (g, (partials, rows, g_record)) for bn_backward_pre(_planes); with_pre as in conv_bwd_data"""
    B, H, W, C = dyp.shape
    wimg = _wi.weight_image(w, "d3", True, h2=True)
    flops = 2.0 * B * H * W * C * C * 9
    drop_amax(out)
    if bn_src is not None and BN_BWD_FUSE and not accumulate:
        q, stats, gamma, beta = bn_src
        nr = lib.catseg_dconv3_pl_rows(C, B, H, W)
        part = torch.empty(2 * nr * C, dtype=torch.float32, device=out.device)
        grec = new_amax(out.device)
        with _Timed("dgrad_d3p", flops):
            check(lib.catseg_dconv3_pl_bnbwd(B, H, W, C, ptr(dyp.buf), ptr(dyp.rec), ptr(wimg[0]), ptr(wimg[1]), ptr(out), ld_of(out), ptr(q), ld_of(q),
                                             ptr(stats), ptr(gamma), ptr(beta), ptr(part), part.numel(), ptr(grec), stream()))
        return out, (part, nr, grec)
    with _Timed("dgrad_d3p", flops):
        dconv3_pl(dyp, wimg, None, out=out, accumulate=accumulate)
    return (out, None) if with_pre else out


def bn_backward(dz, z, y, stats, gamma, relu, dgamma, dbeta, dres=None, dres_accumulate=False, dy_out=None, beta=None):
    """z=None (only without a residual branch): the ReLU mask is recomputed from y and beta instead of being read; a z that carries its mask as
    bits (bn_apply(want_mask=True)) is not read either"""
    if dy_out is None:
        dy_out = torch.empty(y.shape, dtype=torch.float32, device=y.device)
    rec = new_amax(y.device) if _trunk_h2() else None
    # algorithmic bytes: two passes over (dz, y [or z, or its mask]) + dy written (+ the residual gradient)
    _bn_backward_call(dz, y, stats, gamma, dgamma, dbeta, 5 + (1 if dres is not None else 0), dy=ptr(dy_out), lddy=ld_of(dy_out), dy_record=ptr(rec),
                      dres=ptr(dres), lddres=_ld(dres), dres_accumulate=1 if dres_accumulate else 0, **_relu_source(z, relu, beta))
    if rec is not None:
        dy_out._amax = rec
    return dy_out


def bn_backward_frozen(dz, z, y, running_mean, running_var, eps, scale, relu, dgamma, dbeta, dres=None, dres_accumulate=False, dy_out=None, beta=None):
    """bn_backward of a BatchNorm whose statistics are constants of the layer (engine.BatchNorm2d.frozen): the forward was bn_apply with
    running_mean and `scale` = bn_eval_scale(gamma, running_var, eps); one streaming pass, dy = g * scale.  z / beta select the ReLU mask
    source as in bn_backward; dgamma and dbeta may both be None (no sums, y read only for a recomputed mask)"""
    if dy_out is None:
        dy_out = torch.empty(y.shape, dtype=torch.float32, device=y.device)
    rec = new_amax(y.device) if _trunk_h2() else None
    # algorithmic bytes: dz and y (or z, or its mask) read once, dy written (+ the residual gradient)
    _bn_backward_call(dz, y, None, None, dgamma, dbeta, 3 + (1 if dres is not None else 0), dy=ptr(dy_out), lddy=ld_of(dy_out), dy_record=ptr(rec),
                      dres=ptr(dres), lddres=_ld(dres), dres_accumulate=1 if dres_accumulate else 0, frozen=1, running_mean=ptr(running_mean),
                      running_var=ptr(running_var), eps=eps, scale=ptr(scale), **_relu_source(z, relu, beta))
    if rec is not None:
        dy_out._amax = rec
    return dy_out


# The HRNet head input -- torch.cat of branch 0 and the bilinearly upsampled branches 1..3 (models/HRNetv2.py:505-508) -- feeds nothing but the two
# 3 x 3 head convolutions on the f16x2 kernels: ONE launch interpolates, splits and writes the blocked planes (csrc/igemm_f16x2.hip:
# concat_bilinear_split2h_kernel); the fp32 concatenation, the copy of branch 0 into it and the split pass over it are gone.
# CATSEG_CONCAT_PLANES=0: fp32 concatenation + catseg_split2h, as before.
CONCAT_PLANES = _plan.get("concat_planes")


def concat_planes_route(ys, consumers):
    """True when every consumer (the Conv2d modules that read the concatenation of `ys` at ys[0]'s size) runs forward AND backward-weight on
    blocked f16x2 planes of its input: the concatenation then never needs to exist in fp32"""
    if not (CONCAT_PLANES and consumers and 1 <= len(ys) <= 4):
        return False
    if not all(y.is_cuda and y.dim() == 4 and y.shape[-1] % 16 == 0 and ld_of(y) % 4 == 0 and amax_of(y) is not None and y.shape[0] == ys[0].shape[0]
               for y in ys):
        return False
    B, H, W, _ = ys[0].shape
    Cin, rows = sum(y.shape[-1] for y in ys), B * H * W
    if 4 * rows * Cin >= B3_PLANE_LIMIT:
        return False
    for conv in consumers:
        _, Cout, kh, kw, st, pd, dl, groups, bias = conv_args(conv)
        if (conv.in_channels != Cin or getattr(conv, "exact_operands", False) or getattr(conv, "stem", False) or groups != 1
                or conv_out_size(H, kh, st, pd, dl) != H or conv_out_size(W, kw, st, pd, dl) != W):
            return False
        L = Layer((B, H, W, Cin), Cout, kh, kw, st, pd, dl, bias=bias is not None)      # (the concatenation carries no amax record and no planes)
        if fwd_route(L) != H2_BLOCKED or wgrad_route(L) != H2_BLOCKED:
            return False
    return True


def concat_bilinear_h2(ys, Ho, Wo):
    """(blocked planes [2, sum C / 16, B Ho Wo, 16], scale record) of cat_i(bilinear(y_i -> Ho x Wo, align_corners=False))"""
    n, B, dev = len(ys), ys[0].shape[0], ys[0].device
    C, rows = sum(y.shape[-1] for y in ys), B * Ho * Wo
    blk = torch.empty((2, C // 16, rows, 16), dtype=torch.int16, device=dev)
    scale = torch.empty(2, dtype=torch.int32, device=dev)
    PA, IA = ctypes.c_void_p * 4, ctypes.c_int * 4
    pad = lambda v: list(v) + [0] * (4 - n)
    xs, recs = PA(*pad([ptr(y) for y in ys])), PA(*pad([ptr(amax_of(y)) for y in ys]))
    lds, Hs, Ws, Cs = IA(*pad([ld_of(y) for y in ys])), IA(*pad([y.shape[1] for y in ys])), IA(*pad([y.shape[2] for y in ys])), IA(*pad([y.shape[-1] for y in ys]))
    with _Timed("hbm:bilinear_fwd", 4.0 * (sum(y.numel() for y in ys) + rows * C)):
        check(lib.catseg_concat_bilinear_split2h(n, xs, lds, Hs, Ws, Cs, recs, B, Ho, Wo, ptr(blk), ptr(scale), stream()))
    return blk, scale


def register_h2_planes(x, blk, scale):
    """x: an UNWRITTEN fp32 placeholder whose contents exist as the blocked planes (blk, scale).  The planes travel with the tensor (they live
    as long as the tape holds it: a second forward pass before this one's backward does not release them); _split3_cached hands them to the
    f16x2 kernels where a split pass of x would have run; every fp32 route refuses x"""
    x._h2_only = True
    x._h2_planes = (blk, scale)


# The head layers (conv -> BatchNorm -> ReLU on the f16x2 kernels: models/OCR.py:72-89, 326-333): the BatchNorm backward writes dy straight
# as the blocked fp16 x 2 planes that the layer's backward-weight AND backward-data read (csrc/norm.hip: bn_bwd_apply_h2_kernel) -- no fp32 dy,
# no split pass over it, the bias gradient from the same pass.  CATSEG_HEAD_DY_PLANES=0: fp32 dy + catseg_split2h, as before.
HEAD_DY_PLANES = _plan.get("head_dy_planes")


def h2_dy_route(x, y, w, kh, kw, stride, pad, dil, groups, need_dx):
    """True when conv_bwd_weight / conv_bwd_data would BOTH run this layer on the blocked f16x2 planes of dy, whether or not x and dy
    carry amax records (asked with records: that is when the pointwise / gather routes could take the layer instead)"""
    if not (HEAD_DY_PLANES and x.is_cuda and x.dim() == 4 and y.dim() == 4 and w.dim() == 4):
        return False
    Cout = y.shape[-1]
    if Cout % 64 != 0 or 4 * rows_of(y) * Cout >= B3_PLANE_LIMIT:
        return False
    L = Layer(x.shape, Cout, kh, kw, stride, pad, dil, groups, yshape=y.shape, x_amax=True, dy_amax=True)
    return wgrad_route(L) == H2_BLOCKED and (not need_dx or dgrad_route(L) == H2_BLOCKED)


def bn_backward_h2(dz, y, stats, gamma, relu, dgamma, dbeta, beta, dbias=None):
    """BatchNorm (+ ReLU, mask recomputed from y) backward without a residual branch: (blocked planes of dy, their scale record); dbias = the
    column sums of dy"""
    C, rows = y.shape[-1], rows_of(y)
    blk = torch.empty((2, C // 16, rows, 16), dtype=torch.int16, device=y.device)
    scale = torch.empty(2, dtype=torch.int32, device=y.device)
    grec, yrec, dyrec = new_amax(y.device), new_amax(y.device), new_amax(y.device)
    _bn_backward_call(dz, y, stats, gamma, dgamma, dbeta, 5, ws_bytes=lib.catseg_bn_backward_h2_workspace(rows, C), relu=1 if relu else 0, beta=ptr(beta),
                      dy_h2_planes=ptr(blk), dy_h2_scale=ptr(scale), dbias=ptr(dbias), g_record=ptr(grec), y_record=ptr(yrec), dy_record=ptr(dyrec))
    return blk, scale


HEAD_FUSE = _plan.get("head_fuse")


def head_fuse_ok(y, K):
    """the classifier behind a head's BatchNorm + ReLU runs fused with it (csrc/headfuse.h): C % 64 == 0 up to 512 channels, at most 32 classes"""
    C = y.shape[-1]
    return bool(HEAD_FUSE and y.is_cuda and y.dim() == 4 and C % 64 == 0 and C <= 512 and 1 <= K <= 32 and ld_of(y) % 4 == 0
                and 4 * rows_of(y) * C < B3_PLANE_LIMIT)


class DropMask:
    """one draw of a Dropout2d layer: mult [B, C] fp32 (0 or keep = 1 / (1 - p)), bits [B, C / 32] int32 (None where C % 32 != 0)"""
    __slots__ = ("mult", "bits", "keep")

    def __init__(self, mult, bits, keep):
        self.mult, self.bits, self.keep = mult, bits, keep


def _drop_tables(p, B, C, device):
    f32 = lambda v: ctypes.c_float(v).value
    p32 = f32(p)
    keep = f32(1.0 / f32(1.0 - p32)) if p32 < 1.0 else 0.0      # (the library's fp32 expression: both roundings are the fp32 operations')
    mult = torch.empty((B, C), dtype=torch.float32, device=device)
    bits = torch.empty((B, C // 32), dtype=torch.int32, device=device) if C % 32 == 0 else None
    return p32, keep, mult, bits


def dropout2d_mask(state, p, B, C):
    """draws the next mask of the layer whose 16-byte device state is `state` (int32 [4]: seed lo, seed hi, layer | rank << 16, draw counter)
    and advances the counter, in one launch (csrc/dropout.hip) -> DropMask"""
    p32, keep, mult, bits = _drop_tables(p, B, C, state.device)
    with _Timed("dropout2d_mask", 0.0):
        check(lib.catseg_dropout2d_mask(ptr(state), p32, B, C, ptr(mult), ptr(bits), stream()))
    return DropMask(mult, bits, keep)


def dropout2d_mask_fixed(keep01, p):
    """DropMask from a given [B, C] table of zeros and ones (fp32) instead of a draw"""
    B, C = keep01.shape
    p32, keep, mult, bits = _drop_tables(p, B, C, keep01.device)
    with _Timed("dropout2d_mask", 0.0):
        check(lib.catseg_dropout2d_mask_fixed(ptr(keep01), p32, B, C, ptr(mult), ptr(bits), stream()))
    return DropMask(mult, bits, keep)


def dropout2d_apply(x, drop, out=None):
    """out = x * drop.mult[image, channel] over an NHWC tensor (out may be x): forward and backward of Dropout2d as a pass of its own"""
    B, H, W, C = x.shape
    if out is None:
        out = torch.empty(x.shape, dtype=torch.float32, device=x.device)
    with _Timed("hbm:dropout2d_apply", 4.0 * x.numel() * 2):
        check(lib.catseg_dropout2d_apply(ptr(x), ld_of(x), ptr(drop.mult), B * H * W, C, H * W, ptr(out), ld_of(out), stream()))
    return drop_amax(out)


def head_fwd(y, mean, scale, beta, wh, bh, K, ld, drop=None):
    """logits [B, H, W, K] (pixel stride ld, zero padded) = relu(bn(y)) wh^T + bh; the normalised activation is not written.
    drop (a DropMask): Dropout2d between the ReLU and the classifier, applied in registers"""
    B, H, W, C = y.shape
    buf = torch.empty((B, H, W, ld), dtype=torch.float32, device=y.device)
    rows = rows_of(y)
    if drop is not None:
        with _Timed("hbm:head_fwd_drop", 4.0 * y.numel()):
            check(lib.catseg_head_fwd_drop(ptr(y), ld_of(y), ptr(mean), ptr(scale), ptr(beta), ptr(wh), ptr(bh), K, rows, C, ptr(buf), ld, min(ld, 32),
                                           ptr(drop.bits), H * W, drop.keep, stream()))
        return buf[..., :K] if ld != K else buf
    with _Timed("hbm:head_fwd", 4.0 * y.numel()):
        check(lib.catseg_head_fwd(ptr(y), ld_of(y), ptr(mean), ptr(scale), ptr(beta), ptr(wh), ptr(bh), K, rows, C, ptr(buf), ld, min(ld, 32),
                                  stream()))
    return buf[..., :K] if ld != K else buf


def head_backward(dl, y, stats, gamma, beta, wh, dwh, dbh, dgamma, dbeta, dbias=None, drop=None):
    """backward of head_fwd: (blocked planes of dy, their scale record) as bn_backward_h2 returns them; dwh / dbh / dgamma / dbeta / dbias written"""
    C, rows, K = y.shape[-1], rows_of(y), wh.shape[0]
    if ld_of(dl) < 32 or ld_of(dl) % 4:        # (a caller's dense gradient: the kernels read 128-byte rows)
        padded = new_act(dl.shape[0], dl.shape[1], dl.shape[2], K, dl.device, ld=32, zero=True)
        padded.copy_(dl)
        dl = padded
    blk = torch.empty((2, C // 16, rows, 16), dtype=torch.int16, device=y.device)
    scale = torch.empty(2, dtype=torch.int32, device=y.device)
    ws = workspace(lib.catseg_head_backward_workspace(rows, C), y.device)
    grec, yrec, dyrec = new_amax(y.device), new_amax(y.device), new_amax(y.device)
    if drop is not None:
        with _Timed("hbm:head_backward_drop", 4.0 * y.numel() * 3):
            check(lib.catseg_head_backward_drop(ptr(dl), ld_of(dl), ptr(y), ld_of(y), ptr(stats), ptr(gamma), ptr(beta), ptr(wh), K, rows, C, ptr(blk),
                                                ptr(scale), ptr(dgamma), ptr(dbeta), ptr(dbias), ptr(dwh), ptr(dbh), ptr(grec), ptr(yrec), ptr(dyrec),
                                                ptr(ws), ws.numel(), ptr(drop.bits), y.shape[1] * y.shape[2], drop.keep, stream()))
        return blk, scale
    with _Timed("hbm:head_backward", 4.0 * y.numel() * 3):
        check(lib.catseg_head_backward(ptr(dl), ld_of(dl), ptr(y), ld_of(y), ptr(stats), ptr(gamma), ptr(beta), ptr(wh), K, rows, C, ptr(blk),
                                       ptr(scale), ptr(dgamma), ptr(dbeta), ptr(dbias), ptr(dwh), ptr(dbh), ptr(grec), ptr(yrec), ptr(dyrec),
                                       ptr(ws), ws.numel(), stream()))
    return blk, scale


def conv_bwd_weight_h2(x, dyp, dysc, Cout, dw, kh, kw, stride, pad, dil):
    """backward-weight from the blocked planes of dy (bn_backward_h2) and of x (kept from the forward pass, or split now)"""
    Cin = x.shape[-1]
    d = make_desc(x.shape, Cin, Cout, (Cout + 7) // 8 * 8, kh, kw, stride, pad, dil)
    wsb = _wgrad_workspace(d, OPERANDS_F16X2_BLOCKED, 256 * Cout * 4, x.device)
    with _Timed("split3", 0.0):
        xp, xsc = _split3_cached(x, "h2")
    with _Timed("wgrad_h2", 2.0 * d.B * d.Ho * d.Wo * Cout * Cin * kh * kw):
        _conv_call(ConvBwdWeightDesc, d, OPERANDS_F16X2_BLOCKED, x=xp, x_scale=xsc, dy=dyp, dy_scale=dysc, dw=dw, workspace=wsb,
                   workspace_bytes=wsb.numel())
    return dw


def conv_bwd_data_h2(dyp, dysc, w, xshape, Cout, kh, kw, pad, dil, out, accumulate):
    """backward-data (stride 1) from the blocked planes of dy"""
    B, H, W, Cin = xshape
    drop_amax(out)
    d = make_desc(xshape, ld_of(out), Cout, (Cout + 7) // 8 * 8, kh, kw, 1, pad, dil)
    with _Timed("split3", 0.0):
        wtp, wtsc = _wi.weight_image(w, "h2", True)
    with _Timed("dgrad_h2", 2.0 * d.B * d.Ho * d.Wo * Cout * Cin * kh * kw):
        _conv_call(ConvBwdDataDesc, d, OPERANDS_F16X2_BLOCKED, dy=dyp, dy_scale=dysc, w=wtp, w_scale=wtsc, dx=out, accumulate=1 if accumulate else 0)
    return out


def bn_backward_pre(g, q, stats, gamma, partials, dgamma, dbeta, dq_out=None):
    """backward of relu(bn(q)) from the masked gradient g and the per-tile sums (partials, n_tiles) that conv_bwd_data(bn_src=...)
    returned: merge + apply pass only"""
    part, nt = partials[:2]
    if dq_out is None:
        dq_out = torch.empty(q.shape, dtype=torch.float32, device=q.device)
    rec = new_amax(q.device) if _trunk_h2() else None
    # one pass: g and q read, dq written
    _bn_backward_call(g, q, stats, gamma, dgamma, dbeta, 3, partials=ptr(part), n_blocks=nt, dy=ptr(dq_out), lddy=ld_of(dq_out), dy_record=ptr(rec))
    if rec is not None:
        dq_out._amax = rec
    return dq_out


def nchw3_to_nhwc4(x):
    B, C, H, W = x.shape
    assert C == 3 and x.is_contiguous() and x.dtype == torch.float32
    y = torch.empty((B, H, W, 4), dtype=torch.float32, device=x.device)
    check(lib.catseg_nchw3_to_nhwc4(ptr(x), ptr(y), B, H, W, stream()))
    return y


IMAGENET_MEAN, IMAGENET_STD = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)


def nchw3_to_nhwc4_norm(x, mean=IMAGENET_MEAN, std=IMAGENET_STD):
    """torchvision Normalize(mean, std) of an NCHW frame, written in the stem's NHWC-4 layout: ((x - mean) / std, 4th channel 0), one pass"""
    B, C, H, W = x.shape
    assert C == 3 and x.is_contiguous() and x.dtype == torch.float32 and len(mean) == 3 and len(std) == 3
    y = torch.empty((B, H, W, 4), dtype=torch.float32, device=x.device)
    check(lib.catseg_nchw3_to_nhwc4_norm(ptr(x), ptr(y), B, H, W, (ctypes.c_float * 3)(*mean), (ctypes.c_float * 3)(*std), stream()))
    return y


def stem_pack_weight(w, O):
    pk = torch.empty((O, 7, 8, 4), dtype=torch.float32, device=w.device)
    check(lib.catseg_stem_pack_weight(ptr(w), ptr(pk), O, stream()))
    return pk


def stem_unpack_grad(pk, dw, O):
    check(lib.catseg_stem_unpack_grad(ptr(pk), ptr(dw), O, stream()))
    return dw


def axpy(src, dst, alpha=1.0, accumulate=True):
    drop_amax(dst)
    check(lib.catseg_axpy2d(ptr(src), ld_of(src), ptr(dst), ld_of(dst), rows_of(src), src.shape[-1], alpha,
                            1 if accumulate else 0, stream()))
    return dst


def scale_by_device_scalar(x, s):
    """x *= s (s: 0-dim / 1-element device tensor), in place"""
    assert x.is_contiguous() and s.numel() == 1 and s.dtype == torch.float32
    check(lib.catseg_scale_by_device_scalar(ptr(x), x.numel(), ptr(s), stream()))
    return x


def bias_grad(dy, C, dbias):
    """dbias[c] = sum over the rows of dy[:, c], c < C (dy: 2-D rows or NHWC)"""
    ws = workspace(256 * C * 4 + 1024, dy.device)
    check(lib.catseg_bias_grad(ptr(dy), ld_of(dy), rows_of(dy), C, ptr(dbias), ptr(ws), ws.numel(), stream()))
    return dbias


def maxpool_fwd(x):
    B, H, W, C = x.shape
    Ho, Wo = (H + 1) // 2, (W + 1) // 2
    y = torch.empty((B, Ho, Wo, C), dtype=torch.float32, device=x.device)
    idx = torch.empty((B, Ho, Wo, C), dtype=torch.uint8, device=x.device)
    check(lib.catseg_maxpool3x3s2_fwd(ptr(x), ld_of(x), ptr(y), C, ptr(idx), B, H, W, C, Ho, Wo, stream()))
    return y, idx


def maxpool_bwd(dy, idx, xshape):
    B, H, W, C = xshape
    dx = torch.empty(xshape, dtype=torch.float32, device=dy.device)
    check(lib.catseg_maxpool3x3s2_bwd(ptr(dy), ld_of(dy), ptr(idx), ptr(dx), C, B, H, W, C, dy.shape[1], dy.shape[2], stream()))
    return dx


def maxpool2_fwd(x):
    """F.max_pool2d(x, 2) (models/FCN.py:44-53 of the reference) -> (y, argmax position inside the window)"""
    B, H, W, C = x.shape
    y = torch.empty((B, H // 2, W // 2, C), dtype=torch.float32, device=x.device)
    idx = torch.empty((B, H // 2, W // 2, C), dtype=torch.uint8, device=x.device)
    check(lib.catseg_maxpool2x2_fwd(ptr(x), ld_of(x), ptr(y), C, ptr(idx), B, H, W, C, stream()))
    return y, idx


def maxpool2_bwd(dy, idx, out, accumulate=False):
    B, H, W, C = out.shape
    dst = torch.empty(out.shape, dtype=torch.float32, device=dy.device) if accumulate else out
    check(lib.catseg_maxpool2x2_bwd(ptr(dy), ld_of(dy), ptr(idx), ptr(dst), ld_of(dst), B, H, W, C, stream()))
    if accumulate:
        axpy(dst, out, 1.0, True)
    return out


# Records without BatchNorm (csrc/unet.hip).  The f16x2 direct / pointwise / gather kernels take a layer only when its input (backward: its
# output gradient) carries an amax record; in a conv + bias + ReLU network (models/UNet.py) none of the record producers above runs.  With
# the plan field `bnfree_records` the engine's recording layers (conv_act(record=), maxpool2(record=True), upcat) leave the records in the
# passes the skip junction needs anyway.  CATSEG_BNFREE_RECORDS=0: the composed passes without records (fp32 MFMA / bf16x3 routes).
# Measured (tools/time_unet.py, profiles/unet_step_time.json, one run: 8 x 3 x 544 x 960, five alternating rounds of four steps, medians):
# UNet train step 125.3 -> 82.7 ms in the launch loop, 125.2 -> 82.6 ms as hipGraph replay -- the field is on by default.
BNFREE_RECORDS = _plan.get("bnfree_records")


def bnfree_records():
    return bool(BNFREE_RECORDS and _trunk_h2())


def amax_record(x):
    """attaches the record of max|x| to x (a read-only pass over its valid columns) and returns x"""
    rec = new_amax(x.device)
    with _Timed("hbm:amax_record", 4.0 * x.numel()):
        check(lib.catseg_amax_record(ptr(x), ld_of(x), rows_of(x), x.shape[-1], ptr(rec), stream()))
    x._amax = rec
    return x


def maxpool2_fwd_rec(x):
    """maxpool2_fwd + the amax records of its input (attached to x when it has none) and of its output"""
    B, H, W, C = x.shape
    y = torch.empty((B, H // 2, W // 2, C), dtype=torch.float32, device=x.device)
    idx = torch.empty((B, H // 2, W // 2, C), dtype=torch.uint8, device=x.device)
    xrec = new_amax(x.device) if amax_of(x) is None else None
    yrec = new_amax(x.device)
    with _Timed("hbm:maxpool2_fwd_rec", 4.0 * x.numel() + 5.0 * y.numel()):
        check(lib.catseg_maxpool2x2_fwd_rec(ptr(x), ld_of(x), ptr(y), C, ptr(idx), B, H, W, C, ptr(xrec), ptr(yrec), stream()))
    if xrec is not None:
        x._amax = xrec
    y._amax = yrec
    return y, idx


def upcat2x_fwd(x, skip, record=True):
    """cat = [bilinear 2x (align_corners=True) of x, skip] along the channels in one launch; record: with the amax record of cat"""
    B, h, w, Cx = x.shape
    Cs = skip.shape[-1]
    assert tuple(skip.shape[:3]) == (B, 2 * h, 2 * w)
    cat = torch.empty((B, 2 * h, 2 * w, Cx + Cs), dtype=torch.float32, device=x.device)
    rec = new_amax(x.device) if record else None
    with _Timed("hbm:upcat2x_fwd", 4.0 * (x.numel() + skip.numel() + cat.numel())):
        check(lib.catseg_upcat2x_fwd(ptr(x), ld_of(x), ptr(skip), ld_of(skip), ptr(cat), Cx + Cs, B, h, w, Cx, Cs, ptr(rec), stream()))
    if rec is not None:
        cat._amax = rec
    return cat


def relu_bwd_rec(dz, z, pool=None, record=True):
    """g = d * (z > 0) with the amax record of g.  pool = (dpool, idx): z also fed a 2x2 max-pool, d = dz + the pooled gradient routed
    through idx (maxpool2_bwd), in the same pass; dz may be a channel slice of a wider gradient buffer"""
    B, H, W, C = z.shape
    g = torch.empty(z.shape, dtype=torch.float32, device=z.device)
    rec = new_amax(z.device) if record else None
    dpool, idx = pool if pool is not None else (None, None)
    with _Timed("hbm:relu_bwd_rec", 4.0 * 3 * z.numel() + (5.0 * dpool.numel() if dpool is not None else 0.0)):
        check(lib.catseg_relu_bwd_rec(ptr(dz), ld_of(dz), ptr(dpool), ld_of(dpool) if dpool is not None else 0, ptr(idx), ptr(z), ld_of(z), ptr(g), C,
                                      B, H, W, C, ptr(rec), stream()))
    if rec is not None:
        g._amax = rec
    return g


def widen(t):
    """the [B, H, W, ld] tensor behind a class-logit view [B, H, W, K] whose rows are zero padded to ld floats (conv_fwd(zero_to=),
    engine.Ctx.dest): the 16-byte-granular kernels run on all ld columns"""
    B, H, W, _ = t.shape
    ld = ld_of(t)
    return t if ld == t.shape[-1] else torch.as_strided(t, (B, H, W, ld), (H * W * ld, W * ld, ld, 1))


def conv_transpose_fwd(x, w, bias, Cout, k, stride, pad, ld=32):
    """nn.ConvTranspose2d(Cin, Cout, k, stride, pad) on class-logit tensors (models/FCN.py:35-38, utils/torch_utils.py:151-168 of the
    reference): y = bias + backward-data of the convolution that has the same weight tensor (physical layout [Cin][k][k][Cout] = that
    convolution's OHWI).  x: [B, H, W, Cin] view with zero-padded rows of ld floats; returns the same kind of view of the output and the
    padded weight image the backward pass reuses."""
    B, H, W, Cin = x.shape
    Ho, Wo = (H - 1) * stride - 2 * pad + k, (W - 1) * stride - 2 * pad + k
    assert ld_of(x) == ld and Cout <= ld and Cin <= ld
    wp = weight_pad_cin(w, Cin, k * k, Cout, ld)
    y = new_act(B, Ho, Wo, Cout, x.device, ld=ld, zero=True)
    if bias is not None:
        check(lib.catseg_bias_rows(ptr(bias), ptr(y), ld, rows_of(y), Cout, stream()))
    conv_bwd_data(x, wp, (B, Ho, Wo, ld), k, k, stride, pad, 1, out=widen(y), accumulate=True)
    return y, wp


def conv_transpose_bwd(dy, x, wp, dw, dbias, k, stride, pad, dx, accumulate, ld=32):
    """gradients of conv_transpose_fwd: dw = backward-weight of the same convolution with the roles of input and output gradient swapped,
    dx = that convolution's FORWARD pass over dy"""
    Cin, Cout = x.shape[-1], dy.shape[-1]
    if ld_of(dy) != ld:     # the loss hands the gradient of the network's output over as a dense [B, H, W, K] tensor: re-pitch it (a copy)
        padded = new_act(dy.shape[0], dy.shape[1], dy.shape[2], Cout, dy.device, ld=ld, zero=True)
        padded.copy_(dy)
        dy = padded
    dyw = widen(dy)
    dwp = torch.empty_like(wp)
    conv_bwd_weight(dyw, x, dwp, None, k, k, stride, pad, 1)
    weight_unpad_cin(dwp, dw, Cin, k * k, Cout, ld)
    if dbias is not None:
        ws = workspace(256 * Cout * 4 + 1024, dy.device)
        check(lib.catseg_bias_grad(ptr(dy), ld_of(dy), rows_of(dy), Cout, ptr(dbias), ptr(ws), ws.numel(), stream()))
    if dx is not None:
        dst = new_act(x.shape[0], x.shape[1], x.shape[2], Cin, x.device, ld=ld, zero=True) if accumulate else dx
        conv_fwd(dyw, wp, None, Cin, k, k, stride, pad, 1, out=dst, zero_to=ld)
        if accumulate:
            axpy(widen(dst), widen(dx), 1.0, True)


def bilinear_fwd(x, Ho, Wo, align_corners, out=None, accumulate=False):
    B, H, W, C = x.shape
    if out is None:
        out = torch.empty((B, Ho, Wo, C), dtype=torch.float32, device=x.device)
    with _Timed("hbm:bilinear_fwd", 4.0 * (x.numel() + out.numel() * (2 if accumulate else 1))):
        check(lib.catseg_bilinear_fwd(ptr(x), ld_of(x), ptr(out), ld_of(out), B, H, W, C, Ho, Wo, 1 if align_corners else 0,
                                      1 if accumulate else 0, stream()))
    if accumulate:
        drop_amax(out)
    elif amax_of(x) is not None:
        out._amax = amax_of(x)       # an interpolation with weights in [0, 1] that sum to 1: max|out| <= max|x| (the fuse sum's bound adds it)
    return out


def bilinear_bwd(dy, xshape, align_corners, out=None, zero_to=0, accumulate=False):
    B, H, W, C = xshape
    Ho, Wo = dy.shape[1], dy.shape[2]
    if out is None:
        out = new_act(B, H, W, C, dy.device, ld=max(zero_to, (C + 3) // 4 * 4))
        accumulate = False
    ws = workspace(B * H * Wo * C * 4, dy.device)
    with _Timed("hbm:bilinear_bwd", 4.0 * (dy.numel() + B * H * W * C * (2 if accumulate else 1))):
        _bilinear_bwd(dy, out, B, H, W, C, Ho, Wo, align_corners, zero_to, accumulate, ws)
    return out


def _bilinear_bwd(dy, out, B, H, W, C, Ho, Wo, align_corners, zero_to, accumulate, ws):
    check(lib.catseg_bilinear_bwd(ptr(dy), ld_of(dy), ptr(out), ld_of(out), B, H, W, C, Ho, Wo, 1 if align_corners else 0,
                                  zero_to, 1 if accumulate else 0, ptr(ws), ws.numel(), stream()))
    return out


def global_avgpool_fwd(x):
    B, H, W, C = x.shape
    y = torch.empty((B, 1, 1, C), dtype=torch.float32, device=x.device)
    check(lib.catseg_global_avgpool_fwd(ptr(x), ld_of(x), ptr(y), B, H * W, C, stream()))
    return y


def global_avgpool_bwd(dy, dx, accumulate):
    B, H, W, C = dx.shape
    check(lib.catseg_global_avgpool_bwd(ptr(dy), ptr(dx), ld_of(dx), B, H * W, C, 1 if accumulate else 0, stream()))
    return dx


def softmax_spatial_fwd(x, K):
    """x: [B, N, ld] buffer (logits in columns [0, K)); returns same-shape probabilities, pad columns zero."""
    B, N, ld = x.shape
    y = torch.empty_like(x)
    ws = workspace(lib.catseg_softmax_spatial_workspace(B, N), x.device)
    check(lib.catseg_softmax_spatial_fwd(ptr(x), ptr(y), B, N, K, ld, ptr(ws), ws.numel(), stream()))
    return y


def softmax_spatial_bwd(y, dy, dx, K, accumulate=False):
    B, N, ld = y.shape
    ws = workspace(lib.catseg_softmax_spatial_workspace(B, N), y.device)
    check(lib.catseg_softmax_spatial_bwd(ptr(y), ptr(dy), ptr(dx), B, N, K, ld, 1 if accumulate else 0, ptr(ws), ws.numel(), stream()))
    return dx


def softmax_rows_fwd(x, K, scale):
    rows, ld = x.shape
    y = torch.empty_like(x)
    check(lib.catseg_softmax_rows_fwd(ptr(x), ptr(y), rows, K, ld, scale, stream()))
    return y


def softmax_rows_bwd(y, dy, K, scale):
    rows, ld = y.shape
    dx = torch.empty_like(y)
    check(lib.catseg_softmax_rows_bwd(ptr(y), ptr(dy), ptr(dx), rows, K, ld, scale, stream()))
    return dx


def lovasz_softmax(logits, labels, weight=1.0, dlogits=None, accumulate=False, loss_out=None):
    """logits: [P, K] contiguous (NHWC flattened); labels int64 [P]."""
    Pn, K = logits.shape
    assert logits.is_contiguous() and labels.dtype == torch.int64 and labels.is_contiguous()
    if loss_out is None:
        loss_out = torch.empty(1, dtype=torch.float32, device=logits.device)
    ws = workspace(lib.catseg_lovasz_workspace(Pn, K), logits.device)
    # algorithmic minimum: logits read + gradient written (the sort passes on top are data dependent: active-set pruning)
    with _Timed("hbm:lovasz", 4.0 * Pn * K * (2 if dlogits is not None else 1) + 8.0 * Pn):
        _lovasz(logits, labels, Pn, K, weight, loss_out, dlogits, accumulate, ws)
    return loss_out


def _lovasz(logits, labels, Pn, K, weight, loss_out, dlogits, accumulate, ws):
    check(lib.catseg_lovasz_softmax(ptr(logits), ptr(labels), Pn, K, weight, ptr(loss_out), ptr(dlogits),
                                    1 if accumulate else 0, ptr(ws), ws.numel(), stream()))
    return loss_out


def lovasz_softmax_fwd(logits, labels, weight=1.0, want_grad=True):
    """forward half of lovasz_softmax for autograd: (loss, workspace) -- the workspace holds d loss / d prob for lovasz_softmax_bwd and is
    a buffer of its own (not the stream's shared scratch: other launches run between the two halves)"""
    Pn, K = logits.shape
    assert logits.is_contiguous() and labels.dtype == torch.int64 and labels.is_contiguous()
    loss_out = torch.empty(1, dtype=torch.float32, device=logits.device)
    need = lib.catseg_lovasz_workspace(Pn, K)
    ws = torch.empty(need, dtype=torch.uint8, device=logits.device) if want_grad else workspace(need, logits.device)
    with _Timed("hbm:lovasz", 4.0 * Pn * K * (2 if want_grad else 1) + 8.0 * Pn):
        check(lib.catseg_lovasz_softmax_fwd(ptr(logits), ptr(labels), Pn, K, weight, ptr(loss_out), 1 if want_grad else 0, ptr(ws), need, stream()))
    return loss_out, (ws if want_grad else None)


def lovasz_softmax_bwd(logits, ws, upstream, weight=1.0, dlogits=None, accumulate=False):
    """dlogits (+)= d loss / d logits * upstream (upstream: 1-element float32 device tensor, autograd's grad_output; None = 1)"""
    Pn, K = logits.shape
    if dlogits is None:
        dlogits = torch.empty_like(logits)
        accumulate = False
    assert upstream is None or (upstream.numel() == 1 and upstream.dtype == torch.float32 and upstream.is_cuda)
    with _Timed("hbm:lovasz", 0.0):
        check(lib.catseg_lovasz_softmax_bwd(ptr(logits), Pn, K, weight, ptr(upstream), ptr(dlogits), 1 if accumulate else 0, ptr(ws), ws.numel(), stream()))
    return dlogits


def cross_entropy(logits, labels, ignore_index, weight=1.0, dlogits=None, loss_out=None):
    Pn, K = logits.shape
    assert logits.is_contiguous() and labels.dtype == torch.int64 and labels.is_contiguous()
    if loss_out is None:
        loss_out = torch.empty(1, dtype=torch.float32, device=logits.device)
    ws = workspace(lib.catseg_ce_workspace(Pn), logits.device)
    check(lib.catseg_cross_entropy(ptr(logits), ptr(labels), Pn, K, ignore_index, weight, ptr(loss_out), ptr(dlogits),
                                   ptr(ws), ws.numel(), stream()))
    return loss_out


def ohem_cross_entropy(logits, labels, ignore_index, thresh, min_kept, weight=1.0, dlogits=None, loss_out=None):
    Pn, K = logits.shape
    assert logits.is_contiguous() and labels.dtype == torch.int64 and labels.is_contiguous()
    if loss_out is None:
        loss_out = torch.empty(1, dtype=torch.float32, device=logits.device)
    ws = workspace(lib.catseg_ohem_workspace(Pn), logits.device)
    check(lib.catseg_ohem_cross_entropy(ptr(logits), ptr(labels), Pn, K, ignore_index, thresh, min_kept, weight, ptr(loss_out),
                                        ptr(dlogits), ptr(ws), ws.numel(), stream()))
    return loss_out


def _host_floats(v, K):
    """a per-class list as a ctypes float array (passed to the kernels by value), or None"""
    if v is None:
        return None
    assert len(v) == K
    return (ctypes.c_float * K)(*[float(x) for x in v])


def overlap_fwd(logits, labels, kind, ignore_index=-1, naive=False, weight_mode=0, weights=None):
    """forward half of SoftIoU (kind 0) / GenDiceLoss (kind 1) for autograd: (loss [1], coef [128], invalid_labels int64 [1]) -- coef
    holds d loss / d prob for overlap_bwd in a buffer of its own (not the stream's shared scratch: other launches run between the halves)"""
    Pn, K = logits.shape
    assert logits.is_contiguous() and labels.dtype == torch.int64 and labels.is_contiguous() and labels.numel() == Pn
    dev = logits.device
    loss_out = torch.empty(1, dtype=torch.float32, device=dev)
    coef = torch.empty(128, dtype=torch.float32, device=dev)
    invalid = torch.empty(1, dtype=torch.int64, device=dev)
    need = lib.catseg_overlap_workspace(Pn, K)
    ws = workspace(need, dev)
    with _Timed("hbm:overlap_fwd", 4.0 * Pn * K + 8.0 * Pn):
        check(lib.catseg_overlap_fwd(ptr(logits), ptr(labels), Pn, K, ignore_index, kind, 1 if naive else 0, weight_mode,
                                     _host_floats(weights, K), ptr(loss_out), ptr(coef), ptr(invalid), ptr(ws), ws.numel(), stream()))
    return loss_out, coef, invalid


def overlap_bwd(logits, labels, coef, upstream, ignore_index=-1):
    """d loss / d logits * upstream (upstream: 1-element float32 device tensor, autograd's grad_output; None = 1)"""
    Pn, K = logits.shape
    assert upstream is None or (upstream.numel() == 1 and upstream.dtype == torch.float32 and upstream.is_cuda)
    dlogits = torch.empty_like(logits)
    with _Timed("hbm:overlap_bwd", 8.0 * Pn * K + 8.0 * Pn):
        check(lib.catseg_overlap_bwd(ptr(logits), ptr(labels), Pn, K, ignore_index, ptr(coef), ptr(upstream), ptr(dlogits), stream()))
    return dlogits


def focal_fwd(logits, labels, gamma, alpha=None):
    """FocalLoss forward: (loss [1], invalid_labels int64 [1]); alpha = per-class host list or None"""
    Pn, K = logits.shape
    assert logits.is_contiguous() and labels.dtype == torch.int64 and labels.is_contiguous() and labels.numel() == Pn
    dev = logits.device
    loss_out = torch.empty(1, dtype=torch.float32, device=dev)
    invalid = torch.empty(1, dtype=torch.int64, device=dev)
    ws = workspace(lib.catseg_focal_workspace(Pn), dev)
    with _Timed("hbm:focal_fwd", 4.0 * Pn * K + 8.0 * Pn):
        check(lib.catseg_focal_fwd(ptr(logits), ptr(labels), Pn, K, float(gamma), _host_floats(alpha, K), ptr(loss_out), ptr(invalid),
                                   ptr(ws), ws.numel(), stream()))
    return loss_out, invalid


def focal_bwd(logits, labels, gamma, alpha, upstream):
    """d focal / d logits * upstream (1-element float32 device tensor; None = 1)"""
    Pn, K = logits.shape
    assert upstream is None or (upstream.numel() == 1 and upstream.dtype == torch.float32 and upstream.is_cuda)
    dlogits = torch.empty_like(logits)
    with _Timed("hbm:focal_bwd", 8.0 * Pn * K + 8.0 * Pn):
        check(lib.catseg_focal_bwd(ptr(logits), ptr(labels), Pn, K, float(gamma), _host_floats(alpha, K), ptr(upstream), ptr(dlogits),
                                   stream()))
    return dlogits


def _label_tables(lut, tables, B):
    """(T, per-frame table index or None) for the `_tables` entry points, or None for the plain ones: lut uint8 [T,256] with
    tables DEVICE int32 [B] (None = row 0 for every frame; csrc/warp_label.h clamps the index into [0, T)); lut [256] or None: plain"""
    if lut is None or lut.dim() == 1:
        assert tables is None, "a per-frame table index needs label tables uint8 [T, 256]"
        assert lut is None or lut.numel() == 256
        return None
    assert lut.dim() == 2 and lut.shape[1] == 256 and lut.shape[0] >= 1, "label tables are uint8 [T, 256]"
    assert tables is None or (tables.dtype == torch.int32 and tables.numel() == B and tables.is_contiguous() and tables.device == lut.device)
    return int(lut.shape[0]), tables


def ingest_u8(img, lbl, lut=None, flips=None, pad_top=0, pad_bottom=0, mean=None, std=None, nhwc4=False, tables=None):
    """img uint8 [B,H,W,3] and / or lbl uint8 [B,H,W] -> (x float32 [B,3,H',W] (or NHWC-4 [B,H',W,4]), labels int64 [B,H',W]).
    tables: DEVICE int32 [B], the row of lut uint8 [T,256] every frame's labels go through (a batch of raw and already remapped label maps
    in one launch; None with such a lut: row 0 for every frame); lut [256]: one table, the plain entry point"""
    ref = img if img is not None else lbl
    B, H, W = ref.shape[:3]
    Ho = H + pad_top + pad_bottom
    for t in (img, lbl, lut):
        assert t is None or (t.dtype == torch.uint8 and t.is_contiguous() and t.is_cuda)
    tabled = _label_tables(lut, tables, B)
    assert flips is None or (flips.dtype == torch.int32 and flips.numel() == B)
    x = x4 = labels = None
    if img is not None:
        assert img.shape == (B, H, W, 3)
        if nhwc4:
            x4 = torch.empty((B, Ho, W, 4), dtype=torch.float32, device=ref.device)
        else:
            x = torch.empty((B, 3, Ho, W), dtype=torch.float32, device=ref.device)
    if lbl is not None:
        assert lbl.shape == (B, H, W)
        labels = torch.empty((B, Ho, W), dtype=torch.int64, device=ref.device)
    if tabled is not None:
        check(lib.catseg_ingest_u8_tables(ptr(img), ptr(lbl), B, H, W, ptr(lut), tabled[0], ptr(tabled[1]), ptr(flips), pad_top, pad_bottom, ptr(mean),
                                          ptr(std), ptr(x), ptr(x4), ptr(labels), stream()))
        return (x4 if nhwc4 else x), labels
    check(lib.catseg_ingest_u8(ptr(img), ptr(lbl), B, H, W, ptr(lut), ptr(flips), pad_top, pad_bottom, ptr(mean), ptr(std),
                               ptr(x), ptr(x4), ptr(labels), stream()))
    return (x4 if nhwc4 else x), labels


def _warp_matrices(minv, B, dev, who):
    """HOST canvas -> frame matrices [B,3,3] (or [B,2,3]) -> DEVICE float64 [B,6] (rows 0 and 1), or None"""
    if minv is None:
        return None
    m = np.ascontiguousarray(np.asarray(minv, dtype=np.float64)[:, :2, :])
    if m.shape != (B, 2, 3) or not np.isfinite(m).all():
        raise ValueError("%s: the inverse matrices must be finite float64 [B, 3, 3], got shape %s" % (who, np.shape(minv)))
    return torch.from_numpy(m.reshape(B, 6)).to(dev, non_blocking=True)


def ingest_warp_u8(img, lbl, lut=None, flips=None, minv=None, canvas=None, origin=None, window=None, pad_top=0, pad_bottom=0,
                   mean=None, std=None, outputs=("nchw",), tables=None):
    """ingest_u8 with the geometric augmentations fused in (csrc/warp.hip): remap -> flip -> warp onto `canvas` (Hc, Wc) -> `window`
    (Hw, Ww) of the canvas at the per-frame `origin` -> reflect pad of the rows -> ToTensor / Normalize.
    minv: HOST float64 [B,3,3] (or [B,2,3]) canvas -> frame matrices (utils.geometry.affine_inverse), None = identity on canvas = frame;
    origin: HOST int [B,2] = (v, h), None = (0, 0), or a DEVICE int32 [B,2] tensor (crop_freq_pick's result), which is passed on without a
    host check: the kernel is guarded, window pixels outside the canvas are zeros; outputs: any of "nchw", "nhwc4", "u8" (the image forms;
    ignored without img); tables: as ingest_u8 takes it (lut is then uint8 [T,256]).
    Returns {"nchw" | "nhwc4" | "u8": tensor, ..., "labels": int64 [B,H',Ww] or None}.  The host-side values are checked here (finite
    matrices, windows inside the canvas); whatever reaches the kernel regardless yields zeros, never an unguarded read."""
    ref = img if img is not None else lbl
    B, H, W = ref.shape[:3]
    dev = ref.device
    for t in (img, lbl, lut):
        assert t is None or (t.dtype == torch.uint8 and t.is_contiguous() and t.is_cuda)
    assert flips is None or (flips.dtype == torch.int32 and flips.numel() == B)
    assert set(outputs) <= {"nchw", "nhwc4", "u8"} and (img is None or len(outputs) > 0)
    tabled = _label_tables(lut, tables, B)
    Hc, Wc = (int(canvas[0]), int(canvas[1])) if canvas is not None else (H, W)
    Hw, Ww = (int(window[0]), int(window[1])) if window is not None else (Hc, Wc)
    minv_d, origin_d = _warp_matrices(minv, B, dev, "ingest_warp_u8"), None
    if isinstance(origin, torch.Tensor) and origin.is_cuda:
        assert origin.dtype == torch.int32 and tuple(origin.shape) == (B, 2) and origin.is_contiguous() and origin.device == dev
        origin_d = origin
    elif origin is not None:
        o = np.ascontiguousarray(np.asarray(origin, dtype=np.int64))
        if o.shape != (B, 2) or (o < 0).any() or (o[:, 0] + Hw > Hc).any() or (o[:, 1] + Ww > Wc).any():
            raise ValueError("ingest_warp_u8: window origins must be [B, 2] = (v, h) with the %d x %d window inside the %d x %d canvas"
                             % (Hw, Ww, Hc, Wc))
        origin_d = torch.from_numpy(o.astype(np.int32)).to(dev, non_blocking=True)
    Ho = Hw + pad_top + pad_bottom
    out = {"labels": None}
    if img is not None:
        assert img.shape == (B, H, W, 3)
        if "nchw" in outputs:
            out["nchw"] = torch.empty((B, 3, Ho, Ww), dtype=torch.float32, device=dev)
        if "nhwc4" in outputs:
            out["nhwc4"] = torch.empty((B, Ho, Ww, 4), dtype=torch.float32, device=dev)
        if "u8" in outputs:
            out["u8"] = torch.empty((B, Ho, Ww, 3), dtype=torch.uint8, device=dev)
    if lbl is not None:
        assert lbl.shape == (B, H, W)
        out["labels"] = torch.empty((B, Ho, Ww), dtype=torch.int64, device=dev)
    if tabled is not None:
        check(lib.catseg_ingest_warp_u8_tables(ptr(img), ptr(lbl), B, H, W, ptr(lut), tabled[0], ptr(tabled[1]), ptr(flips), ptr(minv_d), Hc, Wc,
                                               ptr(origin_d), Hw, Ww, pad_top, pad_bottom, ptr(mean), ptr(std), ptr(out.get("nchw")),
                                               ptr(out.get("nhwc4")), ptr(out.get("u8")), ptr(out["labels"]), stream()))
        return out
    check(lib.catseg_ingest_warp_u8(ptr(img), ptr(lbl), B, H, W, ptr(lut), ptr(flips), ptr(minv_d), Hc, Wc, ptr(origin_d), Hw, Ww,
                                    pad_top, pad_bottom, ptr(mean), ptr(std), ptr(out.get("nchw")), ptr(out.get("nhwc4")),
                                    ptr(out.get("u8")), ptr(out["labels"]), stream()))
    return out


def crop_freq_table(wq, device):
    """the 256-entry DEVICE weight table of crop_freq_pick from the integer class weights (utils.geometry.freq_weight_table); label values
    past the last class weigh 0"""
    wq = [int(v) for v in wq]
    if len(wq) > 256 or any(v < 0 or v >= 1 << 62 for v in wq):
        raise ValueError("crop_freq_table: at most 256 weights in [0, 2^62)")
    return torch.tensor(wq + [0] * (256 - len(wq)), dtype=torch.int64).to(device)


def crop_freq_pick(lbl, lut, flips, minv, canvas, px, wq, m53, return_debug=False, tables=None):
    """the window origins of CropNP(crop_mode='freq') on the device (csrc/cropfreq.hip): lbl uint8 [B,H,W] raw ids, lut / flips / minv / canvas
    as ingest_warp_u8 takes them (the labels weighed are the labels that launch writes); px: the window edge (utils.geometry.crop_px);
    wq: the integer class weights (a sequence of Python ints, or the device table crop_freq_table made of them); m53: per frame
    int(u * 2 ** 53) of utils.geometry.sample_freq_u's u.  Returns a DEVICE int32 [B,2] = (v, h) for ingest_warp_u8(origin=...);
    return_debug: (origins, totals int64 [B], flat region indices int64 [B]); tables: as ingest_u8 takes it (lut is then uint8 [T,256]).  Refuses (ValueError) weights whose sum over the region could
    pass 2^62."""
    from .utils.geometry import check_freq_weights, crop_freq_region
    B, H, W = lbl.shape
    dev = lbl.device
    assert lbl.dtype == torch.uint8 and lbl.is_contiguous() and lbl.is_cuda
    assert lut is None or (lut.dtype == torch.uint8 and lut.is_contiguous() and lut.is_cuda)
    tabled = _label_tables(lut, tables, B)
    assert flips is None or (flips.dtype == torch.int32 and flips.numel() == B and flips.is_cuda)
    Hc, Wc = (int(canvas[0]), int(canvas[1])) if canvas is not None else (H, W)
    px = int(px)
    if isinstance(wq, torch.Tensor):
        assert wq.dtype == torch.int64 and wq.numel() == 256 and wq.is_contiguous() and wq.device == dev
        table = wq
    else:
        _, rh, rw = crop_freq_region(Hc, Wc, px)
        check_freq_weights([int(v) for v in wq], rh * rw)
        table = crop_freq_table(wq, dev)
    m = [int(v) for v in m53]
    if len(m) != B or any(v < 0 or v >= 1 << 53 for v in m):
        raise ValueError("crop_freq_pick: m53 must hold B integers in [0, 2^53)")
    m_d = torch.tensor(m, dtype=torch.int64).to(dev, non_blocking=True)
    minv_d = _warp_matrices(minv, B, dev, "crop_freq_pick")
    origin = torch.empty((B, 2), dtype=torch.int32, device=dev)
    total = torch.empty(B, dtype=torch.int64, device=dev) if return_debug else None
    flat = torch.empty(B, dtype=torch.int64, device=dev) if return_debug else None
    nbytes = lib.catseg_crop_freq_workspace(B, Hc, Wc, px)
    ws = torch.empty(max(nbytes, 8) // 8, dtype=torch.int64, device=dev)
    if tabled is not None:
        check(lib.catseg_crop_freq_pick_tables(ptr(lbl), B, H, W, ptr(lut), tabled[0], ptr(tabled[1]), ptr(flips), ptr(minv_d), Hc, Wc, px, ptr(table),
                                               ptr(m_d), ptr(origin), ptr(total), ptr(flat), ptr(ws), nbytes, stream()))
        return (origin, total, flat) if return_debug else origin
    check(lib.catseg_crop_freq_pick(ptr(lbl), B, H, W, ptr(lut), ptr(flips), ptr(minv_d), Hc, Wc, px, ptr(table), ptr(m_d), ptr(origin),
                                    ptr(total), ptr(flat), ptr(ws), nbytes, stream()))
    return (origin, total, flat) if return_debug else origin


def label_census(lbl, nbins=36, lut=None, out=None, accumulate=False):
    """per-frame class pixel counts of raw label maps (csrc/census.hip): lbl uint8 [B,H,W] (any storage offset: no alignment is asked of
    the frames), lut uint8 [256] on the device or None = identity.  Returns DEVICE int64 [B, nbins + 1]; the last column holds the pixels
    whose (table-mapped) value is >= nbins.  out + accumulate=True adds to the counts already there (64-bit dataset totals)."""
    assert lbl.dtype == torch.uint8 and lbl.dim() == 3 and lbl.is_contiguous() and lbl.is_cuda
    assert lut is None or (lut.dtype == torch.uint8 and lut.numel() == 256 and lut.is_contiguous() and lut.device == lbl.device)
    B, H, W = lbl.shape
    nbins = int(nbins)
    if out is None:
        if accumulate:
            raise ValueError("label_census: accumulate=True needs out=")
        out = torch.empty((B, max(nbins, 0) + 1), dtype=torch.int64, device=lbl.device)
    assert out.dtype == torch.int64 and tuple(out.shape) == (B, nbins + 1) and out.is_contiguous() and out.device == lbl.device
    check(lib.catseg_label_census_u8(ptr(lbl), B, H, W, ptr(lut), nbins, ptr(out), 1 if accumulate else 0, stream()))
    return out


def iou_ema(cm_running, cm_prev, iou_values, update, iou_batch=None):
    """the per-class IoU of the batch added to cm_running since the last call, and its exponential average (csrc/census.hip; one launch, no
    host decision: it can be captured): iou_values = float32(1 - update) * iou_values + float32(update) * iou, cm_prev = cm_running.
    cm_running / cm_prev: int32 [K,K]; iou_values (in/out), iou_batch (optional): float32 [K].  Returns iou_values."""
    import numpy as np
    K = cm_running.shape[0]
    for t in (cm_running, cm_prev):
        assert t.dtype == torch.int32 and tuple(t.shape) == (K, K) and t.is_contiguous() and t.is_cuda
    for t in (iou_values, iou_batch):
        assert t is None or (t.dtype == torch.float32 and t.numel() == K and t.is_contiguous() and t.device == cm_running.device)
    a = float(update)
    check(lib.catseg_iou_ema(ptr(cm_running), ptr(cm_prev), K, float(np.float32(1 - a)), float(np.float32(a)), ptr(iou_values), ptr(iou_batch),
                             stream()))
    return iou_values


def resize_nearest(src, Ho, Wo, flip=0, out=None, accumulate=False, divide_by=0.0):
    """NHWC nearest resize (F.interpolate(mode='nearest', size=(Ho, Wo))); flip 1 = flip the source, 2 = flip the result"""
    B, Hi, Wi, C = src.shape
    if out is None:
        out = new_act(B, Ho, Wo, C, src.device)
        accumulate = False
    check(lib.catseg_resize_nearest(ptr(src), ld_of(src), ptr(out), ld_of(out), B, Hi, Wi, Ho, Wo, C, flip, 1 if accumulate else 0,
                                    divide_by, stream()))
    return out


MERGE_MODES = {"mean": 0, "max": 1}


def ensemble_merge(members, mode="mean", want_probs=True, want_labels=False):
    """members: M NHWC logit tensors [B, H, W, K] (pixel strides may differ) -> softmax per member, mean / max over the members, in ONE
    launch.  Returns (probs [B, H, W, K] NHWC or None, labels int64 [B, H, W] or None); labels = argmax of probs, first maximum."""
    t0 = members[0]
    B, H, W, K = t0.shape
    n = len(members)
    for t in members:
        assert tuple(t.shape) == (B, H, W, K) and t.dtype == torch.float32 and t.stride(-1) == 1 and t.device == t0.device
        assert (H == 1 or W == 1 or t.stride(1) == W * t.stride(2)) and (B == 1 or t.stride(0) == H * W * ld_of(t)), \
            "ensemble_merge: pixels must be evenly spaced (one pixel stride over the whole tensor)"
    Pn = B * H * W
    probs = new_act(B, H, W, K, t0.device) if want_probs else None
    labels = torch.empty((B, H, W), dtype=torch.int64, device=t0.device) if want_labels else None
    ptrs = (ctypes.c_void_p * n)(*[t.data_ptr() for t in members])
    lds = (ctypes.c_int * n)(*[ld_of(t) for t in members])
    with _Timed("hbm:ensemble_merge", 4.0 * (n + (1 if want_probs else 0)) * Pn * K + (8.0 * Pn if want_labels else 0.0)):
        check(lib.catseg_ensemble_merge(ptrs, lds, n, Pn, K, MERGE_MODES[mode], ptr(probs), ld_of(probs) if want_probs else 0, ptr(labels),
                                        stream()))
    return probs, labels


def egress_u8(rows, probs=False, crop=(0, 0), threshold=0.0, ignore_value=0, lut=None, palette=None, frame=None, mean=None, std=None,
              bgr=False, target=None, want_i64=False, want_u8=False, want_canvas=True):
    """rows: NHWC logits (or probabilities, probs=True) [B, H, W, K], any pixel stride (None: no prediction, the other panels alone) -> (labels int64 [B, H', W] of network ids or None,
    labels uint8 [B, H', W] of dataset ids or None, canvas uint8 [B, H', n_panels * W, 3] frame | target | prediction or None) in ONE launch
    (csrc/egress.hip).  frame: float32 NCHW [B, 3, H, W] or NHWC-4 [B, H, W, 4]; mean / std: sequences of 3 floats (un_normalise);
    target: int64 [B, H, W]; lut uint8[256], palette uint8[256, 3] (already in the output channel order) on the device."""
    if rows is None:                      # no prediction: the frame / target panels alone (mask_to_colormap of a label map)
        ref = target if target is not None else frame
        B, H, W = ref.shape if ref.dim() == 3 else ((ref.shape[0],) + tuple(ref.shape[1:3] if ref.shape[-1] == 4 and ref.shape[1] != 3 else ref.shape[2:]))
        K = ld = 0
        dev = ref.device
    else:
        B, H, W, K = rows.shape
        assert rows.dtype == torch.float32 and rows.is_cuda and rows.stride(-1) == 1
        ld = ld_of(rows)
        assert (H == 1 or W == 1 or rows.stride(1) == W * rows.stride(2)) and (B == 1 or rows.stride(0) == H * W * ld), \
            "egress_u8: pixels must be evenly spaced (one pixel stride over the whole tensor)"
        dev = rows.device
    for t in (lut, palette):
        assert t is None or (t.dtype == torch.uint8 and t.is_contiguous() and t.device == dev and t.numel() == (256 if t is lut else 768))
    nhwc4 = False
    if frame is not None:
        nhwc4 = frame.dim() == 4 and frame.shape[-1] == 4 and frame.shape[1] != 3
        assert frame.dtype == torch.float32 and frame.is_contiguous() and frame.device == dev
        assert tuple(frame.shape) == ((B, H, W, 4) if nhwc4 else (B, 3, H, W)), "egress_u8: the frame must have the rows' B, H, W"
    if target is not None:
        assert target.dtype == torch.int64 and target.is_contiguous() and tuple(target.shape) == (B, H, W) and target.device == dev
    Ho = H - crop[0] - crop[1]
    li = torch.empty((B, max(Ho, 0), W), dtype=torch.int64, device=dev) if want_i64 else None
    lu = torch.empty((B, max(Ho, 0), W), dtype=torch.uint8, device=dev) if want_u8 else None
    n_panels = (rows is not None) + (frame is not None) + (target is not None)
    canvas = torch.empty((B, max(Ho, 0), n_panels * W, 3), dtype=torch.uint8, device=dev) if want_canvas else None
    cm = (ctypes.c_float * 3)(*mean) if mean is not None else None
    cs = (ctypes.c_float * 3)(*std) if std is not None else None
    nbytes = float(B) * max(Ho, 0) * W * (4 * ld + (8 if want_i64 else 0) + (1 if want_u8 else 0) + (3 * n_panels if want_canvas else 0)
                                          + (12 if frame is not None else 0) + (8 if target is not None else 0))
    with _Timed("hbm:egress", nbytes):
        check(lib.catseg_egress_u8(ptr(rows), ld, B, H, W, K, 1 if probs else 0, crop[0], crop[1], float(threshold or 0.0), int(ignore_value or 0),
                                   ptr(lut), ptr(palette), ptr(frame), 1 if nhwc4 else 0, cm, cs, 1 if bgr else 0, ptr(target), ptr(li), ptr(lu),
                                   ptr(canvas), stream()))
    return li, lu, canvas


def confusion_matrix(logits, labels, cm=None):
    Pn, K = logits.shape
    if cm is None:
        cm = torch.zeros((K, K), dtype=torch.int32, device=logits.device)
    check(lib.catseg_confusion_matrix(ptr(logits), ptr(labels), Pn, K, ptr(cm), stream()))
    return cm


def adam_step(p, g, m, v, lr, step, beta1=0.9, beta2=0.999, eps=1e-8, grad_scale=1.0):
    with _Timed("hbm:adam", 28.0 * p.numel()):          # 16 B read + 12 B written per parameter
        _adam_step(p, g, m, v, lr, step, beta1, beta2, eps, grad_scale)


def _adam_step(p, g, m, v, lr, step, beta1, beta2, eps, grad_scale):
    check(lib.catseg_adam_step(ptr(p), ptr(g), ptr(m), ptr(v), p.numel(), lr, beta1, beta2, eps, step, grad_scale, stream()))


def adam_step_dev(p, g, m, v, hyper, beta1=0.9, beta2=0.999, eps=1e-8):
    """adam_step with {lr, bias corrections, gradient scale} in device memory (hyper: float32[4], optim.FusedAdam.upload_hyper)"""
    with _Timed("hbm:adam", 28.0 * p.numel()):
        check(lib.catseg_adam_step_dev(ptr(p), ptr(g), ptr(m), ptr(v), p.numel(), ptr(hyper), beta1, beta2, eps, stream()))


# ---- the fused optimiser updates of include/catseg_optim.h.  hyper: the 20 step scalars (catseg_optim_hyper) as a HOST float32
# tensor (passed by value) or a DEVICE one (read by the kernel: a captured launch replays with what was uploaded); group_map: uint8 per
# 64-float chunk or None; clip: the float32[2] that grad_norm wrote, or None
OPTIM_HYPER_FLOATS, OPTIM_MAX_GROUPS = 20, 8
WD_NONE, WD_COUPLED, WD_DECOUPLED = range(3)


def _hyper_args(hyper):
    if hyper.dtype != torch.float32 or hyper.numel() < OPTIM_HYPER_FLOATS or not hyper.is_contiguous():
        raise ValueError("the step-scalar row is %d contiguous float32 values" % OPTIM_HYPER_FLOATS)
    return (None, ptr(hyper)) if hyper.is_cuda else (ptr(hyper), None)


def optim_hyper(row, step, beta1, beta2, grad_scale, dampening, lrs, wds):
    """fill a HOST float32 row with the step scalars of `step` (catseg_optim_hyper); lrs, wds: one value per parameter group"""
    G = len(lrs)
    if row.is_cuda or row.dtype != torch.float32 or row.numel() < OPTIM_HYPER_FLOATS or not 1 <= G <= OPTIM_MAX_GROUPS or len(wds) != G:
        raise ValueError("optim_hyper: a host float32 row of %d values and 1..%d groups" % (OPTIM_HYPER_FLOATS, OPTIM_MAX_GROUPS))
    lib.catseg_optim_hyper(int(step), beta1, beta2, grad_scale, dampening, G, (ctypes.c_float * G)(*lrs), (ctypes.c_float * G)(*wds), row.data_ptr())
    return row


def adam_step_ex(p, g, m, v, hyper, G=1, group_map=None, vmax=None, beta1=0.9, beta2=0.999, eps=1e-8, wd_mode=WD_NONE, clip=None):
    nbytes = (28.0 + (8.0 if vmax is not None else 0.0) + (1.0 / 64 if group_map is not None else 0.0)) * p.numel()
    hh, hd = _hyper_args(hyper)
    with _Timed("hbm:adam_ex", nbytes):
        check(lib.catseg_adam_step_ex(ptr(p), ptr(g), ptr(m), ptr(v), ptr(vmax), p.numel(), ptr(group_map), G, hh, hd, beta1, beta2, eps, wd_mode,
                                      ptr(clip), stream()))


def sgd_step(p, g, buf, hyper, G=1, group_map=None, momentum=0.0, nesterov=False, use_wd=False, clip=None):
    nbytes = (12.0 + (8.0 if buf is not None else 0.0) + (1.0 / 64 if group_map is not None else 0.0)) * p.numel()
    hh, hd = _hyper_args(hyper)
    with _Timed("hbm:sgd", nbytes):
        check(lib.catseg_sgd_step(ptr(p), ptr(g), ptr(buf), p.numel(), ptr(group_map), G, hh, hd, momentum, 1 if nesterov else 0,
                                  1 if use_wd else 0, ptr(clip), stream()))


def grad_norm_workspace(n):
    return int(lib.catseg_grad_norm_workspace(n))


def grad_norm(g, out, work, max_norm, grad_scale=1.0, hyper_dev=None):
    """out[0] = ||g * grad_scale||_2, out[1] = min(1, max_norm / (out[0] + 1e-6)); two launches, deterministic; work: DEVICE bytes"""
    with _Timed("hbm:grad_norm", 4.0 * g.numel()):
        check(lib.catseg_grad_norm(ptr(g), g.numel(), grad_scale, ptr(hyper_dev), max_norm, ptr(work), work.numel() * work.element_size(), ptr(out),
                                   stream()))
    return out


# ---- the running average of the weights (include/catseg_ema.h).  w: a float (passed by value) or a DEVICE float32 tensor whose
# first element the kernel reads (a captured launch replays with what was uploaded)
EMA_LERP, EMA_SWAP = 0, 1
EMA_ENTRY = [("live", "<i8"), ("shadow_off", "<i8"), ("n", "<i4"), ("pad", "<i4")]      # csrc/ema.hip: EmaEntry (24 bytes)


def _ema_weight(w):
    if torch.is_tensor(w):
        if not w.is_cuda or w.dtype != torch.float32 or w.numel() < 1:
            raise ValueError("the weight is a number or a DEVICE float32 tensor")
        return 0.0, ptr(w)
    return float(w), None


def ema_update(p, avg, w):
    """avg = lerp(avg, p, w) over two flat float32 buffers of one length (torch.lerp's two-sided form; w = 1 copies p)"""
    if avg.numel() != p.numel():
        raise ValueError("ema_update: p and avg differ in length")
    wh, wd = _ema_weight(w)
    with _Timed("hbm:ema", 12.0 * p.numel()):
        check(lib.catseg_ema_update(ptr(p), ptr(avg), p.numel(), wh, wd, stream()))


def ema_swap(a, b):
    """exchanges two flat float32 buffers of one length in place"""
    if a.numel() != b.numel():
        raise ValueError("ema_swap: a and b differ in length")
    with _Timed("hbm:ema_swap", 16.0 * a.numel()):
        check(lib.catseg_ema_swap(ptr(a), ptr(b), a.numel(), stream()))


def ema_table(entries, count, shadow, mode, w=0.0):
    """one launch over a DEVICE table of EMA_ENTRY records: mode EMA_LERP shadow = lerp(shadow, live, w), mode EMA_SWAP exchanges the two"""
    wh, wd = _ema_weight(w)
    check(lib.catseg_ema_table(ptr(entries), count, ptr(shadow), mode, wh, wd, stream()))


def add_n_act(terms, relu, out=None):
    """out = act(sum(terms)); terms: up to 4 NHWC tensors of one shape (row strides may differ)"""
    t0 = terms[0]
    rows, C = rows_of(t0), t0.shape[-1]
    if out is None:
        out = torch.empty(t0.shape, dtype=torch.float32, device=t0.device)
    n = len(terms)
    ptrs = (ctypes.c_void_p * n)(*[t.data_ptr() for t in terms])
    lds = (ctypes.c_int * n)(*[ld_of(t) for t in terms])
    planes = planes_ok(C, rows) and all(amax_of(t) is not None for t in terms)
    rec = new_amax(t0.device) if planes or _trunk_h2() else None
    recs = (ctypes.c_void_p * n)(*[amax_of(t).data_ptr() for t in terms]) if planes else None
    buf = torch.empty(lib.catseg_planes_bytes(rows, C), dtype=torch.uint8, device=t0.device) if planes else None
    check(lib.catseg_add_n_act(ptrs, lds, recs, n, ptr(out), ld_of(out), ptr(buf), rows, C, 1 if relu else 0, ptr(rec), stream()))
    if rec is not None:
        out._amax = rec
    if planes:
        out._planes = Planes(buf, rec, t0.shape)
    return out


def relu_bwd(dz, z):
    g = torch.empty(z.shape, dtype=torch.float32, device=z.device)
    check(lib.catseg_relu_bwd(ptr(dz), ld_of(dz), ptr(z), ld_of(z), ptr(g), ld_of(g), rows_of(z), z.shape[-1], stream()))
    return g


def weight_pad_cin(w, O, taps, cin, cpad):
    out = torch.empty((O, taps, cpad), dtype=torch.float32, device=w.device)
    check(lib.catseg_weight_pad_cin(ptr(w), ptr(out), O, taps, cin, cpad, 0, stream()))
    return out


def weight_unpad_cin(pk, dw, O, taps, cin, cpad):
    check(lib.catseg_weight_pad_cin(ptr(pk), ptr(dw), O, taps, cin, cpad, 1, stream()))
    return dw


def adaptive_avgpool_fwd(x, S):
    B, H, W, C = x.shape
    y = torch.empty((B, S, S, C), dtype=torch.float32, device=x.device)
    check(lib.catseg_adaptive_avgpool_fwd(ptr(x), ld_of(x), ptr(y), B, H, W, C, S, stream()))
    return y


def adaptive_avgpool_bwd(dy, dx, S, accumulate):
    B, H, W, C = dx.shape
    check(lib.catseg_adaptive_avgpool_bwd(ptr(dy), ptr(dx), ld_of(dx), B, H, W, C, S, 1 if accumulate else 0, stream()))
    return dx


def fold_bn(w, bias, gamma, beta, rm, rv, eps, O, per_out):
    """conv weight / bias with an eval-mode BatchNorm folded in (inference fast path)"""
    wf = torch.empty(O * per_out, dtype=torch.float32, device=w.device)
    bf = torch.empty(O, dtype=torch.float32, device=w.device)
    check(lib.catseg_fold_bn(ptr(w), ptr(bias), ptr(gamma), ptr(beta), ptr(rm), ptr(rv), eps, O, per_out, ptr(wf), ptr(bf), stream()))
    return wf, bf


def conv_fwd_fused(x, w, bias, residual, relu, Cout, kh, kw, stride=1, pad=0, dil=1, out=None, stem4=False, groups=1):
    B, H, W, Cin = x.shape
    Ho, Wo = conv_out_size(H, kh, stride, pad, dil), conv_out_size(W, kw, stride, pad, dil)
    if out is None:
        out = new_act(B, Ho, Wo, Cout, x.device)
    flops = 2.0 * B * Ho * Wo * Cout * (3 if stem4 else Cin // groups) * kh * kw
    epilogue = dict(bias=bias, ldr=ld_of(residual) if residual is not None else 0, relu=1 if relu else 0)
    if (_fwd_gemm_ok(Layer(x.shape, Cout, kh, kw, stride, pad, dil, groups, stem4=stem4, w4d=w.numel() == Cout * kh * kw * Cin))
            and _b3_blocked_shape(Cout, Cin) and 6 * Cout * kh * kw * Cin < (1 << 32) - 64):
        # the bf16x3 kernel with the fused epilogue; the batch is cut so that the three blocked planes of a piece stay below 4 GB
        # (UPerNet's 3x3 2048 -> 512 on a 4 x 272 x 480 map: 6.4 GB of planes in one piece)
        per_img = 6 * H * W * Cin
        nb = max(1, min(B, B3_PLANE_LIMIT // per_img))
        if per_img < B3_PLANE_LIMIT:
            wp = None
            for b0 in range(0, B, nb):
                xs, os_ = (x, out) if nb == B else (x[b0:b0 + nb], out[b0:b0 + nb])    # (x itself: the split-plane cache is keyed by identity)
                rs = residual[b0:b0 + nb] if residual is not None else None
                d = make_desc(xs.shape, Cin, Cout, ld_of(out), kh, kw, stride, pad, dil)
                with _Timed("split3", 0.0):      # (w: OHWI weights, 4-D or the flat buffer catseg_fold_bn writes)
                    if _h2():
                        kind, operands = "fwd_h2", OPERANDS_F16X2_BLOCKED
                        xp, xsc = _split3_cached(xs, "h2") if nb == B else split2h_blocked(xs)
                        if wp is None:
                            wp, wsc = _wi.weight_image(w, "h2", geometry=(Cout, kh * kw, Cin))
                    else:
                        kind, operands, xsc, wsc = "fwd_b3", OPERANDS_BF16X3_BLOCKED, None, None
                        xp = _split3_cached(xs, "blk") if nb == B else split3_blocked(xs)[0]
                        if wp is None:
                            wp = _wi.weight_image(w, "b3", blocked=True, geometry=(Cout, kh * kw, Cin))
                with _Timed(kind, flops * xs.shape[0] / B):
                    _conv_call(ConvFwdDesc, d, operands, x=xp, x_scale=xsc, w=wp, w_scale=wsc, residual=rs, y=os_, **epilogue)
            return out
    d = make_desc(x.shape, ld_of(x), Cout, ld_of(out), kh, kw, stride, pad, dil, stem4, groups)
    with _Timed("fwd", flops):
        _conv_call(ConvFwdDesc, d, OPERANDS_F32, x=x, w=w, residual=residual, y=out, **epilogue)
    return out


# ---------------------------------------------------------------------------------------------- split precision (bf16 x 3)
def split3(x):
    """fp32 NHWC activation [..., C] (pixel stride ld) -> int16 planes [3, rows, roundup(C, 8)]"""
    rows, C, ld = rows_of(x), x.shape[-1], ld_of(x)
    planes = torch.empty((3, rows, (C + 7) // 8 * 8), dtype=torch.int16, device=x.device)
    check(lib.catseg_split3(ptr(x), ld, rows, C, ptr(planes), stream()))
    return planes


def split3_blocked(x, with_planar=False):
    """fp32 NHWC activation -> (blocked planes [3, ceil(C/16), rows, 16], planar planes [3, rows, roundup(C, 8)] or None), one pass"""
    rows, C, ld = rows_of(x), x.shape[-1], ld_of(x)
    blk = torch.empty((3, (C + 15) // 16, rows, 16), dtype=torch.int16, device=x.device)
    planar = torch.empty((3, rows, (C + 7) // 8 * 8), dtype=torch.int16, device=x.device) if with_planar else None
    check(lib.catseg_split3_blocked(ptr(x), rows, C, ld, ptr(blk), ptr(planar), stream()))
    return blk, planar


def split2h(x, blocked=True, planar=False):
    """fp32 NHWC activation -> fp16 planes of x * 2^e in the blocked layout [2, ceil(C/16), rows, 16] and / or the planar layout
    [2, rows, roundup(C, 8)] (one pass for both) + the device record int32[2] = {bits of max|x|, e}: (blocked or None, planar or None, scale)"""
    rows, C, ld = rows_of(x), x.shape[-1], ld_of(x)
    blk = torch.empty((2, (C + 15) // 16, rows, 16), dtype=torch.int16, device=x.device) if blocked else None
    pl = torch.empty((2, rows, (C + 7) // 8 * 8), dtype=torch.int16, device=x.device) if planar else None
    scale = torch.empty(2, dtype=torch.int32, device=x.device)
    recs = amax_records_of(x) if SPLIT_BOUND else None
    if recs:        # the producers of x left max|x|: no pass over x to find it (csrc/igemm_f16x2.hip: catseg_split2h_bound)
        r = list(recs) + [None] * (4 - len(recs))
        check(lib.catseg_split2h_bound(ptr(x), rows, C, ld, ptr(blk), ptr(pl), ptr(scale), ptr(r[0]), ptr(r[1]), ptr(r[2]), ptr(r[3]), stream()))
    else:
        check(lib.catseg_split2h(ptr(x), rows, C, ld, ptr(blk), ptr(pl), ptr(scale), stream()))
    return blk, pl, scale


def split2h_blocked(x):
    blk, _, scale = split2h(x, True, False)
    return blk, scale


H2W_BANK = _plan.get("h2w_bank")     # head layers keep their image buffers in the network's bank (weight_images.py)


# [O, I, kh, kw] weights (physical OHWI) -> the operand of a GEMM route, forward or (_t) backward-data (the transposed bank); shapes, and which
# of them a network's bank keeps: weight_images.py.  split2h: (fp16 planes, scale record), I % 16 == 0; split3: bf16 planes, I % 8 == 0
# (blocked: % 16)
def split2h_weight_blocked(w):
    return _wi.weight_image(w, "h2")


def split2h_weight_t_blocked(w):
    return _wi.weight_image(w, "h2", True)


def split3_weight_blocked(w):
    return _wi.weight_image(w, "b3", blocked=True)


def split3_weight_t_blocked(w):
    return _wi.weight_image(w, "b3", True, blocked=True)


def split3_weight(w):
    return _wi.weight_image(w, "b3")


def split3_weight_t(w):
    return _wi.weight_image(w, "b3", True)


def conv_fwd_b3(xshape, xp, wp, bias, Cout, kh, kw, stride=1, pad=0, dil=1, out=None, zero_to=0, blocked=False):
    """forward from pre-split bf16x3 planes (tests and tools): split3 / split3_weight, or with blocked=True split3_blocked /
    split3_weight_blocked (always the 256 x 256 register-pipelined kernel)"""
    B, H, W, Cin = xshape
    Ho, Wo = conv_out_size(H, kh, stride, pad, dil), conv_out_size(W, kw, stride, pad, dil)
    if out is None:
        out = new_act(B, Ho, Wo, Cout, xp.device, ld=max(zero_to, (Cout + 3) // 4 * 4))
    d = make_desc(xshape, Cin, Cout, ld_of(out), kh, kw, stride, pad, dil)
    with _Timed("fwd", 2.0 * B * Ho * Wo * Cout * Cin * kh * kw):
        _conv_call(ConvFwdDesc, d, OPERANDS_BF16X3_BLOCKED if blocked else OPERANDS_BF16X3, x=xp, w=wp, bias=bias, y=out, zero_to=zero_to)
    return out


def conv_bwd_data_b3(dyp, wtp, xshape, Cout, kh, kw, stride=1, pad=0, dil=1, out=None, accumulate=False, blocked=False):
    """backward-data from pre-split bf16x3 planes (tests and tools): split3 / split3_weight_t, or their blocked twins"""
    B, H, W, Cin = xshape
    if out is None:
        out = new_act(B, H, W, Cin, dyp.device)
        accumulate = False
    d = make_desc(xshape, ld_of(out), Cout, (Cout + 7) // 8 * 8, kh, kw, stride, pad, dil)
    with _Timed("dgrad", 2.0 * B * d.Ho * d.Wo * Cout * Cin * kh * kw):
        _conv_call(ConvBwdDataDesc, d, OPERANDS_BF16X3_BLOCKED if blocked else OPERANDS_BF16X3, dy=dyp, w=wtp, dx=out,
                   accumulate=1 if accumulate else 0)
    return out


# ---------------------------------------------------------------------------------------------- uint8 augmentation (csrc/augment.hip)
def aug_pad_flip_u8(img, flips, pad_top, pad_bottom):
    """uint8 [B,H,W,C] -> uint8 [B,H+pad,W,C]: FlipNP flags (bit 0 horizontal, bit 1 vertical) + PadNP reflect rows"""
    assert img.dtype == torch.uint8 and img.is_contiguous() and img.is_cuda and img.dim() == 4
    B, H, W, C = img.shape
    out = torch.empty((B, H + pad_top + pad_bottom, W, C), dtype=torch.uint8, device=img.device)
    check(lib.catseg_aug_pad_flip_u8(ptr(img), ptr(out), B, H, W, C, ptr(flips), pad_top, pad_bottom, stream()))
    return out


def aug_gaussian_blur(img, radius, ww, fw):
    """ImageFilter.GaussianBlur per image: three box passes along W, then three along H; radius[b] < 0: image unchanged"""
    assert img.dtype == torch.uint8 and img.is_contiguous() and img.is_cuda and img.shape[-1] == 3
    B, H, W, _ = img.shape
    a, b = img, torch.empty_like(img)
    for axis in (1, 1, 1, 0, 0, 0):
        check(lib.catseg_aug_box_blur(ptr(a), ptr(b), B, H, W, axis, ptr(radius), ptr(ww), ptr(fw), stream()))
        a, b = b, (torch.empty_like(img) if a is img else a)
    return a


def aug_color_workspace_bytes(B, H, W, extended=None):
    """the workspace sizes of catseg_aug_color_op (include/catseg.h): None = the ColorJitter pipeline (op codes < 4), "lut" = the extended
    pipeline with the band histograms (codes 0 ... 7; CATSEG_AUG_WS_LUT), "full" = with the source copy as well (code 8; CATSEG_AUG_WS_FULL)"""
    if extended is None:
        return 8 * B + 256
    if extended not in ("lut", "full"):
        raise ValueError("aug_color_op: extended must be None, 'lut' or 'full', got %r" % (extended,))
    lut = (8 * B + 255) // 256 * 256 + 3072 * B
    return lut if extended == "lut" else lut + 3 * B * H * W


def aug_color_op(img, op, factor, extended=None):
    """one photometric operation per image, IN PLACE.  op 0 brightness, 1 contrast, 2 saturation (factor = the enhance factor), 3 hue (factor
    = the H shift): torchvision ColorJitter's, two launches.  extended="lut" adds 4 autocontrast, 5 equalize, 6 posterize (factor = bits),
    7 solarize (factor = threshold); extended="full" adds 8 sharpness (factor = the enhance factor), which needs a copy of the frames in
    the workspace.  The library picks the pipeline from the workspace size it is handed, so exactly the size asked for is passed on."""
    assert img.dtype == torch.uint8 and img.is_contiguous() and img.is_cuda and img.shape[-1] == 3
    B, H, W, _ = img.shape
    nbytes = aug_color_workspace_bytes(B, H, W, extended)
    ws = workspace(nbytes, img.device)
    check(lib.catseg_aug_color_op(ptr(img), B, H, W, ptr(op), ptr(factor), ptr(ws), nbytes, stream()))
    return img


# ---------------------------------------------------------------------------------------------- PointRend refinement (csrc/pointrend.hip)
def pointrend_upsample2x(seg):
    """seg [B, h, w, K] class logits (any pixel stride >= K) -> (up [B, 2h, 2w, K] dense, uncertainty [B, 2h, 2w]): up IS the launch
    bilinear_fwd(seg, 2h, 2w, False); uncertainty = second-largest - largest of the K logits it stored (utils/pointrend_utils.py:220-232
    of the reference).  The pad columns of seg's rows never take part."""
    B, H, W, K = seg.shape
    if K < 2:
        raise ValueError("PointRend's uncertainty is the difference of the two largest logits: it needs at least 2 classes (got %d)" % K)
    up = bilinear_fwd(seg, 2 * H, 2 * W, False)
    unc = torch.empty((B, 2 * H, 2 * W), dtype=torch.float32, device=seg.device)
    with _Timed("hbm:pointrend_uncertainty", 4.0 * (up.numel() + unc.numel())):
        check(lib.catseg_pointrend_uncertainty(ptr(up), ld_of(up), ptr(unc), unc.numel(), K, stream()))
    return up, unc


def pointrend_topk(unc, k):
    """indices (int32 [N, k], ascending) of the k largest entries of every row of unc [N, ...]; among equal values the lower index is
    selected (-0.0 == +0.0); k >= the row length selects everything.  No host synchronisation: capturable."""
    assert unc.dtype == torch.float32 and unc.is_contiguous()
    N = unc.shape[0]
    n = unc.numel() // N
    k = min(int(k), n)
    idx = torch.empty((N, k), dtype=torch.int32, device=unc.device)
    need = lib.catseg_pointrend_topk_workspace(N, n)
    ws = workspace(need, unc.device)
    check(lib.catseg_pointrend_topk(ptr(unc), N, n, k, ptr(idx), ptr(ws), ws.numel(), stream()))
    return idx


def pointrend_gather(sources, idx, h, w, out=None, extras=()):
    """the point matrix [N k, sum of the sources' channels, each rounded up to 4]: for every selected cell idx[b, p] of the h x w grid
    F.grid_sample(bilinear, align_corners=False, zero padding) of every source (NHWC [N, H_s, W_s, C_s]) at the cell's centre, the blocks
    side by side in the order given (models/PointRend.py:81-83: deepest stage first, the coarse logits last).  extras: [(buffer [N k, ld],
    first column)] -- further places the LAST source's block is written to."""
    N, k = idx.shape
    cols = sum((s.shape[-1] + 3) // 4 * 4 for s in sources)
    if out is None:
        out = torch.empty((N * k, cols), dtype=torch.float32, device=idx.device)
    d = _lib.PointrendGatherDesc()
    for i, s in enumerate(sources):
        assert s.shape[0] == N and s.dtype == torch.float32
        d.src[i], d.ld[i], d.H[i], d.W[i], d.C[i] = ptr(s), ld_of(s), s.shape[1], s.shape[2], s.shape[3]
    d.n_sources, d.idx, d.N, d.k, d.h, d.w, d.out, d.ld_out = len(sources), ptr(idx), N, k, h, w, ptr(out), out.stride(0)
    for i, (buf, c0) in enumerate(extras):
        d.extra[i], d.extra_ld[i], d.extra_off[i] = ptr(buf), buf.stride(0), c0
    d.n_extra = len(extras)
    check(lib.catseg_pointrend_gather(ctypes.byref(d), stream()))
    return out


def pointrend_scatter(rows, idx, seg):
    """seg[b, idx[b, p], :] = rows[b k + p, :K] in place (seg NHWC [N, h, w, K])"""
    N, k = idx.shape
    _, h, w, K = seg.shape
    check(lib.catseg_pointrend_scatter(ptr(rows), rows.stride(0), ptr(idx), N, k, h * w, ptr(seg), ld_of(seg), K, stream()))
    return seg


# ---------------------------------------------------------------------------------------------- PointRend training (csrc/pointrend_train.hip)
def pointrend_draw(state, N, M, fixed=None):
    """[N, M, 2] uniforms in [0, 1): the next draw of the sampler whose 16-byte device state is `state` (int32 [4]: seed lo, seed hi,
    layer | rank << 16, draw counter); the launch advances the counter.  fixed (a test knob): the given [N, M, 2] coordinates instead of a
    draw, the state does not move."""
    dev = fixed.device if fixed is not None else state.device
    out = torch.empty((N, M, 2), dtype=torch.float32, device=dev)
    if fixed is not None:
        assert tuple(fixed.shape) == (N, M, 2) and fixed.dtype == torch.float32 and fixed.is_contiguous()
    check(lib.catseg_pointrend_draw(None if fixed is not None else ptr(state), ptr(fixed) if fixed is not None else None, N, M, ptr(out), stream()))
    return out


def pointrend_point_uncertainty(coarse, coords):
    """[N, M]: second-largest - largest of the K logits of coarse (NHWC [N, H, W, K], any pixel stride) point-sampled at coords [N, M, 2]"""
    N, H, W, K = coarse.shape
    if K < 2:
        raise ValueError("PointRend's uncertainty is the difference of the two largest logits: it needs at least 2 classes (got %d)" % K)
    M = coords.shape[1]
    assert coords.shape[0] == N and coords.dtype == torch.float32 and coords.is_contiguous()
    unc = torch.empty((N, M), dtype=torch.float32, device=coarse.device)
    with _Timed("pointrend_point_uncertainty", 0.0):
        check(lib.catseg_pointrend_point_uncertainty(ptr(coarse), ld_of(coarse), N, H, W, K, ptr(coords), M, ptr(unc), stream()))
    return unc


def pointrend_compose(cand, sel, rest, h, w, lbl=None):
    """(coords [N, P, 2], pix int32 [N, P], labels int64 [N, P] or None): the selected candidates cand[b, sel[b]] followed by rest; per
    point its pixel of the h x w map (models/PointRend.py:56-57 of the reference) and, with lbl (int64 [N, Hl, Wl]), its nearest label."""
    N = (cand if cand is not None else rest).shape[0]
    kb = 0 if sel is None else sel.shape[1]
    R = 0 if rest is None else rest.shape[1]
    P = kb + R
    dev = (cand if cand is not None else rest).device
    coords = torch.empty((N, P, 2), dtype=torch.float32, device=dev)
    pix = torch.empty((N, P), dtype=torch.int32, device=dev)
    labels = None
    Hl = Wl = 0
    if lbl is not None:
        assert lbl.dtype == torch.int64 and lbl.is_contiguous() and lbl.dim() == 3 and lbl.shape[0] == N
        Hl, Wl = lbl.shape[1:]
        labels = torch.empty((N, P), dtype=torch.int64, device=dev)
    check(lib.catseg_pointrend_compose(ptr(cand) if kb else None, cand.shape[1] if kb else 0, ptr(sel) if kb else None, kb, ptr(rest) if R else None, N, P,
                                       h, w, ptr(lbl) if lbl is not None else None, Hl, Wl, ptr(coords), ptr(pix),
                                       ptr(labels) if labels is not None else None, stream()))
    return coords, pix, labels


def pointrend_point_labels(coords, lbl):
    """int64 [N, P]: F.grid_sample(lbl.float(), mode='nearest') at coords [N, P, 2] (managers/EncDec_Manager.py:164 of the reference)"""
    coords = coords.detach()
    if not coords.is_contiguous():
        coords = coords.contiguous()
    return pointrend_compose(None, None, coords, lbl.shape[1], lbl.shape[2], lbl.contiguous())[2]


def pointrend_gather_at(sources, coords, out=None, extras=()):
    """pointrend_gather at given points: coords [N, P, 2] (x, y) in [0, 1]^2"""
    N, k, _ = coords.shape
    assert coords.dtype == torch.float32 and coords.is_contiguous()
    cols = sum((s.shape[-1] + 3) // 4 * 4 for s in sources)
    if out is None:
        out = torch.empty((N * k, cols), dtype=torch.float32, device=coords.device)
    d = _lib.PointrendGatherDesc()
    for i, s in enumerate(sources):
        assert s.shape[0] == N and s.dtype == torch.float32
        d.src[i], d.ld[i], d.H[i], d.W[i], d.C[i] = ptr(s), ld_of(s), s.shape[1], s.shape[2], s.shape[3]
    d.n_sources, d.N, d.k, d.out, d.ld_out = len(sources), N, k, ptr(out), out.stride(0)
    for i, (buf, c0) in enumerate(extras):
        d.extra[i], d.extra_ld[i], d.extra_off[i] = ptr(buf), buf.stride(0), c0
    d.n_extra = len(extras)
    with _Timed("hbm:pointrend_gather_at", 4.0 * (4 + 1) * N * k * cols):
        check(lib.catseg_pointrend_gather_at(ctypes.byref(d), ptr(coords), stream()))
    return out


def pointrend_gather_bwd(dx, coords, dests):
    """the adjoint of pointrend_gather_at: dx [N P, >= cols] -> dests = [(NHWC gradient buffer [N, H, W, C], accumulate?)] in the order of
    the gather's sources.  accumulate False: the whole buffer is written (pixels no tap touches: zero).  Deterministic, no atomics."""
    N, P, _ = coords.shape
    d = _lib.PointrendGatherBwdDesc()
    nbytes = 0.0
    for i, (g, acc) in enumerate(dests):
        assert g.shape[0] == N and g.dtype == torch.float32
        d.dst[i], d.ld[i], d.H[i], d.W[i], d.C[i], d.accumulate[i] = ptr(g), ld_of(g), g.shape[1], g.shape[2], g.shape[3], 1 if acc else 0
        nbytes += 4.0 * ((0 if acc else g.numel()) + (4 + 4) * N * P * g.shape[3])
    d.n_sources, d.coords, d.N, d.P, d.dx, d.ld_dx = len(dests), ptr(coords), N, P, ptr(dx), dx.stride(0)
    with _Timed("hbm:pointrend_gather_bwd", nbytes):
        check(lib.catseg_pointrend_gather_bwd(ctypes.byref(d), stream()))
    return [g for g, _ in dests]


def pointrend_scatter_last(rows, pix, seg):
    """seg[b, pix[b, p], :] = rows[b P + p, :K] in place (seg NHWC [N, h, w, K]); among the points of one pixel the last one writes"""
    N, P = pix.shape
    _, h, w, K = seg.shape
    check(lib.catseg_pointrend_scatter_last(ptr(rows), rows.stride(0), ptr(pix), N, P, h * w, ptr(seg), ld_of(seg), K, stream()))
    return seg


def pointrend_scatter_bwd(dseg, pix, drows, accumulate):
    """drows[b P + p, :K] (+)= dseg[b, pix[b, p], :] for every point, then dseg = 0 at every scattered pixel (in place)"""
    N, P = pix.shape
    _, h, w, K = dseg.shape
    check(lib.catseg_pointrend_scatter_bwd(ptr(dseg), ld_of(dseg), ptr(pix), N, P, h * w, ptr(drows), drows.stride(0), K, 1 if accumulate else 0, stream()))
    return drows


def _pointrend_weight(w, main, K, cache=None, slot=None):
    """device image of a point-head layer's weight [O, main + K (, 1)] for an input whose coarse block is K rounded up to 4 columns wide:
    the columns of the pad are zero (the parameter keeps the reference's shape).  cache (a dict the head owns) keeps the image until the
    parameter moves or is written in place (data_ptr, version), as the other layers' device images are kept."""
    Kq = (K + 3) // 4 * 4
    w2 = w.reshape(w.shape[0], -1)
    if w2.shape[1] == main or Kq == K:
        return w2.contiguous()
    key = (w.data_ptr(), w._version, tuple(w.shape), str(w.device))
    if cache is not None and slot in cache and cache[slot][0] == key and not torch.cuda.is_current_stream_capturing():
        return cache[slot][1]
    img = torch.zeros((w2.shape[0], main + Kq), dtype=torch.float32, device=w.device)
    img[:, :main + K].copy_(w2)
    if cache is not None and not torch.cuda.is_current_stream_capturing():     # (an image built inside a capture lives in the graph's pool)
        cache[slot] = (key, img)
    return img


def pointrend_refine(seg, feats, head, k0, steps, record=None):
    """The eval-mode loop of the reference's PointRend.forward (models/PointRend.py:74-90).  seg: coarse logits NHWC [N, h, w, K]; feats: the
    encoder stages NHWC, shallow to deep; head: {"fc": [(weight [O, I(, 1)], bias)], "predictor": (weight, bias), "coarse_in_each_layer":
    bool}; k0 = pr_subdivision_num_pts.  Per step: upsample x 2 + uncertainty, the min(h w, k0) most uncertain pixels, the point matrix
    [c5 | c4 | c3 | c2 | coarse], the head's 1 x 1 layers over the N k points, the scatter.  Returns the refined logits [N, h 2^steps,
    w 2^steps, K]; record (a list) receives per step {"idx": int32 [N, k] ascending, "uncertainty": [N, h, w]}.  No host synchronisation."""
    N, _, _, K = seg.shape
    if K < 2:
        raise ValueError("PointRend's uncertainty is the difference of the two largest logits: it needs at least 2 classes (got %d)" % K)
    Kq = (K + 3) // 4 * 4
    each = bool(head.get("coarse_in_each_layer", True))
    srcs = list(feats[::-1])
    Cf = sum(f.shape[-1] for f in srcs)
    if any(f.shape[-1] % 4 for f in srcs):
        raise ValueError("PointRend: the encoder stages' channel counts must be multiples of 4 (got %s)" % [f.shape[-1] for f in feats])
    fcs = head["fc"]
    widths = [w.shape[0] for w, _ in fcs]
    if any(o % 4 for o in widths):
        raise ValueError("PointRend: ph_fc_dim must be a multiple of 4 (got %s)" % widths)
    mains = [Cf] + widths                      # width of each layer's input in front of its coarse block
    cache = head.get("images")
    imgs = [_pointrend_weight(w, m, K if (i == 0 or each) else 0, cache, i) for i, ((w, _), m) in enumerate(zip(list(fcs) + [head["predictor"]], mains))]
    dev = seg.device
    for _ in range(steps):
        up, unc = pointrend_upsample2x(seg)
        _, h, w, _ = up.shape
        idx = pointrend_topk(unc, k0)
        k = idx.shape[1]
        rows = N * k
        x = torch.empty((rows, Cf + Kq), dtype=torch.float32, device=dev)
        bufs, extras = [], []
        for li, o in enumerate(widths):
            if each:                            # (two buffers in turn: layer i + 1 reads what layer i wrote beside the coarse block)
                if li < 2:
                    bufs.append(torch.empty((rows, o + Kq), dtype=torch.float32, device=dev))
                    extras.append((bufs[-1], o))
                elif widths[li] == widths[li - 2]:
                    bufs.append(bufs[li - 2])
                else:
                    bufs.append(torch.empty((rows, o + Kq), dtype=torch.float32, device=dev))
                    extras.append((bufs[-1], o))
            else:
                bufs.append(torch.empty((rows, o), dtype=torch.float32, device=dev))
        pointrend_gather(srcs + [up], idx, h, w, out=x, extras=extras)
        cur = x
        for li, ((_, b), o) in enumerate(zip(fcs, widths)):
            y = bufs[li]
            conv_fwd_fused(cur.view(1, 1, rows, cur.shape[1]), imgs[li], b, None, True, o, 1, 1, out=y.view(1, 1, rows, y.shape[1])[..., :o])
            cur = y
        p = conv_fwd(cur.view(1, 1, rows, cur.shape[1]), imgs[-1], head["predictor"][1], K, 1, 1, zero_to=Kq)
        pointrend_scatter(torch.as_strided(p, (rows, K), (Kq, 1)), idx, up)      # (the predictor's rows are Kq floats apart)
        if record is not None:
            record.append({"idx": idx, "uncertainty": unc})
        seg = up
    return seg


# ---- the dense contrastive loss over K * M anchor slots (include/ext/catseg_contrast.h; losses.DenseContrastiveLoss).  Thin wrappers: the
# loss module owns the buffers that live from its forward to its backward (Z, S / G).  r4(n) = n rounded up to a multiple of 4.
CONTRAST_MAX_ANCHORS = 8192


def r4(n):
    return (n + 3) // 4 * 4


def contrast_pick(labels, h, w, K, M, state=None, fixed_u=None, eval_mode=False):
    """the anchors of one batch -> (idx [A], label [A], n_pos [1]), int32 on the device, A = K * M.  labels: int64 [B, H, W]; (h, w): the
    feature map.  A training draw reads the 16-byte device state and advances its draw counter; with fixed_u (int32 [A]) or eval_mode
    (u24 = 2^23) the state does not move."""
    B, H, W = labels.shape
    A = K * M
    if A > CONTRAST_MAX_ANCHORS:
        raise ValueError("contrast_pick: K * M = %d anchor slots exceed %d" % (A, CONTRAST_MAX_ANCHORS))
    assert labels.dtype == torch.int64 and labels.is_contiguous()
    if fixed_u is not None:
        assert fixed_u.dtype == torch.int32 and fixed_u.numel() == A and fixed_u.is_contiguous()
    dev = labels.device
    idx = torch.empty(A, dtype=torch.int32, device=dev)
    lab = torch.empty(A, dtype=torch.int32, device=dev)
    n_pos = torch.empty(1, dtype=torch.int32, device=dev)
    need = lib.catseg_contrast_pick_workspace(B, h, w, K)
    ws = workspace(need, dev)
    draws = fixed_u is None and not eval_mode
    with _Timed("hbm:contrast_pick", 8.0 * B * h * w * 2 + 8.0 * A):      # the sampled labels twice (count, select), the slots' outputs
        check(lib.catseg_contrast_pick(ptr(labels), B, H, W, h, w, K, M, ptr(state) if draws else None, ptr(fixed_u) if fixed_u is not None else None,
                                       1 if eval_mode else 0, ptr(idx), ptr(lab), ptr(n_pos), ptr(ws), ws.numel(), stream()))
    return idx, lab, n_pos


def contrast_gather(feat, idx, eps, Z=None, inv_norm=None):
    """feat: NHWC [B, h, w, d] of any pixel stride -> (Z [A, r4(d)], inv_norm [A]): the normalised feature rows of the anchors"""
    B, h, w, d = feat.shape
    A = idx.numel()
    if Z is None:
        Z = torch.empty((A, r4(d)), dtype=torch.float32, device=feat.device)
    if inv_norm is None:
        inv_norm = torch.empty(A, dtype=torch.float32, device=feat.device)
    with _Timed("hbm:contrast_gather", 4.0 * A * (d + r4(d) + 2)):
        check(lib.catseg_contrast_gather(ptr(feat), ld_of(feat), B * h * w, d, ptr(idx), A, eps, ptr(Z), ptr(inv_norm), stream()))
    return Z, inv_norm


def contrast_rows(S, A, label, Wt, inv_tau, n_pos, ell=None):
    """S [A, lds] holds z_i . z_j; -> ell [A]; S is overwritten with G (zeros on the diagonal, in empty rows / columns and the pad columns)"""
    K = Wt.shape[0]
    if ell is None:
        ell = torch.empty(A, dtype=torch.float32, device=S.device)
    with _Timed("hbm:contrast_rows", 8.0 * A * r4(A)):
        check(lib.catseg_contrast_rows(ptr(S), S.stride(0), A, ptr(label), ptr(Wt), K, inv_tau, ptr(n_pos), ptr(ell), stream()))
    return ell


def contrast_finalize(ell, n_pos):
    loss = torch.empty(1, dtype=torch.float32, device=ell.device)
    with _Timed("hbm:contrast_finalize", 4.0 * ell.numel()):
        check(lib.catseg_contrast_finalize(ptr(ell), ell.numel(), ptr(n_pos), ptr(loss), stream()))
    return loss


def contrast_scatter_bwd(dZ, Z, inv_norm, idx, d, g, inv_tau, shape):
    """-> the dense NHWC gradient [B, h, w, d] of the feature map: zero but at the anchors' pixels"""
    B, h, w, _ = shape
    A = idx.numel()
    dfeat = torch.empty((B, h, w, d), dtype=torch.float32, device=dZ.device)
    with _Timed("hbm:contrast_scatter_bwd", 4.0 * B * h * w * d + 12.0 * A * d):
        check(lib.catseg_contrast_scatter_bwd(ptr(dZ), ptr(Z), dZ.stride(0), ptr(inv_norm), ptr(idx), A, d, ptr(g), inv_tau, ptr(dfeat), B * h * w,
                                              stream()))
    return dfeat
