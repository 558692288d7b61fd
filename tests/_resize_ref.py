"""References and case tables of tests/test_resize_ref_cpu.py and tests/test_resize_pool_gpu.py (needs no GPU).

References: F.interpolate(mode="bilinear") / F.adaptive_avg_pool2d and their autograd on the CPU, in float64 (the reference) or float32 (the
yardstick of tests/_yardstick.py), and an independent second reference of the resize: the dense weight matrices of the rule written out in
bilinear_matrix(), applied as the separable product Wy . x . Wx^T.

Case tables: every case names the launcher route it is meant to reach.  fwd_route() / bwd_route() transcribe the decisions of
catseg_bilinear_fwd / catseg_bilinear_bwd (csrc/pointwise.hip) line for line; they are a coverage claim -- test ids, and the assertion of
tests/test_resize_ref_cpu.py that each case reaches the route it names -- never a correctness check of a kernel."""
import functools
import math

import numpy as np
import torch
import torch.nn.functional as F

f32 = np.float32


# ------------------------------------------------------------------------------------------------------------------ references
def _nchw(t):
    return t.permute(0, 3, 1, 2)


def _nhwc(t):
    return t.permute(0, 2, 3, 1).contiguous()


def bilinear_ref(x_nhwc, Ho, Wo, align, dtype):
    """F.interpolate on the CPU in `dtype`; NHWC in, NHWC out"""
    x = _nchw(x_nhwc.detach().cpu().to(dtype))
    return _nhwc(F.interpolate(x, size=(Ho, Wo), mode="bilinear", align_corners=align))


def bilinear_bwd_ref(dy_nhwc, H, W, align, dtype):
    """autograd of F.interpolate on the CPU in `dtype`: the gradient of a (B, H, W, C) input for the (B, Ho, Wo, C) gradient dy"""
    dy = _nchw(dy_nhwc.detach().cpu().to(dtype))
    B, C, Ho, Wo = dy.shape
    x = torch.zeros(B, C, H, W, dtype=dtype, requires_grad=True)
    F.interpolate(x, size=(Ho, Wo), mode="bilinear", align_corners=align).backward(dy)
    return _nhwc(x.grad)


def bilinear_matrix(n_in, n_out, align):
    """The dense n_out x n_in weight matrix of a one-dimensional linear resize, in float64, from the rule itself:
         scale = (n_in - 1) / (n_out - 1) [0 when n_out == 1]   src = scale * dst                          align_corners=True
         scale = n_in / n_out                                   src = max(scale * (dst + .5) - .5, 0)      align_corners=False
         i0 = min(floor(src), n_in - 1), i1 = min(i0 + 1, n_in - 1), l1 = clamp(src - i0, 0, 1): row dst has 1 - l1 at i0 and l1 at i1."""
    m = torch.zeros(n_out, n_in, dtype=torch.float64)
    if align:
        scale = (n_in - 1) / (n_out - 1) if n_out > 1 else 0.0
    else:
        scale = n_in / n_out
    for dst in range(n_out):
        src = scale * dst if align else max(scale * (dst + 0.5) - 0.5, 0.0)
        i0 = min(int(math.floor(src)), n_in - 1)
        i1 = min(i0 + 1, n_in - 1)
        l1 = min(max(src - i0, 0.0), 1.0)
        m[dst, i0] += 1.0 - l1
        m[dst, i1] += l1
    return m


def bilinear_matrix_fwd(x_nhwc, Ho, Wo, align):
    _, H, W, _ = x_nhwc.shape
    return torch.einsum("oh,bhwc,pw->bopc", bilinear_matrix(H, Ho, align), x_nhwc.detach().cpu().double(), bilinear_matrix(W, Wo, align))


def bilinear_matrix_bwd(dy_nhwc, H, W, align):
    _, Ho, Wo, _ = dy_nhwc.shape
    return torch.einsum("oh,bopc,pw->bhwc", bilinear_matrix(H, Ho, align), dy_nhwc.detach().cpu().double(), bilinear_matrix(W, Wo, align))


def bilinear_taps(H, W, Ho, Wo, align):
    """the largest number of output pixels that feed one input pixel"""
    ny = int((bilinear_matrix(H, Ho, align) != 0).sum(0).max())
    nx = int((bilinear_matrix(W, Wo, align) != 0).sum(0).max())
    return ny * nx


def adaptive_avgpool_ref(x_nhwc, S, dtype):
    return _nhwc(F.adaptive_avg_pool2d(_nchw(x_nhwc.detach().cpu().to(dtype)), S))


def adaptive_avgpool_bwd_ref(dy_nhwc, H, W, dtype):
    dy = _nchw(dy_nhwc.detach().cpu().to(dtype))
    B, C, S, _ = dy.shape
    x = torch.zeros(B, C, H, W, dtype=dtype, requires_grad=True)
    F.adaptive_avg_pool2d(x, S).backward(dy)
    return _nhwc(x.grad)


# ------------------------------------------------------------------------------------------------------------------ inputs
def gen(*seed):
    return torch.Generator().manual_seed(sum((i + 1) * int(s) for i, s in enumerate(seed)) % (2 ** 31))


GROUPS = 4      # channel c has magnitude 10^-(c % 4) (times 1 .. 2): a kernel that mixes channels shows at the small channels' scale


def act(shape, g):
    """activation-like float32 data, (..., C): randn with per-channel magnitudes over four orders of magnitude and a few exact zeros"""
    C = shape[-1]
    mag = 10.0 ** -(torch.arange(C) % GROUPS).double() * (1.0 + torch.rand(C, generator=g, dtype=torch.float64))
    x = torch.randn(shape, generator=g, dtype=torch.float64) * mag
    x[torch.rand(shape, generator=g) < 0.1] = 0.0
    return x.float()


# ------------------------------------------------------------------------------------------------------------------ case tables
# FWD_CASES: (route, B, H, W, C, Ho, Wo, ldx, xoff, ldy, yoff, align): x is channels xoff .. xoff + C of an ldx-wide buffer, y channels
# yoff .. yoff + C of an ldy-wide one
FWD_CASES = (
    ("mode2", 2, 6, 10, 8, 24, 40, 8, 0, 8, 0, False),
    ("mode2", 3, 5, 7, 48, 5, 7, 48, 0, 48, 0, False),                    # identity
    ("mode2", 2, 9, 9, 8, 20, 31, 8, 0, 8, 0, True),                      # non-integer ratio
    ("mode2", 1, 40, 64, 8, 5, 8, 8, 0, 8, 0, False),                     # 8x downsample
    ("mode2", 2, 1, 1, 4, 3, 5, 4, 0, 4, 0, True),                        # H == W == 1: both scales 0
    ("mode2", 2, 5, 7, 8, 1, 1, 8, 0, 8, 0, True),                        # Ho == Wo == 1
    ("mode2", 1, 7, 1, 8, 14, 1, 8, 0, 8, 0, False),                      # W == Wo == 1
    ("mode2-slice", 2, 5, 9, 48, 10, 18, 64, 0, 112, 16, True),           # out of a 64-wide buffer into channels 16 .. 64 of a 112-wide one
    ("mode2-slice", 1, 2, 27, 96, 8, 108, 112, 8, 96, 0, False),          # source slice at channel 8
    ("mode2-slice", 2, 3, 20, 200, 6, 40, 208, 0, 208, 4, True),
    ("mode2-slice", 1, 1, 9, 8, 1, 9, 16, 4, 16, 8, True),                # H == Ho == 1
    ("lds", 2, 6, 10, 25, 24, 40, 32, 0, 25, 0, False),
    ("lds", 2, 6, 10, 25, 24, 40, 32, 4, 25, 0, True),                    # 16-byte aligned source slice
    ("lds", 1, 5, 7, 3, 10, 16, 4, 0, 3, 0, True),                        # C = 3: one thread's 4 floats span two pixels
    ("lds", 1, 4, 5, 2, 9, 10, 4, 0, 2, 0, False),                        # C = 2
    ("lds", 1, 3, 5, 1, 6, 12, 4, 0, 1, 0, True),                         # C = 1: four pixels per thread
    ("lds", 1, 2, 256, 25, 4, 512, 32, 0, 25, 0, False),                  # 2 W ldx 4 == 64 KB exactly
    ("mode1-lds-too-large", 1, 2, 257, 25, 4, 516, 32, 0, 25, 0, False),  # 2 W ldx 4 == 64 KB + 256 B
    ("mode1-downsample", 2, 33, 20, 25, 4, 12, 32, 0, 25, 0, False),
    ("mode1-downsample", 1, 5, 8, 25, 5, 8, 32, 0, 25, 0, False),         # identity
    ("mode1-downsample", 1, 5, 8, 25, 9, 16, 32, 0, 25, 0, True),         # Ho == 2 H - 1
    ("mode1-unaligned-source", 2, 6, 10, 8, 24, 40, 12, 2, 8, 0, False),  # C % 4 == 0, but the slice starts at channel 2
    ("mode1-unaligned-source", 2, 6, 10, 25, 24, 40, 25, 0, 25, 0, True),  # dense source: ldx % 4 != 0
    ("mode1-unaligned-source", 1, 5, 7, 3, 10, 16, 3, 0, 3, 0, True),
    ("mode1-unaligned-source", 1, 4, 5, 2, 9, 10, 2, 0, 2, 0, False),
    ("mode1-unaligned-source", 1, 3, 5, 1, 6, 12, 1, 0, 1, 0, False),
    ("mode0-odd-row", 2, 9, 9, 25, 20, 31, 32, 0, 25, 0, True),
    ("mode0-odd-row", 1, 4, 5, 1, 9, 11, 1, 0, 1, 0, False),
    ("mode0-odd-row", 2, 5, 7, 3, 1, 1, 3, 0, 3, 0, True),                # Ho == Wo == 1
    ("mode0-odd-row", 1, 2, 257, 25, 4, 514, 32, 0, 25, 0, False),        # (514 x 25 is no multiple of 4: not a MODE 1 row)
    ("mode0-padded-dest", 2, 6, 10, 25, 24, 40, 32, 0, 32, 0, False),
    ("mode0-padded-dest", 1, 5, 7, 25, 5, 7, 25, 0, 40, 3, False),
    ("mode0-padded-dest", 1, 7, 1, 8, 14, 1, 8, 0, 12, 2, False),         # C % 4 == 0, but the destination slice starts at channel 2
)

# BWD_CASES: (route, B, H, W, C, Ho, Wo, lddy, align, zero_to, lddx, dxoff): dy is channels 0 .. C of an lddy-wide buffer, dx channels
# dxoff .. dxoff + C of an lddx-wide one, with columns C .. zero_to behind it zeroed by the kernel.  The route is that of the default
# setting (catseg_debug_set_bilinear_bwd_fused(1)).
BWD_CASES = (
    ("fused1", 1, 5, 7, 3, 10, 16, 3, True, 0, 3, 0),
    ("fused1", 1, 5, 7, 3, 10, 16, 3, False, 4, 8, 0),
    ("fused1", 1, 1, 3, 8, 32, 6, 8, True, 0, 8, 0),                         # sh == 0, below the row limit
    ("fused1-multiseg", 2, 6, 10, 25, 24, 40, 25, False, 32, 32, 0),
    ("fused1-multiseg", 2, 9, 9, 8, 20, 31, 8, True, 0, 8, 0),                  # non-integer ratio
    ("fused1-multiseg", 2, 33, 20, 12, 4, 9, 12, False, 0, 12, 0),              # downsample to non-square
    ("fused1-lds-cap", 1, 3, 300, 25, 6, 600, 25, False, 32, 40, 0),            # many segments
    ("fused1-lds-cap", 1, 2, 104, 25, 8, 416, 25, False, 0, 25, 0),             # Wo C = 10400 > 10240 forces the first halving
    ("fused1-maxrows", 1, 1, 3, 8, 64, 6, 8, True, 0, 8, 0),                    # sh == 0: all 64 rows listed
    ("fused1-maxrows", 1, 2, 3, 8, 56, 6, 8, False, 0, 8, 0),                   # 2 / sh + 8 == 64
    ("twopass-rows-do-not-fit-rows1", 1, 1, 3, 8, 65, 6, 8, True, 0, 8, 0),
    ("twopass-rows-do-not-fit-rows1", 1, 2, 3, 8, 57, 6, 8, False, 0, 8, 0),
    ("twopass-rows-do-not-fit-rows1", 1, 1, 1, 4, 40, 9, 4, False, 0, 4, 0),    # 40x upsample of one pixel
    ("twopass-rows-do-not-fit-rows2", 1, 2, 3, 8, 57, 6, 16, False, 12, 16, 0),
    ("twopass-rows-do-not-fit-rows0", 1, 1, 3, 5, 65, 6, 5, True, 8, 8, 0),
    ("fused2", 1, 2, 27, 96, 8, 108, 112, False, 0, 96, 0),                     # 4 segments, 1 chunk
    ("fused2", 3, 5, 7, 48, 5, 7, 64, False, 0, 64, 8),                         # identity resize, into channels 8 .. 56 of a 64-wide buffer
    ("fused2", 1, 40, 64, 8, 5, 8, 16, False, 12, 24, 4),                       # 8x downsample: most input rows get nothing
    ("fused2", 1, 1, 9, 8, 1, 9, 16, True, 0, 8, 0),                            # H == Ho == 1
    ("fused2", 1, 7, 1, 8, 14, 1, 16, False, 0, 8, 0),                          # W == Wo == 1
    ("fused2", 2, 5, 7, 8, 1, 1, 16, True, 0, 8, 0),                            # Ho == Wo == 1
    ("fused2-chunks-ragged", 1, 2, 27, 100, 8, 108, 112, False, 112, 120, 0),   # 2 chunks, the last of 4 channels, zero_to = 112
    ("fused2-chunks-ragged", 2, 3, 20, 200, 6, 40, 208, True, 208, 216, 0),     # 3 chunks, the last of 8
    ("fused2-seg-above-8", 4, 128, 32, 4, 256, 64, 8, False, 0, 4, 0),          # segment of 16
    ("twopass-split-grid", 2, 6, 10, 25, 48, 80, 32, False, 32, 36, 0),
    ("twopass-mode0", 1, 5, 7, 25, 5, 7, 25, False, 0, 25, 0),
    ("twopass-mode0", 1, 4, 5, 1, 9, 11, 1, False, 0, 1, 0),                    # C = 1, odd Wo
    ("twopass-split-grid", 1, 5, 11, 25, 10, 15, 25, True, 28, 40, 5),          # both passes split; dx at channel 5 of a 40-wide buffer
)

# POOL_CASES: (what, B, S, H, W, C, ldx, xoff, lddx, dxoff): x is channels xoff .. xoff + C of an ldx-wide buffer, dx likewise
POOL_CASES = (
    ("one-bin", 1, 1, 9, 13, 24, 24, 0, 24, 0),
    ("one-bin", 3, 1, 9, 13, 24, 24, 0, 24, 0),
    ("second-channel-block-slices", 1, 2, 9, 13, 260, 268, 3, 264, 4),
    ("second-channel-block-slices", 3, 2, 9, 13, 260, 268, 3, 264, 4),
    ("overlapping-bins", 1, 3, 17, 30, 8, 8, 0, 8, 0),
    ("overlapping-bins", 3, 3, 17, 30, 8, 8, 0, 8, 0),
    ("overlapping-bins-slices", 1, 6, 17, 30, 24, 32, 5, 28, 0),
    ("overlapping-bins-slices", 3, 6, 17, 30, 24, 32, 5, 28, 0),
    ("more-bins-than-pixels-second-channel-block", 1, 6, 3, 4, 260, 260, 0, 260, 0),
    ("more-bins-than-pixels-second-channel-block", 3, 6, 3, 4, 260, 260, 0, 260, 0),
    ("even-bins", 1, 6, 6, 6, 4, 4, 0, 4, 0),
    ("even-bins", 3, 6, 6, 6, 4, 4, 0, 4, 0),
    ("S64-repeated-bins", 1, 64, 5, 7, 4, 4, 0, 4, 0),
    ("S64-repeated-bins", 3, 64, 5, 7, 4, 4, 0, 4, 0),
)

FWD_ROUTES = ("mode2", "mode2-slice", "lds", "mode1-downsample", "mode1-lds-too-large", "mode1-unaligned-source", "mode0-odd-row",
              "mode0-padded-dest")
BWD_ROUTES = ("fused1", "fused1-multiseg", "fused1-lds-cap", "fused1-maxrows", "fused2", "fused2-chunks-ragged", "fused2-seg-above-8",
              "twopass-rows-do-not-fit-rows1", "twopass-rows-do-not-fit-rows2", "twopass-rows-do-not-fit-rows0", "twopass-mode0",
              "twopass-split-grid")


def fwd_id(case):
    r, B, H, W, C, Ho, Wo, ldx, xoff, ldy, yoff, align = case
    return "%s-B%d-%dx%dx%d-to-%dx%d-x%d+%d-y%d+%d-%s" % (r, B, H, W, C, Ho, Wo, ldx, xoff, ldy, yoff, "ac" if align else "hp")


def bwd_id(case):
    r, B, H, W, C, Ho, Wo, lddy, align, zero_to, lddx, dxoff = case
    return "%s-B%d-%dx%dx%d-from-%dx%d-dy%d-%s-z%d-dx%d+%d" % (r, B, H, W, C, Ho, Wo, lddy, "ac" if align else "hp", zero_to, lddx, dxoff)


def pool_id(case):
    r, B, S, H, W, C, ldx, xoff, lddx, dxoff = case
    return "%s-B%d-S%d-%dx%dx%d-x%d+%d-dx%d+%d" % (r, B, S, H, W, C, ldx, xoff, lddx, dxoff)


# ------------------------------------------------------------------------------------------------------------------ the launchers, transcribed
BIL_MAXROWS = 64        # csrc/pointwise.hip:455
LDS_CAP = 10240         # csrc/pointwise.hip:975 (floats)


def resize_scale(n_in, n_out, align):
    """csrc/lerp.h:23-26 (resize_scale), in float32"""
    if align:
        return f32(n_in - 1) / f32(n_out - 1) if n_out > 1 else f32(0)
    return f32(n_in) / f32(n_out)


def lerp_setup(scale, dst, align, in_size):
    """csrc/lerp.h:7-22 (src_index, lerp_setup), in float32 without contraction: (i0, i1, l0, l1)"""
    if align:
        s = f32(scale * f32(dst))
    else:
        s = f32(f32(scale * f32(dst + 0.5)) - f32(0.5))
        if s < 0:
            s = f32(0)
    i0 = min(int(s), in_size - 1)
    i1 = i0 + (1 if i0 < in_size - 1 else 0)
    l1 = f32(s - f32(i0))
    return i0, i1, f32(f32(1) - l1), l1


def bil_cand_host(scale, i, align, out_size):
    """csrc/pointwise.hip:589-598 (bil_cand_host; bil_cand at 465-474 is the same text), in float32: (lo, hi)"""
    if scale > 0:
        if align:
            lo = int(math.floor(f32(i - 1) / scale)) - 1
            hi = int(math.ceil(f32(i + 1) / scale)) + 1
        else:
            lo = int(math.floor(f32(i - 0.5) / scale)) - 2
            hi = int(math.ceil(f32(i + 1.5) / scale)) + 1
    else:
        lo, hi = 0, out_size - 1
    return max(lo, 0), min(hi, out_size - 1)


def bil_fused_lds_floats(W, Wo, C, CC, mode, align, sw, seg, cap):
    """csrc/pointwise.hip:601-621 (bil_fused_lds_floats)"""
    need = 0
    for ix0 in range(0, W, seg):
        nix = min(seg, W - ix0)
        oxa = bil_cand_host(sw, ix0, align, Wo)[0]
        oxb = bil_cand_host(sw, ix0 + nix - 1, align, Wo)[1]
        if mode == 1:
            f0 = (oxa * C) & ~3
            f1 = min(((oxb + 1) * C + 3) & ~3, Wo * C)
            n = f1 - f0
        else:
            n = (oxb - oxa + 1) * CC
        if n > cap:
            return 0
        need = max(need, n)
    return need


def _aligned16(channel_offset):
    # the buffers are fresh torch allocations (256-byte aligned): a slice is 16-byte aligned when it starts at a channel that is a multiple of 4
    return channel_offset % 4 == 0


@functools.lru_cache(maxsize=None)
def fwd_route(case):
    """csrc/pointwise.hip:932-950 (catseg_bilinear_fwd): {"route": name, "kernel": kernel name}"""
    _, B, H, W, C, Ho, Wo, ldx, xoff, ldy, yoff, align = case
    ax, ay = _aligned16(xoff), _aligned16(yoff)
    if C % 4 == 0 and ldx % 4 == 0 and ldy % 4 == 0 and ax and ay:                    # :937
        return {"route": "mode2-slice" if (ldx != C or ldy != C) else "mode2", "kernel": "bilinear_fwd<2>"}
    if ldy == C and (Wo * C) % 4 == 0 and ay:                                         # :939
        lds = 2 * W * ldx * 4                                                         # :940
        if ldx % 4 == 0 and ax and lds <= 64 * 1024 and Ho >= 2 * H:                  # :941
            return {"route": "lds", "kernel": "bilinear_fwd_lds", "lds": lds}
        # the first of the three conditions that refuses the LDS kernel, in the order the launcher tests them
        why = "mode1-unaligned-source" if not (ldx % 4 == 0 and ax) else "mode1-lds-too-large" if lds > 64 * 1024 else "mode1-downsample"
        return {"route": why, "kernel": "bilinear_fwd<1>", "lds": lds}
    return {"route": "mode0-odd-row" if ldy == C else "mode0-padded-dest", "kernel": "bilinear_fwd<0>"}      # :947


@functools.lru_cache(maxsize=None)
def bwd_route(case, fused=1):
    """csrc/pointwise.hip:951-1013 (catseg_bilinear_bwd) under catseg_debug_set_bilinear_bwd_fused(fused): {"route": name, "kernel": ...}"""
    _, B, H, W, C, Ho, Wo, lddy, align, zero_to, lddx, dxoff = case
    out = {}
    mode = 1 if (lddy == C and (Wo * C) % 4 == 0) else (2 if (C % 4 == 0 and lddy % 4 == 0) else 0)      # :963 (dy starts its buffer: aligned)
    shf = resize_scale(H, Ho, align)                                                                     # :964
    rows_est = f32(f32(2) / shf + f32(8)) if shf > 0 else f32(Ho)
    rows_fit = bool(rows_est <= f32(BIL_MAXROWS))                                                        # :966
    out.update(mode=mode, rows_fit=rows_fit)
    if fused and mode != 0 and rows_fit:                                                                 # :962, :967
        sw = resize_scale(W, Wo, align)
        CC = C if mode == 1 else min(C, 96)                                                              # :973
        nchunk = 1 if mode == 1 else (C + CC - 1) // CC                                                  # :974
        seg, need, cap_halvings = W, 0, 0
        while seg >= 1:                                                                                  # :978
            need = bil_fused_lds_floats(W, Wo, C, CC, mode, align, sw, seg, LDS_CAP)
            if need != 0:
                break
            seg = (seg + 1) // 2 if seg > 1 else 0
            cap_halvings += 1
        while seg > 8 and B * H * ((W + seg - 1) // seg) * nchunk < 1024:                                # :979-982
            seg = (seg + 1) // 2
            need = bil_fused_lds_floats(W, Wo, C, CC, mode, align, sw, seg, LDS_CAP)
        if seg >= 1 and need > 0:                                                                        # :983
            nseg = (W + seg - 1) // seg
            out.update(kernel="bilinear_bwd_fused<%d>" % mode, seg=seg, nseg=nseg, nchunk=nchunk, CC=CC, lds_floats=need,
                       cap_halvings=cap_halvings, grid=(B * H, nseg * nchunk))
            if mode == 1:
                # (at the row limit: the host's estimate, or the row count where sh == 0, is the last one that fits)
                out["route"] = ("fused1-maxrows" if rows_est > f32(BIL_MAXROWS - 1) else "fused1-lds-cap" if cap_halvings
                                else "fused1-multiseg" if nseg > 1 else "fused1")
            else:
                out["route"] = "fused2-chunks-ragged" if (nchunk > 1 and C % CC) else "fused2-seg-above-8" if seg > 8 else "fused2"
            return out
    per_row = (2048 + B * H - 1) // (B * H)
    ysplit_r = max(min(per_row, (Wo * C + 255) // 256), 1)                                               # :997-998, :1001
    ysplit_c = max(min(per_row, (W * C + 255) // 256), 1)                                                # :999-1000, :1009
    rows_mode = mode                                                                                     # :1003-1008: the conditions of :963 again
    out.update(kernel="bilinear_bwd_rows<%d>+cols" % rows_mode, ysplit_r=ysplit_r, ysplit_c=ysplit_c)
    if not fused:
        out["route"] = "twopass-forced"
    elif not rows_fit:
        out["route"] = "twopass-rows-do-not-fit-rows%d" % rows_mode
    else:
        out["route"] = "twopass-split-grid" if (ysplit_r > 1 or ysplit_c > 1) else "twopass-mode0"
    return out


def listed_rows(case):
    """the largest number of output rows with a non-zero weight for one input row, as bilinear_bwd_fused_kernel lists them
    (csrc/pointwise.hip:488-516) -- what BIL_MAXROWS has to hold"""
    _, B, H, W, C, Ho, Wo, lddy, align, zero_to, lddx, dxoff = case
    sh = resize_scale(H, Ho, align)
    worst = 0
    for iy in range(H):
        lo, hi = bil_cand_host(sh, iy, align, Ho)
        n = 0
        for oy in range(lo, hi + 1):
            y0, y1, l0, l1 = lerp_setup(sh, oy, align, H)
            w = f32(0)
            if y0 == iy:
                w = f32(w + l0)
            if y1 == iy:
                w = f32(w + l1)
            n += 1 if w != 0 else 0
        worst = max(worst, n)
    return worst
