"""Cases, operands, buffers and references for the CATSEG_OPERANDS_F32 convolutions (csrc/igemm.hip, csrc/wgrad_direct.hip) in all three
directions; importable without a GPU.  tests/test_conv_exact_cpu.py holds this file to its own preconditions, tests/test_conv_exact_gpu.py
holds the kernels to it.  The method is that of tests/_gemm_ref.py, whose helpers are reused.

The operands are INTEGERS stored as float32 with (reduction length) * max|a| * max|b| + |bias| + |residual| + |initial dx| < 2^23: every
product and every partial sum, in any order, on any tile form, with or without a K split, through one or two accumulator levels, is an
integer below 2^24 and therefore exact in fp32 -- the GPU result has to equal the float64 convolution bit for bit and the comparison needs
no tolerance.  Where the reduction is at most 256 long one operand reaches 4099 (odd, > 2^12): a reduced-precision operand path cannot hold
it.  Nothing here speaks about rounding or summation order; the tolerance tests (test_kernels_gpu.py, test_w48_gpu.py) keep that job.

The buffers follow the operand contract written at catseg_conv2d_fwd / _bwd_data / _bwd_weight in include/catseg.h ("Operand contract of
the F32 convolutions"), sentence by sentence:
  * x, y, dy, dx and the residual are channel slices of wider buffers (ld > C, the slice starts 4 floats into a pixel), with a head in
    front of the first pixel and rows behind the last; w, dw, bias and dbias have a head and a tail.  Every float outside a logical operand
    is NaN: "never read" is then a statement the result shows.
  * backward-data: the pad columns [Cout, r4(Cout)) of dy are ZERO, as the contract demands (they meet zeros that stand for w's rows >=
    Cout).  backward-weight: the same columns "may hold anything" -- they are NaN, and so are the columns [Cout, 32) that the 32-float-row
    dbias kernel reads.
  * every destination starts as NaNs with one payload per float (for `accumulate`: small integers in the logical block); after the launch
    every float the launch must not touch has to keep its bits and every [Cout, zero_to) float has to be +0.
The stem's x and w are produced on the device by nchw3_to_nhwc4 / stem_pack_weight (dense, ldx == 4): they carry no NaNs."""
import collections
import functools
import math
import os
import sys

import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _gemm_ref as GR  # noqa: E402

LIMIT, C0_MAX, HEAD = GR.LIMIT, GR.C0_MAX, GR.HEAD
roundup4, nan_pattern, bits = GR.roundup4, GR.nan_pattern, GR.bits
EXTRA = 3 * C0_MAX      # |bias| + |residual| + |initial dx|, each at most C0_MAX

FWD, DGRAD, WGRAD = "fwd", "dgrad", "wgrad"
DIRECTIONS = (FWD, DGRAD, WGRAD)
LAYOUT = {FWD: GR.NT, DGRAD: GR.NN, WGRAD: GR.TN}     # the operand layout of csrc/igemm.hip each direction runs on

Geo = collections.namedtuple("Geo", "B H W Cin Cout k stride pad dil groups stem ldy")


def G(B, H, W, Cin, Cout, k, stride, pad, dil, groups=1, stem=False, ldy=0):
    """ldy: 0 = dy / y is a slice of a wider buffer; else its exact pixel stride (32: the rows of class logits)"""
    return Geo(B, H, W, Cin, Cout, k, stride, pad, dil, groups, stem, ldy)


def geo_id(g):
    return "b%d_%dx%d_c%d_o%d_k%d_s%d_p%d_d%d" % tuple(g[:9]) + ("_g%d" % g.groups if g.groups > 1 else "") + ("_stem" if g.stem else "") + (
        "_ldy%d" % g.ldy if g.ldy else "")


def out_hw(g):
    return ((g.H + 2 * g.pad - g.dil * (g.k - 1) - 1) // g.stride + 1, (g.W + 2 * g.pad - g.dil * (g.k - 1) - 1) // g.stride + 1)


def rows_out(g):
    Ho, Wo = out_hw(g)
    return g.B * Ho * Wo


def reduction(direction, g):
    taps = g.k * g.k
    if direction == FWD:
        return taps * g.Cin // g.groups
    if direction == DGRAD:
        return taps * g.Cout // g.groups
    return rows_out(g)


def magnitudes(K):
    """_gemm_ref.magnitudes' rule with room for the terms added to the sum: K max|a| max|b| + EXTRA < LIMIT; max|a| = 4099 where K <= 256"""
    room = LIMIT - 1 - EXTRA
    if K <= 256:
        amax = 4099
        bmax = room // (K * amax)
    else:
        amax = bmax = math.isqrt(room // K)
    assert bmax >= 1 and K * amax * bmax + EXTRA < LIMIT
    return amax, bmax


def gemm_dims(direction, g):
    """(M, N) of the GEMM a launch tiles: forward rows = output pixels, columns = Cout (per group); backward-data rows = input pixels
    (stride 1), columns = Cin; backward-weight rows = Cout, columns = taps x Cin (the stem: 32 per filter row)"""
    if direction == FWD:
        return rows_out(g), g.Cout // g.groups
    if direction == DGRAD:
        return g.B * g.H * g.W, g.Cin // g.groups
    return g.Cout // g.groups, 32 if g.stem else g.k * g.k * g.Cin // g.groups


# ---------------------------------------------------------------------------------------------------------------------------------
# The geometries: the smallest shapes at which the edges in question exist.

NAMED = {
    FWD: [
        G(20, 1, 1, 8, 5, 1, 1, 0, 1),            # one-pixel images, Cout % 4 != 0
        G(5, 2, 3, 16, 17, 3, 1, 1, 1),           # 6-pixel images, one column past the 16-wide form
        G(1, 2, 40, 8, 33, 3, 1, 1, 1),           # two rows high, M = 80 past a 64-row tile, one column past 32
        G(2, 9, 11, 12, 49, 3, 1, 2, 2),          # dilation 2, M = 198 past 192 and 128, one column past 48
        G(1, 13, 17, 8, 65, 3, 2, 1, 1),          # stride 2 on odd extents, M = 63, one column past 64
        G(1, 19, 23, 4, 97, 3, 1, 12, 12),        # dilation 12: most taps outside the image; M = 437 past 256, one column past 96
        G(2, 8, 9, 4, 129, 7, 1, 3, 1),           # 49 taps without stem4: the non-FAST kernel; one column past 128
        G(1, 16, 16, 8, 193, 1, 2, 0, 1),         # 1x1 stride 2, M = 64 exactly, one column past 192
        G(1, 16, 16, 16, 256, 1, 1, 0, 1),        # whole tiles only on the square forms: the unpredicated epilogue
        G(1, 16, 16, 16, 192, 1, 1, 0, 1),        # ... and on the 48-wide forms
        G(2, 6, 7, 32, 48, 3, 1, 1, 1, 4),        # grouped
        G(1, 5, 5, 8, 10, 3, 1, 1, 1, 2),         # grouped, forward only (Cout / groups % 4 != 0)
        G(2, 13, 15, 3, 64, 7, 2, 3, 1, stem=True),
    ],
    DGRAD: [
        G(20, 1, 1, 8, 5, 1, 1, 0, 1),            # the forward shapes with the roles exchanged: N = Cin crosses 48, 64, 96, 128, 192;
        G(5, 2, 3, 16, 17, 3, 1, 1, 1),           # Cout = 5, 17, 25: zero pad columns in dy
        G(1, 2, 40, 52, 25, 3, 1, 1, 1),
        G(2, 9, 11, 68, 5, 3, 1, 2, 2),
        G(1, 13, 17, 100, 17, 3, 2, 1, 1),
        G(1, 19, 23, 132, 4, 3, 1, 12, 12),
        G(2, 8, 9, 196, 5, 7, 1, 3, 1),           # 49 taps at stride 1: the non-FAST kernel
        G(1, 16, 16, 64, 8, 1, 2, 0, 1),
        G(1, 16, 16, 256, 16, 1, 1, 0, 1),
        G(1, 16, 16, 192, 16, 1, 1, 0, 1),
        G(2, 6, 7, 32, 48, 3, 1, 1, 1, 4),
        G(1, 1, 5, 8, 8, 3, 2, 1, 1),             # H below the stride: a parity class has no rows
        G(2, 7, 9, 8, 12, 1, 2, 0, 1),            # three parity classes receive no tap: zeros, or left as they were under accumulate
        G(1, 9, 11, 8, 8, 3, 2, 2, 2),            # stride and dilation share a factor
        G(1, 10, 11, 8, 8, 3, 3, 1, 1),           # stride 3: nine classes, one launch each
        G(2, 7, 8, 8, 5, 5, 3, 2, 1),
        G(1, 24, 16, 32, 25, 16, 8, 4, 1, ldy=32),  # FCN's ConvTranspose2d(16, stride 8, pad 4) on a 3 x 2 dy of 25 classes in 32-float rows
        G(2, 9, 10, 4, 8, 13, 2, 6, 1),           # 49 taps per parity class: the generic path
    ],
    WGRAD: [
        G(1, 1, 1, 8, 5, 1, 1, 0, 1),             # 1 row; M = Cout = 5
        G(1, 3, 5, 4, 49, 3, 1, 1, 1),            # 15 rows; M one past 48
        G(1, 4, 4, 68, 65, 1, 1, 0, 1),           # 16 rows; M one past 64, N = taps x Cin one column (of four) past 64
        G(1, 1, 17, 132, 97, 1, 1, 0, 1),         # 17 rows; M one past 96, N past 128
        G(20, 1, 1, 260, 129, 1, 1, 0, 1),        # one-pixel images: 16 images per K step; M one past 128, N past 256
        G(5, 2, 3, 16, 193, 3, 1, 1, 1),          # 6-pixel images: all three carries of the row stepping in one step; M one past 192
        G(1, 2, 40, 8, 257, 3, 1, 1, 1),          # M one past 256
        G(2, 9, 11, 12, 17, 3, 1, 2, 2),
        G(1, 13, 17, 8, 33, 3, 2, 1, 1),
        G(1, 19, 23, 4, 25, 3, 1, 12, 12),
        G(2, 8, 9, 4, 12, 7, 1, 3, 1),
        G(1, 26, 40, 8, 25, 1, 1, 0, 1, ldy=32),  # 1040 rows: the forced splits; dbias through the 32-float-row kernel
        G(1, 26, 40, 8, 49, 1, 1, 0, 1),          # ... and through the general one, more than 1024 rows
        G(2, 6, 7, 32, 48, 3, 1, 1, 1, 4),
        G(2, 13, 15, 3, 64, 7, 2, 3, 1, stem=True),
        G(2, 256, 17, 48, 48, 3, 1, 1, 1),        # the direct kernel: 1024 strips, the second strip of every row holds one pixel
        G(2, 256, 17, 96, 96, 3, 1, 1, 1),
    ],
}

SPLITS = (1, 2, 3, 7, 12, 65)     # forced split counts at 1040 rows (12: rounding rows-per-split up to 16 leaves 11; 65: the wide slab reduction)


def _select():
    """the geometries with a role of their own, picked by PROPERTY (never by position in NAMED)"""
    fwd, dg, wg = (NAMED[d] for d in DIRECTIONS)
    tiny_fwd = [g for g in fwd if g.H <= 2]                                      # images at most two rows high: run on every forward form
    tiny_wgrad = [g for g in wg if g.H <= 2 and rows_out(g) > 17]                # ... and the row stepping of backward-weight on every form
    strided = [g for g in dg if g.stride > 1]                                    # EVERY strided backward-data geometry runs on every form
    # what takes the generic (not FAST) gather: more than 32 taps at stride 1, and the stem -- on every form as well
    generic = {d: [g for g in NAMED[d] if g.stem or (g.k * g.k > 32 and g.stride == 1)] for d in DIRECTIONS}
    split, = [g for g in wg if rows_out(g) == 1040 and g.ldy == 32]
    direct = [g for g in wg if g.Cin == g.Cout and g.Cin in (48, 96) and (g.k, g.stride, g.pad, g.dil) == (3, 1, 1, 1)]
    return tiny_fwd, tiny_wgrad, strided, generic, split, direct


TINY_FWD, TINY_WGRAD, STRIDED_DGRAD, GENERIC, SPLIT_GEO, DIRECT = _select()


def split_plan(rows, forced):
    """(rows per split, splits that run) of a forced split count: plan_tiles in csrc/igemm.hip"""
    rps = ((rows + forced - 1) // forced + 15) // 16 * 16
    return rps, (rows + rps - 1) // rps


def shape3(rows):
    """(B, H, W) with B H W == rows: W the largest divisor up to 41, two images where that leaves an even number of rows"""
    W = max(w for w in range(1, min(rows, 41) + 1) if rows % w == 0)
    rest = rows // W
    B = 2 if rest % 2 == 0 and rest >= 4 else 1
    return B, rest // B, W


def form_geos(direction, tm, tn):
    """for a (tm x tn) tile of the direction's layout: (a case inside one tile, one a row and a column past it, one of whole tiles only).
    Columns come in fours in backward-data (Cin) and backward-weight (taps x Cin): there 'a column past' is tn + 4."""
    if direction == FWD:
        return (G(*shape3(tm - 7), 8, min(tn, 16) - 3, 3, 1, 1, 1), G(*shape3(tm + 1), 8, tn + 1, 3, 1, 1, 1), G(*shape3(2 * tm), 8, tn, 3, 1, 1, 1))
    if direction == DGRAD:
        return (G(*shape3(tm - 7), 12, 5, 3, 1, 1, 1), G(*shape3(tm + 1), tn + 4, 17, 3, 1, 1, 1), G(*shape3(2 * tm), tn, 8, 3, 1, 1, 1))
    return (G(1, 3, 5, 4, tm - 7, 3, 1, 1, 1), G(1, 1, 17, tn + 4, tm + 1, 1, 1, 0, 1), G(1, 4, 4, tn, 2 * tm, 1, 1, 0, 1))


def forms(direction):
    """[(form, mi, ni, tile height, tile width)] of the direction's layout: the lists and the tile expression of tests/test_gemm_gpu.py (that
    module imports without a GPU), which restate CS_FORM in launch_igemm"""
    import test_gemm_gpu as TG
    return [(f, mi, ni) + tuple(TG._tile(f, mi, ni)) for f, mi, ni in TG.FORMS[LAYOUT[direction]]]


def _cases(direction):
    out = list(NAMED[direction])
    for _, _, _, tm, tn in forms(direction):
        out += [g for g in form_geos(direction, tm, tn) if g not in out]
    return out


CASES = {d: _cases(d) for d in DIRECTIONS}


# ---------------------------------------------------------------------------------------------------------------------------------
# Buffers: a Slot is a strided view of a flat buffer and the buffer's length

Slot = collections.namedtuple("Slot", "shape strides offset numel")


def act_slot(B, H, W, C, width=None, ld=0):
    """[B, H, W, C] pixels of `ld` floats; ld == 0: a slice that starts 4 floats into pixels of r4(width) + 8 floats.  Head, four rows and
    12 floats behind the last pixel, tail."""
    width = max(C, width or 0)
    off = 0 if ld else 4
    ld = ld or roundup4(width) + 8
    assert ld % 4 == 0 and off + width <= ld
    return Slot((B, H, W, C), (H * W * ld, W * ld, ld, 1), HEAD + off, HEAD + B * H * W * ld + 4 * ld + 12 + HEAD)


def weight_slot(O, I, k):
    """[O, I, k, k] in the physical OHWI order, dense, with a head and a tail"""
    return Slot((O, I, k, k), (k * k * I, 1, k * I, I), HEAD, HEAD + O * k * k * I + HEAD)


def vector_slot(C):
    return Slot((C,), (1,), 4, C + 8)


def view(flat, slot, cols=None):
    """the logical block of a flat buffer (CPU or GPU); cols = (lo, hi): those channel columns of an activation's pixels instead"""
    if cols is None:
        return torch.as_strided(flat, slot.shape, slot.strides, slot.offset)
    return torch.as_strided(flat, slot.shape[:-1] + (cols[1] - cols[0],), slot.strides, slot.offset + cols[0])


def ld_of(slot):
    return slot.strides[2]


def filled(slot, vals, zero=None, salt=0):
    """NaNs of distinct payloads, `vals` in the logical block, zeros in the channel columns zero = (lo, hi)"""
    flat = nan_pattern(slot.numel, salt)
    view(flat, slot)[...] = vals
    if zero is not None and zero[1] > zero[0]:
        view(flat, slot, zero)[...] = 0.0
    return flat


def dest(slot, initial=None, salt=77):
    """a destination: payload NaNs everywhere; for an accumulating launch `initial` (small integers) in the logical block"""
    flat = nan_pattern(slot.numel, salt)
    if initial is not None:
        view(flat, slot)[...] = initial
    return flat


def check_dest(slot, before, after, want, zero_to=0, what="", plus_zero=None):
    """the contract's statements about a destination, on the CPU: `before` / `after` are the flat buffer around the launch(es), `want` the
    float64 reference of the logical block; plus_zero: mask of the logical elements that have to be +0 to the bit (torch.equal takes -0)"""
    C = slot.shape[-1]
    got = view(after, slot)
    assert float(want.abs().max()) < 2 ** 24
    assert not torch.isnan(got).any(), "%s: %d NaNs in the logical result (a pad, a gap or an unwritten element)" % (what, int(torch.isnan(got).sum()))
    assert torch.equal(got, want.float()) and torch.equal(got.double(), want), "%s: %d of %d elements differ from the float64 reference, max |diff| %g" % (
        what, int((got.double() != want).sum()), want.numel(), float((got.double() - want).abs().max()))
    if plus_zero is not None:
        assert bool(plus_zero.any()) and not bool(bits(got)[plus_zero].any()), "%s: an element that has to be +0 is not (-0?)" % what
    touched = torch.zeros(after.numel(), dtype=torch.bool)
    view(touched, slot)[...] = True
    if zero_to > C:
        z = bits(view(after, slot, (C, zero_to)))
        assert torch.equal(z, torch.zeros_like(z)), "%s: columns [Cout, zero_to) are not +0" % what
        view(touched, slot, (C, zero_to))[...] = True
    same = bits(after) == bits(before)
    assert bool(same[~touched].all()), "%s: %d floats outside the written columns changed" % (what, int((~same[~touched]).sum()))


# ---------------------------------------------------------------------------------------------------------------------------------
# Problems: operands and float64 references of one geometry, built once and left unchanged

def ints(gen, maxabs, shape):
    v = torch.randint(-maxabs, maxabs + 1, shape, generator=gen).float()
    v.view(-1)[0] = maxabs
    v.view(-1)[-1] = -maxabs
    return v


def _gen(direction, g):
    return torch.Generator().manual_seed(1000 * DIRECTIONS.index(direction) + sum((i + 1) * int(v) for i, v in enumerate(g)))


def nchw(t):
    return t.permute(0, 3, 1, 2)


def nhwc(t):
    return t.permute(0, 2, 3, 1)


FWD_VARIANTS = ("plain", "bias_zero", "fused")      # no bias; bias and zero_to; bias, residual and relu through conv_fwd_fused

FwdProblem = collections.namedtuple("FwdProblem", "g x w bias res ref xs ws bs rs ys X W Bias Res amax bmax")


@functools.lru_cache(maxsize=None)
def fwd_problem(g):
    """x [B, H, W, Cin], w [Cout, Cin / groups, k, k], bias, residual as values (x, w, ...), slots (xs, ws, ...) and flat buffers (X, W, ...);
    ref: the float64 convolution without bias.  The stem's x is the 3-channel image; its X and W are None (made on the device)."""
    amax, bmax = magnitudes(reduction(FWD, g))
    gen = _gen(FWD, g)
    Ho, Wo = out_hw(g)
    x = ints(gen, amax, (g.B, g.H, g.W, g.Cin))
    w = ints(gen, bmax, (g.Cout, g.Cin // g.groups, g.k, g.k))
    bias = ints(gen, C0_MAX, (g.Cout,))
    res = ints(gen, C0_MAX, (g.B, Ho, Wo, g.Cout))
    ref = nhwc(F.conv2d(nchw(x).double(), w.double(), None, g.stride, g.pad, g.dil, g.groups)).contiguous()
    xs, ws = act_slot(g.B, g.H, g.W, g.Cin), weight_slot(g.Cout, g.Cin // g.groups, g.k)
    bs, rs = vector_slot(g.Cout), act_slot(g.B, Ho, Wo, g.Cout)
    ys = act_slot(g.B, Ho, Wo, g.Cout, width=fwd_zero_to(g, "bias_zero"), ld=g.ldy)
    X, W = (None, None) if g.stem else (filled(xs, x, salt=1), filled(ws, w, salt=2))
    return FwdProblem(g, x, w, bias, res, ref, xs, ws, bs, rs, ys, X, W, filled(bs, bias, salt=3), filled(rs, res, salt=4), amax, bmax)


def fwd_zero_to(g, variant):
    """zero_to of a forward variant: one 4-column group past r4(Cout) (the grouped launch takes none)"""
    return roundup4(g.Cout) + 4 if variant == "bias_zero" and g.groups == 1 else 0


def fwd_want(p, variant, conv=None):
    """the float64 result of a forward variant; conv: another convolution result in place of the reference (the CPU tests' wrong kernels)"""
    y = p.ref if conv is None else conv
    if variant != "plain":
        y = y + p.bias.double()
    if variant == "fused":
        if p.g.groups == 1:
            y = y + p.res.double()
        y = y.clamp_min(0.0)
    return y


DgradProblem = collections.namedtuple("DgradProblem", "g dy w dx0 ref untapped dys ws dxs DY W amax bmax")


@functools.lru_cache(maxsize=None)
def dgrad_problem(g):
    """dy [B, Ho, Wo, Cout] with ZERO pad columns [Cout, r4(Cout)), w, the integers dx0 an accumulating launch starts from; ref: float64 dx;
    untapped: mask of the dx elements no tap reaches (None where every pixel is reached): a plain launch writes +0 there"""
    amax, bmax = magnitudes(reduction(DGRAD, g))
    gen = _gen(DGRAD, g)
    Ho, Wo = out_hw(g)
    dy = ints(gen, amax, (g.B, Ho, Wo, g.Cout))
    w = ints(gen, bmax, (g.Cout, g.Cin // g.groups, g.k, g.k))
    dx0 = ints(gen, C0_MAX, (g.B, g.H, g.W, g.Cin))
    ref = nhwc(torch.nn.grad.conv2d_input((g.B, g.Cin, g.H, g.W), w.double(), nchw(dy).double(), g.stride, g.pad, g.dil, g.groups)).contiguous()
    reach = torch.nn.grad.conv2d_input((g.B, g.Cin, g.H, g.W), torch.ones_like(w).double(), torch.ones_like(nchw(dy)).double(), g.stride, g.pad, g.dil, g.groups)
    untapped = nhwc(reach == 0).contiguous()
    untapped = untapped if bool(untapped.any()) else None
    dys, ws, dxs = act_slot(g.B, Ho, Wo, g.Cout, width=roundup4(g.Cout), ld=g.ldy), weight_slot(g.Cout, g.Cin // g.groups, g.k), act_slot(g.B, g.H, g.W, g.Cin)
    return DgradProblem(g, dy, w, dx0, ref, untapped, dys, ws, dxs, filled(dys, dy, zero=(g.Cout, roundup4(g.Cout)), salt=5), filled(ws, w, salt=6), amax, bmax)


WgradProblem = collections.namedtuple("WgradProblem", "g x dy ref dbias xs dys dws dbs X DY amax bmax")


@functools.lru_cache(maxsize=None)
def wgrad_problem(g):
    """x, dy [B, Ho, Wo, Cout] with NaN pad columns; ref: float64 dw [Cout, Cin / groups, k, k], dbias: the float64 column sum"""
    amax, bmax = magnitudes(reduction(WGRAD, g))
    gen = _gen(WGRAD, g)
    Ho, Wo = out_hw(g)
    dy = ints(gen, amax, (g.B, Ho, Wo, g.Cout))
    x = ints(gen, bmax, (g.B, g.H, g.W, g.Cin))
    ref = torch.nn.grad.conv2d_weight(nchw(x).double(), (g.Cout, g.Cin // g.groups, g.k, g.k), nchw(dy).double(), g.stride, g.pad, g.dil, g.groups)
    xs, dys = act_slot(g.B, g.H, g.W, g.Cin), act_slot(g.B, Ho, Wo, g.Cout, ld=g.ldy)
    X = None if g.stem else filled(xs, x, salt=7)
    return WgradProblem(g, x, dy, ref, dy.double().sum((0, 1, 2)), xs, dys, weight_slot(g.Cout, g.Cin // g.groups, g.k), vector_slot(g.Cout), X,
                        filled(dys, dy, salt=8), amax, bmax)


PROBLEM = {FWD: fwd_problem, DGRAD: dgrad_problem, WGRAD: wgrad_problem}
