"""catseg_bilinear_fwd / catseg_bilinear_bwd (csrc/pointwise.hip) on every route of their launchers, and catseg_adaptive_avgpool_fwd / bwd
(csrc/pool.hip) past one channel block and in channel slices, against float64.

The cases, the routes they reach and the references are those of tests/_resize_ref.py (tests/test_resize_ref_cpu.py shows without a GPU
that every route is reached).  Every floating-point comparison is _yardstick.within(): the kernel may be off float64 F.interpolate /
F.adaptive_avg_pool2d (and their autograd) by at most 4 x what the same torch lines in float32 on the CPU are off, floor 4 ulp of the
reference's scale; in a case that reads or writes a channel slice the same bar also holds per channel group (channel c has magnitude
10^-(c % 4): a kernel that mixed channels would show at the small channels' scale).  Zeroed pad columns, untouched surroundings of a
slice, repeated calls and the fused launch against the two passes are exact (bit) comparisons.  The adjoint identity
<fwd(x), dy> == <x, bwd(dy)> ties the forward kernels to the backward ones with no reference in between.

Worst ratio of a kernel's error to the yardstick (RATIO lines, pytest -s; the bar is 4), MI355X:
    bilinear_fwd<0>            1.064   9x9x25 -> 20x31, align_corners, channel group 3
    bilinear_fwd<1>            1.084   6x10x8 -> 24x40 out of channels 2 .. 10 of 12, channel group 0
    bilinear_fwd<2>            1.002   3x20x200 -> 6x40 into channels 4 .. 204 of 208, channel group 1
    bilinear_fwd_lds           1.160   6x10x25 -> 24x40 out of channels 4 .. 29 of 32, accumulating
    bilinear_bwd_fused<1>      1.114   9x9x8 <- 20x31, align_corners, accumulating
    bilinear_bwd_fused<2>      1.030   3x20x200 <- 6x40, channel group 3
    bilinear_bwd_rows<0>+cols  1.475   1x3x5 <- 65x6, align_corners, channel group 2
    bilinear_bwd_rows<1>+cols  3.100   1x1x4 <- 40x9 (360 output pixels into one input pixel), accumulating; 2.455 overwriting
    bilinear_bwd_rows<2>+cols  1.030   3x20x200 <- 6x40, channel group 3
    adaptive_avgpool_fwd       1.000   S=2, 9x13x260 out of a slice
    adaptive_avgpool_bwd       1.110   S=6, 17x30x24 into a slice, channel group 1
The adjoint identity holds to 0.019 of its bound at worst (7x1x8 <-> 14x1).  The whole file takes about 2 s."""
import functools

import pytest
import torch

import _resize_ref as R
from _yardstick import EPS32, within      # the shared bound: 4 x the fp32 CPU error, floor 4 ulp of the scale

pytestmark = pytest.mark.gpu
F64, F32 = torch.float64, torch.float32


@pytest.fixture(scope="module")
def ops():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from miccai2021_cataract_semantic_segmentation_amd import ops as o
    return o


def nan_buffer(shape, ld, off, inner):
    """a (..., ld) float32 buffer of NaN with `inner` (..., C) at channels off .. off + C: (the buffer on the device, the view of the slice)"""
    buf = torch.full(tuple(shape[:-1]) + (ld,), float("nan"), dtype=F32)
    buf[..., off:off + shape[-1]] = inner
    return on_device(buf, off, shape[-1])


def on_device(buf, off, C):
    d = buf.cuda()
    return d, (d if (off == 0 and C == d.shape[-1]) else d[..., off:off + C])


def bits(t):
    return t.contiguous().view(torch.int32)


def same_bits(a, b):
    return torch.equal(bits(a), bits(b))


NAN_BITS = int(torch.tensor(float("nan"), dtype=F32).view(torch.int32))


def still_the_nan_fill(t):
    """every float of t holds the bits nan_buffer / torch.full wrote"""
    return bool((bits(t) == NAN_BITS).all())


def outside(ld, lo, hi):
    """the channels of an ld-wide buffer outside lo .. hi"""
    m = torch.ones(ld, dtype=torch.bool)
    m[lo:hi] = False
    return m.cuda()


def check(kernel, cid, got, ref64, ref32, sliced):
    within(kernel, cid, got, ref64, ref32)
    if sliced:
        for k in range(min(R.GROUPS, got.shape[-1])):
            within(kernel, "%s/ch%d" % (cid, k), got[..., k::R.GROUPS], ref64[..., k::R.GROUPS], ref32[..., k::R.GROUPS])


# ---------------------------------------------------------------------------------------------- bilinear forward
@functools.lru_cache(maxsize=None)
def fwd_data(case):
    _, B, H, W, C, Ho, Wo, ldx, xoff, ldy, yoff, align = case
    g = R.gen(*case[1:])
    x = R.act((B, H, W, C), g)
    base = R.act((B, Ho, Wo, ldy), g)              # what the destination buffer holds before an accumulating call
    return x, base, R.bilinear_ref(x, Ho, Wo, align, F64), R.bilinear_ref(x, Ho, Wo, align, F32)


@pytest.mark.parametrize("case", R.FWD_CASES, ids=R.fwd_id)
def test_bilinear_forward(ops, case):
    _, B, H, W, C, Ho, Wo, ldx, xoff, ldy, yoff, align = case
    cid, kernel = R.fwd_id(case), R.fwd_route(case)["kernel"]
    sliced = ldx != C or ldy != C
    x, base, ref64, ref32 = fwd_data(case)
    xbuf, xd = nan_buffer((B, H, W, C), ldx, xoff, x)
    xbits = bits(xbuf).clone()
    out_cols = outside(ldy, yoff, yoff + C)
    # overwriting a destination that holds NaN, twice
    ybuf, yd = on_device(torch.full((B, Ho, Wo, ldy), float("nan"), dtype=F32), yoff, C)
    ops.bilinear_fwd(xd, Ho, Wo, align, out=yd)
    check(kernel, cid, yd, ref64, ref32, sliced)
    assert still_the_nan_fill(ybuf[..., out_cols]), "wrote outside its channel slice"
    ybuf2, yd2 = on_device(torch.full((B, Ho, Wo, ldy), float("nan"), dtype=F32), yoff, C)
    ops.bilinear_fwd(xd, Ho, Wo, align, out=yd2)
    assert same_bits(ybuf, ybuf2), "two forward calls differ"
    # accumulating onto a random base
    abuf, ad = on_device(base.clone(), yoff, C)
    ops.bilinear_fwd(xd, Ho, Wo, align, out=ad, accumulate=True)
    bs = base[..., yoff:yoff + C]
    check(kernel, cid + "/acc", ad, bs.double() + ref64, bs + ref32, sliced)
    assert same_bits(abuf[..., out_cols], base.cuda()[..., out_cols]), "accumulating wrote outside its channel slice"
    assert torch.equal(bits(xbuf), xbits), "the source changed"


def _one_per_route(cases, routes):
    return [next(c for c in cases if c[0] == r) for r in routes]


@pytest.mark.parametrize("case", _one_per_route(R.FWD_CASES, R.FWD_ROUTES), ids=R.fwd_id)
def test_bilinear_forward_against_the_weight_matrices(ops, case):
    _, B, H, W, C, Ho, Wo, ldx, xoff, ldy, yoff, align = case
    x, base, ref64, ref32 = fwd_data(case)
    xbuf, xd = nan_buffer((B, H, W, C), ldx, xoff, x)
    ybuf, yd = on_device(torch.full((B, Ho, Wo, ldy), float("nan"), dtype=F32), yoff, C)
    ops.bilinear_fwd(xd, Ho, Wo, align, out=yd)
    within(R.fwd_route(case)["kernel"], R.fwd_id(case) + "/matrix", yd, R.bilinear_matrix_fwd(x, Ho, Wo, align), ref32)


# ---------------------------------------------------------------------------------------------- bilinear backward
@functools.lru_cache(maxsize=None)
def bwd_data(case):
    _, B, H, W, C, Ho, Wo, lddy, align, zero_to, lddx, dxoff = case
    g = R.gen(*case[1:])
    dy = R.act((B, Ho, Wo, C), g)
    base = R.act((B, H, W, lddx), g)
    return dy, base, R.bilinear_bwd_ref(dy, H, W, align, F64), R.bilinear_bwd_ref(dy, H, W, align, F32)


@pytest.mark.parametrize("case", R.BWD_CASES, ids=R.bwd_id)
def test_bilinear_backward(ops, case):
    _, B, H, W, C, Ho, Wo, lddy, align, zero_to, lddx, dxoff = case
    cid = R.bwd_id(case)
    sliced = lddy != C or lddx != C
    dy, base, ref64, ref32 = bwd_data(case)
    dybuf, dyd = nan_buffer((B, Ho, Wo, C), lddy, 0, dy)
    dybits = bits(dybuf).clone()
    untouched = outside(lddx, dxoff, dxoff + max(C, zero_to))
    bs = base[..., dxoff:dxoff + C]

    def run(fill, acc):
        buf, view = on_device(fill, dxoff, C)
        ops.bilinear_bwd(dyd, (B, H, W, C), align, out=view, zero_to=zero_to, accumulate=acc)
        torch.cuda.synchronize()
        return buf, view

    over, accd = {}, {}
    try:
        for fused in (1, 0):
            ops.lib.catseg_debug_set_bilinear_bwd_fused(fused)
            kernel = R.bwd_route(case, fused)["kernel"]
            # overwriting a destination that holds NaN, twice
            buf, view = run(torch.full((B, H, W, lddx), float("nan"), dtype=F32), False)
            check(kernel, cid, view, ref64, ref32, sliced)
            if zero_to > C:
                assert bool((buf[..., dxoff + C:dxoff + zero_to] == 0).all()), "columns C .. zero_to are not zero (fused=%d)" % fused
            assert still_the_nan_fill(buf[..., untouched]), "wrote beyond max(C, zero_to) or in front of its slice (fused=%d)" % fused
            assert same_bits(buf, run(torch.full((B, H, W, lddx), float("nan"), dtype=F32), False)[0]), "two calls differ (fused=%d)" % fused
            over[fused] = buf
            # accumulating onto a random base
            buf, view = run(base.clone(), True)
            check(kernel, cid + "/acc", view, bs.double() + ref64, bs + ref32, sliced)
            assert same_bits(buf[..., untouched], base.cuda()[..., untouched]), "accumulating wrote outside its columns (fused=%d)" % fused
            accd[fused] = buf
    finally:
        ops.lib.catseg_debug_set_bilinear_bwd_fused(1)
    assert same_bits(over[1], over[0]), "the default route and the two passes differ"
    assert same_bits(accd[1], accd[0]), "the default route and the two passes differ when accumulating"
    assert torch.equal(bits(dybuf), dybits), "the source changed"


@pytest.mark.parametrize("case", R.BWD_CASES, ids=R.bwd_id)
def test_bilinear_backward_is_the_adjoint_of_the_forward(ops, case):
    """<bilinear_fwd(x), dy> == <x, bilinear_bwd(dy)>, both sums in float64 over the kernels' float32 outputs.  The forward rounds a few
    times per output, the backward once per tap it adds: the two sides differ by at most (taps + 2) 2^-23 sum |x| bwd(|dy|), with taps the
    largest number of output pixels that feed one input pixel and bwd(|dy|) from the float64 weight matrices."""
    _, B, H, W, C, Ho, Wo, lddy, align, zero_to, lddx, dxoff = case
    dy = bwd_data(case)[0]
    x = R.act((B, H, W, C), R.gen(7, *case[1:]))
    y = ops.bilinear_fwd(x.cuda(), Ho, Wo, align)
    dyd = nan_buffer((B, Ho, Wo, C), lddy, 0, dy)[1]
    dx = ops.bilinear_bwd(dyd, (B, H, W, C), align)
    lhs = (y.cpu().double() * dy.double()).sum().item()
    rhs = (x.double() * dx.cpu().double()).sum().item()
    taps = R.bilinear_taps(H, W, Ho, Wo, align)
    bound = (taps + 2) * EPS32 * (x.double().abs() * R.bilinear_matrix_bwd(dy.abs(), H, W, align)).sum().item()
    print("ADJOINT %-60s |lhs - rhs| %.3e  bound %.3e  taps %d  ratio %.3f" % (R.bwd_id(case), abs(lhs - rhs), bound, taps, abs(lhs - rhs) / bound))
    assert abs(lhs - rhs) <= bound, (lhs, rhs, bound)


# ---------------------------------------------------------------------------------------------- adaptive average pooling
@pytest.mark.parametrize("case", R.POOL_CASES, ids=R.pool_id)
def test_adaptive_avgpool(ops, case):
    _, B, S, H, W, C, ldx, xoff, lddx, dxoff = case
    cid = R.pool_id(case)
    g = R.gen(*case[1:])
    x, dy, base = R.act((B, H, W, C), g), R.act((B, S, S, C), g), R.act((B, H, W, lddx), g)
    # forward, out of a channel slice
    xbuf, xd = nan_buffer((B, H, W, C), ldx, xoff, x)
    xbits = bits(xbuf).clone()
    y = ops.adaptive_avgpool_fwd(xd, S)
    assert tuple(y.shape) == (B, S, S, C)
    check("adaptive_avgpool_fwd", cid, y, R.adaptive_avgpool_ref(x, S, F64), R.adaptive_avgpool_ref(x, S, F32), ldx != C)
    assert same_bits(ops.adaptive_avgpool_fwd(xd, S), y), "two forward calls differ"
    assert torch.equal(bits(xbuf), xbits), "the source changed"
    # backward into a channel slice: overwriting NaN, then accumulating onto a random base
    ref64, ref32 = R.adaptive_avgpool_bwd_ref(dy, H, W, F64), R.adaptive_avgpool_bwd_ref(dy, H, W, F32)
    dyd = dy.cuda()
    untouched = outside(lddx, dxoff, dxoff + C)
    bs = base[..., dxoff:dxoff + C]
    buf, view = on_device(torch.full((B, H, W, lddx), float("nan"), dtype=F32), dxoff, C)
    ops.adaptive_avgpool_bwd(dyd, view, S, False)
    check("adaptive_avgpool_bwd", cid, view, ref64, ref32, lddx != C)
    assert still_the_nan_fill(buf[..., untouched]), "wrote outside its channel slice"
    buf2, view2 = on_device(torch.full((B, H, W, lddx), float("nan"), dtype=F32), dxoff, C)
    ops.adaptive_avgpool_bwd(dyd, view2, S, False)
    assert same_bits(buf, buf2), "two backward calls differ"
    abuf, aview = on_device(base.clone(), dxoff, C)
    ops.adaptive_avgpool_bwd(dyd, aview, S, True)
    check("adaptive_avgpool_bwd", cid + "/acc", aview, bs.double() + ref64, bs + ref32, lddx != C)
    assert same_bits(abuf[..., untouched], base.cuda()[..., untouched]), "accumulating wrote outside its channel slice"
