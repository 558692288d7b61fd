"""The CATSEG_OPERANDS_F32 convolutions (csrc/igemm.hip, csrc/wgrad_direct.hip) compared WITHOUT a tolerance, in all three directions, on the
planner's choice and on every tile form launch_igemm instantiates.

tests/_conv_ref.py builds integer operands whose products and partial sums are exact in fp32 in any order, so the result equals the float64
convolution bit for bit on every form, with or without a K split; it lays the buffers out by the operand contract of the F32 convolutions
in include/catseg.h (NaN wherever the contract promises that nothing is read into the result, a NaN payload of its own in every float of a
destination the launch must leave alone).  What this finds is indexing: a wrong border pixel, a dropped row of a partial tile, a tap from
the neighbouring image, a pad column read into the result, an unwritten zero column.  It says nothing about rounding or summation order:
test_kernels_gpu.py and test_w48_gpu.py keep that job.

Every call goes through ops.conv_fwd / conv_fwd_fused / conv_bwd_data / conv_bwd_weight with ops.PRECISION = "fp32"; every test asserts
from ops.PROFILE that only the fp32 kinds ran.  test_planned_* runs every geometry on the planner's tile, test_forms_* forces each of the
14 + 10 + 10 forms (catseg_debug_set_tile, confirmed by catseg_debug_plan_conv) on the three cases test_conv_exact_cpu.py proved to exist for
it, on the tiny-image geometries, on EVERY strided backward-data geometry and on what takes the generic gather (49 taps, the stem), whose
arithmetic is per form, and on the forced split counts.  No mismatch was found on any form: the kernels are unchanged.

GPU time on an MI355X, both measured: this file alone 2.6 s for its 190 items (pytest's total; the slowest item 0.83 s); the rest of the
GPU suite, which is the parent commit's suite, 586 s for its 2142 items in a run of its own."""
import contextlib
import ctypes
import os
import sys

import pytest
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _conv_ref as CR  # noqa: E402
import test_gemm_gpu as TG  # noqa: E402  (FORMS / NO_FORMS: the forms CS_FORM instantiates per layout, and tiles it does not)

pytestmark = pytest.mark.gpu

EINVAL = 1
KINDS = {CR.FWD: "fwd", CR.DGRAD: "dgrad", CR.WGRAD: "wgrad"}


def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")


@contextlib.contextmanager
def _fp32(*directions):
    """ops with PRECISION = "fp32" and a PROFILE list; on the way out: the kinds that ran are those of the fp32 kernels of `directions`"""
    from miccai2021_cataract_semantic_segmentation_amd import ops
    saved = (ops.PRECISION, ops.PROFILE)
    ops.PRECISION, ops.PROFILE = "fp32", []
    try:
        yield ops
        ran = {rec[0] for rec in ops.PROFILE}
    finally:
        ops.PRECISION, ops.PROFILE = saved
        lib = ops.lib                       # whatever a test forced is gone, also after a failure
        lib.catseg_debug_set_tile(0, 0)
        lib.catseg_debug_set_splits(0)
        lib.catseg_debug_set_strided_multi(1)
        lib.catseg_debug_set_wgrad_direct(512)      # on, with the default block target
    assert ran == {KINDS[d] for d in directions}, ran


@contextlib.contextmanager
def _knobs(ops, tile=None, splits=0, multi=1, direct=None):
    lib = ops.lib
    try:
        if tile is not None:
            lib.catseg_debug_set_tile(tile[1] + 16 * tile[0], tile[2])
        lib.catseg_debug_set_splits(splits)
        lib.catseg_debug_set_strided_multi(multi)
        if direct is not None:
            lib.catseg_debug_set_wgrad_direct(direct)
        yield
    finally:
        lib.catseg_debug_set_tile(0, 0)
        lib.catseg_debug_set_splits(0)
        lib.catseg_debug_set_strided_multi(1)
        lib.catseg_debug_set_wgrad_direct(512)


def _planned(ops, g, direction):
    """(mi, ni, form, splits, direct) catseg_debug_plan_conv reports for the geometry under the knobs in force"""
    ldx, ldy = (4, CR.roundup4(g.Cout) + 8) if g.stem else (CR.roundup4(g.Cin) + 8, g.ldy or CR.roundup4(g.Cout) + 8)
    d = ops.make_desc((g.B, g.H, g.W, 4 if g.stem else g.Cin), ldx, g.Cout, ldy, g.k, g.k, g.stride, g.pad, g.dil, g.stem, g.groups)
    out = (ctypes.c_int * 5)()
    ops.check(ops.lib.catseg_debug_plan_conv(ctypes.byref(d), CR.DIRECTIONS.index(direction), out))
    return tuple(out)


_DEVICE = {}


def _device(ops, direction, g):
    """the operands of a problem on the GPU as views of their flat buffers, built once and left unchanged"""
    key = (direction, g)
    if key not in _DEVICE:
        p = CR.PROBLEM[direction](g)
        if direction == CR.FWD:
            if g.stem:
                x = ops.nchw3_to_nhwc4(CR.nchw(p.x).contiguous().cuda())
                w = ops.stem_pack_weight(p.w.cuda().contiguous(memory_format=torch.channels_last), g.Cout)
            else:
                x, w = CR.view(p.X.cuda(), p.xs), CR.view(p.W.cuda(), p.ws)
            _DEVICE[key] = (p, x, w, CR.view(p.Bias.cuda(), p.bs), CR.view(p.Res.cuda(), p.rs))
        elif direction == CR.DGRAD:
            _DEVICE[key] = (p, CR.view(p.DY.cuda(), p.dys), CR.view(p.W.cuda(), p.ws))
        else:
            x = ops.nchw3_to_nhwc4(CR.nchw(p.x).contiguous().cuda()) if g.stem else CR.view(p.X.cuda(), p.xs)
            _DEVICE[key] = (p, x, CR.view(p.DY.cuda(), p.dys))
    return _DEVICE[key]


def _launch_fwd(ops, g, variant, keep):
    """no bias; bias and zero_to; bias, residual and relu through conv_fwd_fused: y is a slice of a wider buffer of payload NaNs.
    keep: receives (buffer before, buffer on the GPU) of every destination BEFORE the launch (a refused launch is examined through it)"""
    p, x, w, bias, res = _device(ops, CR.FWD, g)
    conv = (g.Cout, g.k, g.k, g.stride, g.pad, g.dil)
    before = CR.dest(p.ys)
    yd = before.cuda()
    keep.append((before, yd))
    out, zt = CR.view(yd, p.ys), CR.fwd_zero_to(g, variant)
    if variant == "fused":
        ops.conv_fwd_fused(x, w, bias, res if g.groups == 1 else None, True, *conv, out=out, stem4=g.stem, groups=g.groups)
    else:
        ops.conv_fwd(x, w, None if variant == "plain" else bias, *conv, out=out, zero_to=zt, stem4=g.stem, groups=g.groups)
    return p, zt


def _run_fwd(ops, g, what):
    for variant in CR.FWD_VARIANTS:
        keep = []
        p, zt = _launch_fwd(ops, g, variant, keep)
        CR.check_dest(p.ys, keep[0][0], keep[0][1].cpu(), CR.fwd_want(p, variant), zt, "forward %s %s %s" % (CR.geo_id(g), variant, what))


def _launch_dgrad(ops, g, accumulate, keep):
    p, dy, w = _device(ops, CR.DGRAD, g)
    before = CR.dest(p.dxs, p.dx0 if accumulate else None)
    dxd = before.cuda()
    keep.append((before, dxd))
    ops.conv_bwd_data(dy, w, (g.B, g.H, g.W, g.Cin), g.k, g.k, g.stride, g.pad, g.dil, out=CR.view(dxd, p.dxs), accumulate=accumulate, groups=g.groups)
    return p


def _run_dgrad(ops, g, what):
    """into payload NaNs, then accumulating onto integers"""
    for accumulate in (False, True):
        keep = []
        p = _launch_dgrad(ops, g, accumulate, keep)
        want = p.ref + p.dx0.double() if accumulate else p.ref
        CR.check_dest(p.dxs, keep[0][0], keep[0][1].cpu(), want, 0, "backward-data %s %s%s" % (CR.geo_id(g), what, " accumulate" if accumulate else ""),
                      plus_zero=None if accumulate else p.untapped)


def _launch_wgrad(ops, g, keep):
    p, x, dy = _device(ops, CR.WGRAD, g)
    bw, bb = CR.dest(p.dws), CR.dest(p.dbs, salt=78)
    dwd, dbd = bw.cuda(), bb.cuda()
    keep += [(bw, dwd), (bb, dbd)]
    dw, db = CR.view(dwd, p.dws), CR.view(dbd, p.dbs)
    if g.stem:
        dpk = torch.full((g.Cout, 7, 8, 4), float("nan"), device="cuda")
        ops.conv_bwd_weight(x, dy, dpk, db, g.k, g.k, g.stride, g.pad, g.dil, stem4=True)
        ops.stem_unpack_grad(dpk, dw, g.Cout)
    else:
        ops.conv_bwd_weight(x, dy, dw, db, g.k, g.k, g.stride, g.pad, g.dil, groups=g.groups)
    return p


def _run_wgrad(ops, g, what):
    """dw and dbias into payload NaNs"""
    keep = []
    p = _launch_wgrad(ops, g, keep)
    (bw, dwd), (bb, dbd) = keep
    dw = dwd.cpu()
    CR.check_dest(p.dws, bw, dw, p.ref, 0, "backward-weight %s %s" % (CR.geo_id(g), what))
    CR.check_dest(p.dbs, bb, dbd.cpu(), p.dbias, 0, "dbias %s %s" % (CR.geo_id(g), what))
    return dw


def _ids(direction):
    return [CR.geo_id(g) for g in CR.CASES[direction]]


# ---------------------------------------------------------------------------------------------------------------------------------
# (a) every geometry on the tile the planner picks

@pytest.mark.parametrize("g", CR.CASES[CR.FWD], ids=_ids(CR.FWD))
def test_planned_forward(g):
    _need_gpu()
    with _fp32(CR.FWD) as ops:
        _run_fwd(ops, g, "planned")


@pytest.mark.parametrize("g", CR.CASES[CR.DGRAD], ids=_ids(CR.DGRAD))
def test_planned_backward_data(g):
    """stride 2: the parity classes as one launch (catseg_debug_set_strided_multi 1) and as one launch each (0)"""
    _need_gpu()
    with _fp32(CR.DGRAD) as ops:
        for multi in ((1, 0) if g.stride == 2 else (1,)):
            with _knobs(ops, multi=multi):
                _run_dgrad(ops, g, "planned, multi %d" % multi)


@pytest.mark.parametrize("g", CR.CASES[CR.WGRAD], ids=_ids(CR.WGRAD))
def test_planned_backward_weight(g):
    _need_gpu()
    with _fp32(CR.WGRAD) as ops:
        assert _planned(ops, g, CR.WGRAD)[4] == (1 if g in CR.DIRECT else 0)
        _run_wgrad(ops, g, "planned")


@pytest.mark.parametrize("g", CR.DIRECT, ids=[CR.geo_id(g) for g in CR.DIRECT])
def test_direct_backward_weight_equals_the_gemm(g):
    """csrc/wgrad_direct.hip on (catseg_debug_set_wgrad_direct 1) and off (0): both equal the reference, and so each other"""
    _need_gpu()
    with _fp32(CR.WGRAD) as ops:
        got = {}
        for direct in (1, 0):
            with _knobs(ops, direct=direct):
                assert _planned(ops, g, CR.WGRAD)[4] == direct
                got[direct] = _run_wgrad(ops, g, "direct %d" % direct)
        assert torch.equal(CR.bits(got[1]), CR.bits(got[0]))


@pytest.mark.parametrize("splits", CR.SPLITS)
def test_backward_weight_forced_splits(splits):
    """1040 rows on the planner's tile: a short last split, a split count that rounding rows-per-split up to 16 changes, 65 slabs through
    reduce_slabs_wide_kernel"""
    _need_gpu()
    g = CR.SPLIT_GEO
    with _fp32(CR.WGRAD) as ops:
        with _knobs(ops, splits=splits):
            assert _planned(ops, g, CR.WGRAD)[3] == CR.split_plan(CR.rows_out(g), splits)[1]
            _run_wgrad(ops, g, "splits %d" % splits)


# ---------------------------------------------------------------------------------------------------------------------------------
# (b) every tile form of the direction's layout, forced

def _form_params(direction):
    return [pytest.param(f, mi, ni, id="form%d_%dx%d" % (f, mi, ni)) for f, mi, ni in TG.FORMS[CR.LAYOUT[direction]]]


def _forced(ops, g, direction, form, mi, ni):
    assert _planned(ops, g, direction)[:3] == (mi, ni, form), (CR.geo_id(g), _planned(ops, g, direction))
    return "form %d tile %d x %d" % (form, mi, ni)


@pytest.mark.parametrize("form,mi,ni", _form_params(CR.FWD))
def test_forms_forward(form, mi, ni):
    """the form's three cases (inside one tile, a row and a column past it, whole tiles only), the images smaller than one K step, and
    what takes the generic gather (49 taps, the stem): the FAST = false instantiation of every form runs too"""
    _need_gpu()
    with _fp32(CR.FWD) as ops:
        for g in CR.form_geos(CR.FWD, *TG._tile(form, mi, ni)) + tuple(CR.TINY_FWD) + tuple(CR.GENERIC[CR.FWD]):
            with _knobs(ops, tile=(form, mi, ni)):
                _run_fwd(ops, g, _forced(ops, g, CR.FWD, form, mi, ni))


@pytest.mark.parametrize("form,mi,ni", _form_params(CR.DGRAD))
def test_forms_backward_data(form, mi, ni):
    """the form's three cases, EVERY strided geometry (stride 2: the parity classes in one launch and in one launch each; stride 3 and 8:
    one launch per class; 49 taps per class: the generic path) and the 49-tap stride-1 case of the generic gather"""
    _need_gpu()
    with _fp32(CR.DGRAD) as ops:
        for g in CR.form_geos(CR.DGRAD, *TG._tile(form, mi, ni)) + tuple(CR.STRIDED_DGRAD) + tuple(CR.GENERIC[CR.DGRAD]):
            for multi in ((1, 0) if g.stride == 2 else (1,)):
                with _knobs(ops, tile=(form, mi, ni), multi=multi):
                    _run_dgrad(ops, g, _forced(ops, g, CR.DGRAD, form, mi, ni) + ", multi %d" % multi)


@pytest.mark.parametrize("form,mi,ni", _form_params(CR.WGRAD))
def test_forms_backward_weight(form, mi, ni):
    """the form's three cases, the tiny images (the incremental row stepping is per form), 49 taps and the stem (the generic gather, one
    launch row per filter row) and the forced split counts at 1040 rows"""
    _need_gpu()
    with _fp32(CR.WGRAD) as ops:
        for g in CR.form_geos(CR.WGRAD, *TG._tile(form, mi, ni)) + tuple(CR.TINY_WGRAD) + tuple(CR.GENERIC[CR.WGRAD]):
            with _knobs(ops, tile=(form, mi, ni)):
                _run_wgrad(ops, g, _forced(ops, g, CR.WGRAD, form, mi, ni))
        g = CR.SPLIT_GEO
        for splits in CR.SPLITS:
            with _knobs(ops, tile=(form, mi, ni), splits=splits):
                assert _planned(ops, g, CR.WGRAD)[3] == CR.split_plan(CR.rows_out(g), splits)[1]
                _run_wgrad(ops, g, _forced(ops, g, CR.WGRAD, form, mi, ni) + ", splits %d" % splits)


@pytest.mark.parametrize("direction,form,mi,ni", [(d, f, mi, ni) for d in CR.DIRECTIONS for f, mi, ni in TG.NO_FORMS[CR.LAYOUT[d]]])
def test_forms_missing_are_refused(direction, form, mi, ni):
    """a tile form the layout does not have, on a convolution: CATSEG_EINVAL with a message, the destination's bits untouched (backward-data
    also at stride 2, where the classes go out as one launch or as one each)"""
    _need_gpu()
    cases = [(CR.form_geos(direction, 64, 64)[1], 1)] + ([(CR.STRIDED_DGRAD[0], 1), (CR.STRIDED_DGRAD[0], 0)] if direction == CR.DGRAD else [])
    launch = {CR.FWD: lambda ops, g, keep: _launch_fwd(ops, g, "bias_zero", keep), CR.DGRAD: lambda ops, g, keep: _launch_dgrad(ops, g, False, keep),
              CR.WGRAD: _launch_wgrad}[direction]
    with _fp32(direction) as ops:
        for g, multi in cases:
            keep = []
            with _knobs(ops, tile=(form, mi, ni), multi=multi):
                with pytest.raises(RuntimeError, match=r"error %d: .*unsupported tile" % EINVAL):
                    launch(ops, g, keep)
            torch.cuda.synchronize()
            assert keep
            for before, dst in keep:
                assert torch.equal(CR.bits(dst.cpu()), CR.bits(before))
            {CR.FWD: _run_fwd, CR.DGRAD: _run_dgrad, CR.WGRAD: _run_wgrad}[direction](ops, g, "after the refusal")      # (the forced tile is gone again)


# ---------------------------------------------------------------------------------------------------------------------------------
# (c) the fused BatchNorm statistics on every forward form that has them (forms 0 and 1): the inputs, references and bounds of
# test_kernels_gpu.test_conv_epilogue_bn_statistics, only the forced tile is new.  That test's body cannot be called with a forced tile and
# a second launch in it, so its lines are RESTATED in _bn_case and below; test_conv_exact_cpu.py compares them with that function's source,
# line by line, so that a change there cannot leave this copy behind unnoticed.

_BN = {}


def _bn_case(case):
    if case not in _BN:
        import test_kernels_gpu as TK
        B, H, W, Cin, Cout, k, s, p = case
        g = torch.Generator().manual_seed(sum(case))
        x = torch.randn(B, Cin, H, W, generator=g) + 0.5
        w = torch.randn(Cout, Cin, k, k, generator=g) * (2.0 / (Cin * k * k)) ** 0.5
        b = torch.randn(Cout, generator=g) * 3
        y64 = F.conv2d(x.double(), w.double(), b.double(), s, p).permute(0, 2, 3, 1).reshape(-1, Cout)
        gamma = (1 + 0.1 * torch.randn(Cout, generator=g)).cuda()
        _BN[case] = (TK.nhwc(x), TK.ohwi(w), b.cuda(), gamma, y64.shape[0], y64.mean(0), y64.var(0, unbiased=False))
    return _BN[case]


def _bn_forms():
    return [pytest.param(f, mi, ni, id="form%d_%dx%d" % (f, mi, ni)) for f, mi, ni in TG.FORMS[CR.LAYOUT[CR.FWD]] if f in (0, 1)]


@pytest.mark.parametrize("form,mi,ni", _bn_forms())
def test_fused_statistics_on_forced_forms(form, mi, ni):
    _need_gpu()
    import test_kernels_gpu as TK
    close = TK.close
    for case in TK.BNSTAT_CASES:
        B, H, W, Cin, Cout, k, s, p = case
        xd, wd, bd, gamma, n, mean64, var64 = _bn_case(case)
        with _fp32(CR.FWD) as ops:
            with _knobs(ops, tile=(form, mi, ni)):
                y, partials = ops.conv_fwd(xd, wd, bd, Cout, k, k, s, p, 1, bn_stats=True)
                plain = ops.conv_fwd(xd, wd, bd, Cout, k, k, s, p, 1)
        assert partials is not None, "form %d (%d, %d) has fused statistics" % (form, mi, ni)
        assert torch.equal(CR.bits(y.cpu()), CR.bits(plain.cpu())), "y with bn_stats differs from y without"
        rm, rv = torch.zeros(Cout, device="cuda"), torch.ones(Cout, device="cuda")
        stats, scale = ops.bn_finalize(partials, n, Cout, gamma, 1e-5, 0.1, rm, rv)
        close(stats[:Cout], mean64, atol=1e-6, rtol=2e-6)
        close(stats[Cout:], 1.0 / torch.sqrt(var64 + 1e-5), atol=0, rtol=2e-5)
        close(scale, gamma.cpu().double() / torch.sqrt(var64 + 1e-5), atol=0, rtol=2e-5)
        close(rm, 0.1 * mean64, atol=1e-6, rtol=1e-5)
        close(rv, 0.9 + 0.1 * var64 * n / max(n - 1, 1), atol=0, rtol=2e-5)
        rm2, rv2 = torch.zeros(Cout, device="cuda"), torch.ones(Cout, device="cuda")
        stats2, _ = ops.bn_train_stats(y, gamma, 1e-5, 0.1, rm2, rv2)
        close(stats, stats2.cpu(), atol=1e-6, rtol=1e-5)


# ---------------------------------------------------------------------------------------------------------------------------------
# (d) the transposed convolution of the FCN head, which runs forward as a backward-data and backward as a backward-weight and a forward

def test_transposed_convolution_exact():
    """models/FCN.py's ConvTranspose2d(k 16, stride 8, pad 4) in miniature (a 3 x 2 map of 25 classes in rows of 32 floats) through
    ops.conv_transpose_fwd / conv_transpose_bwd against F.conv_transpose2d and its autograd in float64.  The input's pad columns [25, 28)
    are zero as the contract of backward-data demands, [28, 32) are NaN: never read."""
    _need_gpu()
    B, H, W, Ci, Co, k, s, p, ld = 1, 3, 2, 25, 25, 16, 8, 4, 32
    gen = torch.Generator().manual_seed(16)
    room = CR.LIMIT - 1 - CR.EXTRA
    amax, bmax = CR.magnitudes(((k + s - 1) // s) ** 2 * Ci)        # an output pixel is reached by 2 x 2 taps of Cin channels
    gmax = min(room // (k * k * Co * bmax), room // (B * H * W * amax))     # dx sums k k Cout products, dw B H W
    x, w, bias = CR.ints(gen, amax, (B, H, W, Ci)), CR.ints(gen, bmax, (Ci, Co, k, k)), CR.ints(gen, CR.C0_MAX, (Co,))
    x64, w64, b64 = (t.double().requires_grad_() for t in (CR.nchw(x), w, bias))
    y64 = F.conv_transpose2d(x64, w64, b64, s, p)
    Ho, Wo = y64.shape[2:]
    assert (Ho, Wo) == (24, 16) and float(F.conv_transpose2d(CR.nchw(x).abs(), w.abs(), None, s, p).max()) + CR.C0_MAX < 2 ** 23
    gy, dx0 = CR.ints(gen, gmax, (B, Ho, Wo, Co)), CR.ints(gen, CR.C0_MAX, (B, H, W, Ci))
    y64.backward(CR.nchw(gy).double())
    assert gmax >= 16 and max(float(t.abs().max()) for t in (x64.grad, w64.grad, b64.grad)) + CR.C0_MAX < 2 ** 23
    xs = CR.act_slot(B, H, W, Ci, width=28, ld=ld)
    with _fp32(CR.DGRAD, CR.WGRAD, CR.FWD) as ops:
        xd = CR.view(CR.filled(xs, x, zero=(Ci, 28)).cuda(), xs)
        wd = w.cuda().contiguous(memory_format=torch.channels_last)
        y, wp = ops.conv_transpose_fwd(xd, wd, bias.cuda(), Co, k, s, p, ld=ld)
        assert ops.ld_of(y) == ld and torch.equal(y.cpu().double(), CR.nhwc(y64.detach()))
        assert not bool(ops.widen(y)[..., Co:].contiguous().view(torch.int32).any())
        gyd = ops.new_act(B, Ho, Wo, Co, xd.device, ld=ld, zero=True)
        gyd.copy_(gy.cuda())
        for accumulate in (False, True):
            dw, db = torch.full_like(wd, float("nan")), torch.full((Co,), float("nan"), device="cuda")
            dx = ops.new_act(B, H, W, Ci, xd.device, ld=ld, zero=True)
            if accumulate:
                dx.copy_(dx0.cuda())
            ops.conv_transpose_bwd(gyd, xd, wp, dw, db, k, s, p, dx, accumulate, ld=ld)
            assert torch.equal(dw.cpu().double(), w64.grad) and torch.equal(db.cpu().double(), b64.grad)
            assert torch.equal(dx.cpu().double(), CR.nhwc(x64.grad) + (dx0.double() if accumulate else 0.0))
            assert not bool(ops.widen(dx)[..., Ci:].contiguous().view(torch.int32).any())
