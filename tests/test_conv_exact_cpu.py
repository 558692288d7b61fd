"""tests/_conv_ref.py against its own preconditions, without a GPU: the integer operands really make fp32 exact in every direction, the
references equal a plain nested-loop float64 convolution, the case list contains for EVERY tile form of every layout a case inside one tile,
one a row and a column past it and one of whole tiles only (computed from the lists and the tile expression of tests/test_gemm_gpu.py, not
claimed in a comment), every float outside the logical operands is NaN except the pads the contract in include/catseg.h wants zero, and
the checker the GPU tests rely on accepts a convolution written by the rules of the contract and flags the mistakes it is there to find."""
import os
import sys

import pytest
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _conv_ref as CR  # noqa: E402
import _gemm_ref as GR  # noqa: E402

ALL = [(d, g) for d in CR.DIRECTIONS for g in CR.CASES[d]]
IDS = ["%s-%s" % (d, CR.geo_id(g)) for d, g in ALL]


@pytest.mark.parametrize("direction,g", ALL, ids=IDS)
def test_operands_are_exact_in_fp32(direction, g):
    p = CR.PROBLEM[direction](g)
    K = CR.reduction(direction, g)
    a, b = {CR.FWD: lambda: (p.x, p.w), CR.DGRAD: lambda: (p.dy, p.w), CR.WGRAD: lambda: (p.dy, p.x)}[direction]()
    assert float(a.abs().max()) == p.amax and float(b.abs().max()) == p.bmax
    assert K * p.amax * p.bmax + CR.EXTRA < 2 ** 23 and CR.EXTRA == 3 * CR.C0_MAX
    if K <= 256:
        assert p.amax >= 2 ** 12 and p.amax % 2 == 1          # not an fp16 / tf32 / bf16 number
        assert float(a.half().float().sub(a).abs().max()) > 0 and float(a.bfloat16().float().sub(a).abs().max()) > 0
    for t in (a, b):
        assert torch.equal(t, t.round())
    assert p.ref.dtype == torch.float64 and torch.equal(p.ref, p.ref.round())
    # the bound is on the sum of |products|: every partial sum of every order stays below it
    s, pd, dl, gr = g.stride, g.pad, g.dil, g.groups
    if direction == CR.FWD:
        bound = F.conv2d(CR.nchw(p.x).abs(), p.w.abs(), None, s, pd, dl, gr)
        other = CR.nhwc(F.conv2d(CR.nchw(p.x), p.w, None, s, pd, dl, gr))
        extra = float(p.bias.abs().max() + p.res.abs().max())
    elif direction == CR.DGRAD:
        bound = torch.nn.grad.conv2d_input((g.B, g.Cin, g.H, g.W), p.w.abs(), CR.nchw(p.dy).abs(), s, pd, dl, gr)
        other = CR.nhwc(torch.nn.grad.conv2d_input((g.B, g.Cin, g.H, g.W), p.w, CR.nchw(p.dy), s, pd, dl, gr))
        extra = float(p.dx0.abs().max())
    else:
        bound = torch.nn.grad.conv2d_weight(CR.nchw(p.x).abs(), tuple(p.ref.shape), CR.nchw(p.dy).abs(), s, pd, dl, gr)
        other = torch.nn.grad.conv2d_weight(CR.nchw(p.x), tuple(p.ref.shape), CR.nchw(p.dy), s, pd, dl, gr)
        extra = 0.0
        assert float(p.dy.abs().sum((0, 1, 2)).max()) < 2 ** 23 and torch.equal(p.dbias.float().double(), p.dbias)
    assert float(bound.max()) + extra < 2 ** 23 and extra <= CR.EXTRA
    # the same convolution in float32, in whatever order the CPU library sums: the same bits (the property the GPU test stands on)
    assert other.dtype == torch.float32 and torch.equal(other.double(), p.ref)


def _loops(g):
    Ho, Wo = CR.out_hw(g)
    for b in range(g.B):
        for oy in range(Ho):
            for ox in range(Wo):
                for ky in range(g.k):
                    for kx in range(g.k):
                        iy, ix = oy * g.stride - g.pad + ky * g.dil, ox * g.stride - g.pad + kx * g.dil
                        if 0 <= iy < g.H and 0 <= ix < g.W:
                            for gr in range(g.groups):
                                cog, cig = g.Cout // g.groups, g.Cin // g.groups
                                yield b, oy, ox, ky, kx, iy, ix, slice(gr * cog, (gr + 1) * cog), slice(gr * cig, (gr + 1) * cig)


def _loop_fwd(g, x, w):
    Ho, Wo = CR.out_hw(g)
    y = torch.zeros(g.B, Ho, Wo, g.Cout, dtype=torch.float64)
    for b, oy, ox, ky, kx, iy, ix, co, ci in _loops(g):
        y[b, oy, ox, co] += w[co, :, ky, kx] @ x[b, iy, ix, ci]
    return y


def _loop_dgrad(g, dy, w):
    dx = torch.zeros(g.B, g.H, g.W, g.Cin, dtype=torch.float64)
    for b, oy, ox, ky, kx, iy, ix, co, ci in _loops(g):
        dx[b, iy, ix, ci] += w[co, :, ky, kx].t() @ dy[b, oy, ox, co]
    return dx


def _loop_wgrad(g, x, dy):
    dw = torch.zeros(g.Cout, g.Cin // g.groups, g.k, g.k, dtype=torch.float64)
    for b, oy, ox, ky, kx, iy, ix, co, ci in _loops(g):
        dw[co, :, ky, kx] += torch.outer(dy[b, oy, ox, co], x[b, iy, ix, ci])
    return dw


def _smallest(direction, n=2):
    return sorted(CR.NAMED[direction], key=lambda g: CR.rows_out(g) * g.k * g.k * g.groups)[:n]


def test_references_equal_a_nested_loop_convolution():
    """the two smallest cases of every direction, and the smallest grouped, strided and dilated ones"""
    def least(direction, cond):
        return [min((g for g in CR.NAMED[direction] if cond(g)), key=CR.rows_out)]
    extra = {CR.FWD: least(CR.FWD, lambda g: g.groups > 1), CR.WGRAD: [],
             CR.DGRAD: least(CR.DGRAD, lambda g: g.stride == 2 and g.dil == 2) + least(CR.DGRAD, lambda g: g.stride == 3 and g.k == 5)}
    for direction in CR.DIRECTIONS:
        for g in _smallest(direction) + extra[direction]:
            p = CR.PROBLEM[direction](g)
            if direction == CR.FWD:
                got = _loop_fwd(g, p.x.double(), p.w.double())
            elif direction == CR.DGRAD:
                got = _loop_dgrad(g, p.dy.double(), p.w.double())
            else:
                got = _loop_wgrad(g, p.x.double(), p.dy.double())
            assert torch.equal(got, p.ref), (direction, g)


def test_every_form_has_its_three_cases():
    """by computation: for every form CS_FORM instantiates for the layout (test_gemm_gpu.FORMS, tile extents from test_gemm_gpu._tile) the case
    list holds a case inside a single tile, one exactly a row and a (legal) column past it, and one of whole tiles only"""
    import test_gemm_gpu as TG
    assert [len(TG.FORMS[lay]) for lay in (GR.NT, GR.NN, GR.TN)] == [14, 10, 10]
    for direction in CR.DIRECTIONS:
        step = 1 if direction == CR.FWD else 4       # Cin, and so taps x Cin, comes in fours
        fs = CR.forms(direction)
        assert [f[:3] for f in fs] == TG.FORMS[CR.LAYOUT[direction]]
        for form, mi, ni, tm, tn in fs:
            assert (tm, tn) == TG._tile(form, mi, ni)
            inside, past, whole = CR.form_geos(direction, tm, tn)
            for g in (inside, past, whole):
                assert g in CR.CASES[direction] and g.groups == 1 and (direction != CR.DGRAD or g.stride == 1)
            M, N = CR.gemm_dims(direction, inside)
            assert 0 < M < tm and 0 < N <= tn and (N < tn or tn == 16)
            M, N = CR.gemm_dims(direction, past)
            assert M == tm + 1 and N == tn + step
            M, N = CR.gemm_dims(direction, whole)
            assert M % tm == 0 and N % tn == 0 and (M // tm) * (N // tn) >= 2
            # the planned forward variant with zero_to visits r4(Cout) + 4 columns: it is the plain variant that has whole tiles only
            assert CR.fwd_zero_to(whole, "plain") == 0


def test_named_edges_are_present():
    fwd, dg, wg = (CR.NAMED[d] for d in CR.DIRECTIONS)
    # forward: Cout one past every tile width, M past 64 / 128 / 192 / 256 and exactly 64, whole tiles on the square and the 48-wide forms
    assert {5, 17, 33, 49, 65, 97, 129, 193} <= {g.Cout for g in fwd}
    assert {20, 30, 80, 198, 63, 437, 64, 256} <= {CR.rows_out(g) for g in fwd}
    assert any(CR.rows_out(g) % 64 == 0 and g.Cout % 256 == 0 for g in fwd) and any(CR.rows_out(g) % 128 == 0 and g.Cout % 96 == 0 for g in fwd)
    assert any(g.k * g.k > 32 and not g.stem for g in fwd) and any(g.stem for g in fwd) and {2, 4} <= {g.groups for g in fwd}
    assert any(g.H * g.W == 1 for g in fwd) and any(1 < g.H * g.W < 16 for g in fwd) and any(g.dil == 12 for g in fwd)
    # backward-data: N = Cin one group of four past 48 ... 192, Cout with pad columns, the parity-class edges
    assert {52, 68, 100, 132, 196} <= {g.Cin for g in dg} and {5, 17, 25} <= {g.Cout for g in dg}
    assert any(g.stride == 2 and g.H < g.stride for g in dg)                                    # a class without rows
    assert any(g.stride == 2 and g.k == 1 for g in dg)                                          # classes without a tap
    assert any(g.stride == 2 and g.dil == 2 for g in dg) and {(3, 3), (3, 5)} <= {(g.stride, g.k) for g in dg}
    assert any((g.k, g.stride, g.pad) == (16, 8, 4) and CR.out_hw(g) == (3, 2) for g in dg)
    assert any(g.stride == 2 and ((g.k + 1) // 2) ** 2 > 32 for g in dg) and any(g.stride == 1 and g.k * g.k > 32 for g in dg)
    # what runs on EVERY form besides its three cases: all strided backward-data geometries (none dropped), and what takes the generic gather
    assert set(CR.STRIDED_DGRAD) == {g for g in dg if g.stride > 1} and len(CR.STRIDED_DGRAD) == 9
    assert {(g.stride, g.k) for g in CR.STRIDED_DGRAD} >= {(2, 13), (3, 3), (3, 5), (8, 16)}
    assert [(g.k, g.stem) for g in CR.GENERIC[CR.FWD]] == [(7, False), (7, True)] and [(g.k, g.stride) for g in CR.GENERIC[CR.DGRAD]] == [(7, 1)]
    assert [(g.k, g.stem) for g in CR.GENERIC[CR.WGRAD]] == [(7, False), (7, True)]
    assert [(g.B, g.H, g.W) for g in CR.TINY_FWD] == [(20, 1, 1), (5, 2, 3), (1, 2, 40)] == [(g.B, g.H, g.W) for g in CR.TINY_WGRAD]
    assert CR.SPLIT_GEO in wg and len(CR.DIRECT) == 2
    # backward-weight: M = Cout, N = taps x Cin, the rows around the 16-row K step, the split edges, both dbias kernels, the direct kernel
    assert {5, 49, 65, 97, 129, 193, 257} <= {g.Cout for g in wg}
    assert {68, 132, 260} <= {CR.gemm_dims(CR.WGRAD, g)[1] for g in wg}
    assert {1, 15, 16, 17, 1040} <= {CR.rows_out(g) for g in wg}
    rows = CR.rows_out(CR.SPLIT_GEO)
    assert rows == 1040 and {1, 2, 3, 7, 65} <= set(CR.SPLITS)
    plans = {s: CR.split_plan(rows, s) for s in CR.SPLITS}
    assert plans == {1: (1040, 1), 2: (528, 2), 3: (352, 3), 7: (160, 7), 12: (96, 11), 65: (16, 65)}
    assert all(rows % rps != 0 for s, (rps, n) in plans.items() if s in (2, 3, 7, 12))           # the last split is short
    assert plans[12][1] != 12                                                                    # rounding rps up to 16 changed the count
    assert plans[65][1] >= 64 and CR.SPLIT_GEO.Cout * CR.SPLIT_GEO.Cin // 4 <= 64 * 1024         # reduce_slabs_wide_kernel's condition
    assert any(g.ldy == 32 and g.Cout <= 32 and CR.rows_out(g) > 1024 for g in wg) and any(g.ldy == 0 and CR.rows_out(g) > 1024 and g.k == 1 for g in wg)
    assert any(g.groups > 1 for g in wg) and any(g.stem for g in wg)
    for g in CR.DIRECT:                                                                          # wgrad_direct.hip: direct_plan
        assert (g.Cin, g.Cout) in ((48, 48), (96, 96)) and (g.k, g.stride, g.pad, g.dil) == (3, 1, 1, 1)
        assert g.B * g.H * ((g.W + 15) // 16) == 1024 and g.W % 16 == 1
    for d, g in ALL:                                                                             # what check_desc requires of a launch
        assert g.stem or (g.Cin // g.groups) % 4 == 0
        assert d == CR.FWD or g.groups == 1 or (g.Cout // g.groups) % 4 == 0
        assert CR.out_hw(g)[0] > 0 and CR.out_hw(g)[1] > 0


@pytest.mark.parametrize("direction,g", ALL, ids=IDS)
def test_buffers_are_nan_outside_the_operands(direction, g):
    p = CR.PROBLEM[direction](g)
    r4 = CR.roundup4(g.Cout)
    if direction == CR.FWD:
        items = [(p.X, p.xs, p.x, None), (p.W, p.ws, p.w, None), (p.Bias, p.bs, p.bias, None), (p.Res, p.rs, p.res, None)]
        dests = [(p.ys, None)]
        assert CR.ld_of(p.ys) >= 4 + CR.fwd_zero_to(g, "bias_zero")
    elif direction == CR.DGRAD:
        items = [(p.DY, p.dys, p.dy, (g.Cout, r4)), (p.W, p.ws, p.w, None)]          # the ONLY zeros: dy's pad columns [Cout, r4(Cout))
        dests = [(p.dxs, None), (p.dxs, p.dx0)]
    else:
        items = [(p.X, p.xs, p.x, None), (p.DY, p.dys, p.dy, None)]                  # dy's pad columns may hold anything: NaN
        dests = [(p.dws, None), (p.dbs, None)]
    for flat, slot, vals, zero in items:
        if flat is None:
            assert g.stem
            continue
        assert flat.numel() == slot.numel and slot.offset % 4 == 0 and (len(slot.shape) != 4 or slot.strides[2] % 4 == 0 or slot.strides[1] == 1)
        assert torch.equal(CR.view(flat, slot), vals)
        known = torch.zeros(flat.numel(), dtype=torch.bool)
        CR.view(known, slot)[...] = True
        if zero is not None and zero[1] > zero[0]:
            assert float(CR.view(flat, slot, zero).abs().max()) == 0
            CR.view(known, slot, zero)[...] = True
        assert bool(torch.isfinite(flat[known]).all()) and bool(torch.isnan(flat[~known]).all())
        assert int((~known).sum()) >= 8                                       # a head and a tail at the least
        if len(slot.shape) == 4 and slot.strides[-1] == 1 and slot.strides[2] > slot.shape[-1]:      # an activation: ld > C
            assert bool(torch.isnan(flat[:slot.offset]).all()) and bool(torch.isnan(flat[-(4 * slot.strides[2] + 12):]).all())
    for slot, initial in dests:
        flat = CR.dest(slot, initial)
        logical = CR.view(flat, slot)
        assert bool(torch.isfinite(logical).all()) == (initial is not None)
        assert int(torch.isnan(flat).sum()) == flat.numel() - (logical.numel() if initial is not None else 0)
        if initial is None:
            assert flat.numel() < 1 << 22 and CR.bits(flat).unique().numel() == flat.numel()        # one payload per NaN


# ---------------------------------------------------------------------------------------------------------------------------------
# the checker is sharp: convolutions that keep the contract pass, deliberately wrong ones are flagged on at least one case

def _flagged(fn):
    try:
        fn()
    except AssertionError:
        return True
    return False


def _emu_fwd(p, variant, conv=None, zeros=True, rows_written=None):
    """a forward launch that keeps the contract, on the CPU; conv: its convolution; zeros: writes [Cout, zero_to); rows_written: mask"""
    g = p.g
    before = CR.dest(p.ys)
    after = before.clone()
    y = CR.fwd_want(p, variant, conv).float()
    dst = CR.view(after, p.ys)
    if rows_written is None:
        dst[...] = y
    else:
        m = rows_written(torch.arange(CR.rows_out(g))).view(y.shape[:3])
        dst[m] = y[m]
    zt = CR.fwd_zero_to(g, variant)
    if zeros and zt:
        CR.view(after, p.ys, (g.Cout, zt))[...] = 0.0
    CR.check_dest(p.ys, before, after, CR.fwd_want(p, variant), zt, "emulated %s" % variant)


def _conv_of(p, pad_extra=0, dil=None):
    """forward convolution on an explicitly padded image: pad_extra moves the tap origin, dil overrides the dilation"""
    g = p.g
    Ho, Wo = CR.out_hw(g)
    xp = F.pad(CR.nchw(p.x).double(), (g.pad + pad_extra,) * 4)
    y = F.conv2d(xp, p.w.double(), None, g.stride, 0, g.dil if dil is None else dil, g.groups)
    return CR.nhwc(y[:, :, :Ho, :Wo])


def _conv_wrapping(p):
    """taps that leave an image at its top or bottom land in the neighbouring image of the batch: the batch as one tall image"""
    g = p.g
    Ho, Wo = CR.out_hw(g)
    if Ho != g.H or g.stride != 1:
        return p.ref
    tall = CR.nchw(p.x).double().permute(1, 0, 2, 3).reshape(1, g.Cin, g.B * g.H, g.W)
    y = F.conv2d(tall, p.w.double(), None, 1, g.pad, g.dil, g.groups)           # [1, Cout, B H, Wo]
    return y.reshape(g.Cout, g.B, g.H, Wo).permute(1, 2, 3, 0)


def test_checker_flags_wrong_forward_convolutions():
    cases = [g for g in CR.NAMED[CR.FWD] if not g.stem]
    wrong = {"pad off by one": [], "dilation ignored": [], "taps wrap into the next image": [], "last row of a 64-row tile dropped": [],
             "[Cout, zero_to) unwritten": []}
    for g in cases:
        p = CR.fwd_problem(g)
        for variant in CR.FWD_VARIANTS:
            _emu_fwd(p, variant)                                    # the contract itself passes, on every case and variant
        wrong["pad off by one"].append(_flagged(lambda: _emu_fwd(p, "plain", _conv_of(p, pad_extra=1))))
        wrong["dilation ignored"].append(_flagged(lambda: _emu_fwd(p, "plain", _conv_of(p, dil=1))))
        wrong["taps wrap into the next image"].append(_flagged(lambda: _emu_fwd(p, "fused", _conv_wrapping(p))))
        wrong["last row of a 64-row tile dropped"].append(_flagged(lambda: _emu_fwd(p, "bias_zero", rows_written=lambda r: r % 64 != 63)))
        wrong["[Cout, zero_to) unwritten"].append(_flagged(lambda: _emu_fwd(p, "bias_zero", zeros=False)))
    for name, hits in wrong.items():
        assert any(hits), name
    # each is found where its edge exists: on every case, with dil > 1, with B > 1 and 'same' extents, with >= 64 rows, with zero_to
    for g, a, b, c, d, e in zip(cases, *wrong.values()):
        assert a and b == (g.dil > 1 and g.k > 1), g
        assert c == (g.B > 1 and g.stride == 1 and CR.out_hw(g)[0] == g.H and g.k > 1) and d == (CR.rows_out(g) >= 64) and e == (g.groups == 1), g


def _emu_dgrad(p, accumulate, dx=None, skip=None, minus_zero=False):
    before = CR.dest(p.dxs, p.dx0 if accumulate else None)
    after = before.clone()
    r = (p.ref if dx is None else dx) + (p.dx0.double() if accumulate else 0.0)
    if minus_zero:
        r = torch.where(p.untapped, -torch.zeros_like(r), r)
    dst = CR.view(after, p.dxs)
    if skip is None:
        dst[...] = r.float()
    else:
        dst[~skip] = r.float()[~skip]
    CR.check_dest(p.dxs, before, after, p.ref + (p.dx0.double() if accumulate else 0.0), 0, "emulated dgrad", plus_zero=None if accumulate else p.untapped)


def _wrong_phase(ref):
    """the parity class (0, 0) of a stride-2 backward-data written to the phase of (1, 1) and back"""
    dx = ref.clone()
    a, b = ref[:, 0::2, 0::2], ref[:, 1::2, 1::2]
    h, w = min(a.shape[1], b.shape[1]), min(a.shape[2], b.shape[2])
    dx[:, 0::2, 0::2][:, :h, :w] = b[:, :h, :w]
    dx[:, 1::2, 1::2][:, :h, :w] = a[:, :h, :w]
    return dx


def test_checker_flags_wrong_backward_data():
    hits, untouched = [], []
    for g in CR.NAMED[CR.DGRAD]:
        p = CR.dgrad_problem(g)
        for acc in (False, True):
            _emu_dgrad(p, acc)
        if g.stride == 2:
            hits.append(_flagged(lambda: _emu_dgrad(p, True, _wrong_phase(p.ref))))
            # a class no tap reaches that a plain launch leaves unwritten (it has to write zeros there): the pixels stay payload NaNs
            none = (p.ref == 0).all(-1, keepdim=True).expand_as(p.ref) & torch.ones_like(p.ref, dtype=torch.bool)
            if g.k == 1:
                assert bool(none.any()) and torch.equal(none, p.untapped)
                assert _flagged(lambda: _emu_dgrad(p, False, minus_zero=True))         # -0 where the contract says +0
                untouched.append(_flagged(lambda: _emu_dgrad(p, False, skip=none)))
                _emu_dgrad(p, True, skip=none)                     # ... and under accumulate that is exactly what the contract says
    assert len(hits) >= 6 and sum(hits) == len(hits) - 1, hits     # (the 1 x 5 image has a single row: nothing to exchange)
    assert untouched and all(untouched)


def _emu_wgrad(p, pad_as_data=None):
    """pad_as_data: 'behind' = the column sum runs over one pad column of dy as well and stores it behind dbias; 'folded' = the pad column
    is read as one more row of the last output channel: it lands in dw[Cout - 1] and dbias[Cout - 1]"""
    g = p.g
    bw, bb = CR.dest(p.dws), CR.dest(p.dbs, salt=78)
    aw, ab = bw.clone(), bb.clone()
    dw, db = p.ref.clone(), p.dbias.clone()
    if pad_as_data == "folded":
        pad = CR.nchw(CR.view(p.DY, p.dys, (g.Cout, g.Cout + 1))).double()          # what the buffer holds there
        cig = g.Cin // g.groups
        dw[-1] += torch.nn.grad.conv2d_weight(CR.nchw(p.x).double()[:, -cig:], (1, cig, g.k, g.k), pad, g.stride, g.pad, g.dil)[0]
        db[-1] += pad.sum()
    CR.view(aw, p.dws)[...] = dw.float()
    if pad_as_data == "behind":
        n = g.Cout + 1
        s = CR.view(p.DY, p.dys, (0, n)).double().sum((0, 1, 2))
        torch.as_strided(ab, (n,), (1,), p.dbs.offset)[...] = s.float()
    else:
        CR.view(ab, p.dbs)[...] = db.float()
    CR.check_dest(p.dws, bw, aw, p.ref, 0, "emulated dw")
    CR.check_dest(p.dbs, bb, ab, p.dbias, 0, "emulated dbias")


def _emu_dbias_only(p, folded):
    bb = CR.dest(p.dbs, salt=78)
    ab = bb.clone()
    db = p.dbias.clone()
    if folded:
        db[-1] += CR.view(p.DY, p.dys, (p.g.Cout, p.g.Cout + 1)).double().sum()
    CR.view(ab, p.dbs)[...] = db.float()
    CR.check_dest(p.dbs, bb, ab, p.dbias, 0, "emulated dbias")


def test_checker_flags_a_pad_column_of_dy_treated_as_data():
    """backward-weight: the contract lets dy's pad columns hold anything, so the buffers hold NaNs there -- a kernel that reads one into
    dw, into dbias[0, Cout) or into a slot behind dbias shows, each fault on its own"""
    for g in CR.NAMED[CR.WGRAD]:
        p = CR.wgrad_problem(g)
        _emu_wgrad(p)
        _emu_dbias_only(p, False)
        if g.Cout % 4:
            assert bool(torch.isnan(CR.view(p.DY, p.dys, (g.Cout, CR.roundup4(g.Cout)))).all())
            assert _flagged(lambda: _emu_wgrad(p, pad_as_data="behind")), g
            assert _flagged(lambda: _emu_wgrad(p, pad_as_data="folded")), g
            assert _flagged(lambda: _emu_dbias_only(p, True)), g
    assert sum(1 for g in CR.NAMED[CR.WGRAD] if g.Cout % 4) >= 5
    # backward-data: the same columns are zero, as the contract demands -- a kernel may multiply them with anything finite
    for g in CR.NAMED[CR.DGRAD]:
        p = CR.dgrad_problem(g)
        pad = CR.view(p.DY, p.dys, (g.Cout, CR.roundup4(g.Cout)))
        assert pad.numel() == 0 or float(pad.abs().max()) == 0


def test_fused_statistics_test_restates_the_original_line_by_line():
    """test_conv_exact_gpu.test_fused_statistics_on_forced_forms reuses the inputs, the references and the bounds of
    test_kernels_gpu.test_conv_epilogue_bn_statistics by restating them: every such line has to stand in both sources"""
    import inspect
    import test_conv_exact_gpu as TE
    import test_kernels_gpu as TK
    lines = ["g = torch.Generator().manual_seed(sum(case))",
             "x = torch.randn(B, Cin, H, W, generator=g) + 0.5",
             "w = torch.randn(Cout, Cin, k, k, generator=g) * (2.0 / (Cin * k * k)) ** 0.5",
             "y64 = F.conv2d(x.double(), w.double(), b.double(), s, p).permute(0, 2, 3, 1).reshape(-1, Cout)",
             "rm, rv = torch.zeros(Cout, device=\"cuda\"), torch.ones(Cout, device=\"cuda\")",
             "close(stats[:Cout], mean64, atol=1e-6, rtol=2e-6)",
             "close(stats[Cout:], 1.0 / torch.sqrt(var64 + 1e-5), atol=0, rtol=2e-5)",
             "close(scale, gamma.cpu().double() / torch.sqrt(var64 + 1e-5), atol=0, rtol=2e-5)",
             "close(rm, 0.1 * mean64, atol=1e-6, rtol=1e-5)",
             "close(rv, 0.9 + 0.1 * var64 * n / max(n - 1, 1), atol=0, rtol=2e-5)",
             "rm2, rv2 = torch.zeros(Cout, device=\"cuda\"), torch.ones(Cout, device=\"cuda\")",
             "stats2, _ = ops.bn_train_stats(y, gamma, 1e-5, 0.1, rm2, rv2)",
             "close(stats, stats2.cpu(), atol=1e-6, rtol=1e-5)"]
    fragments = ["torch.randn(Cout, generator=g) * 3", "(1 + 0.1 * torch.randn(Cout, generator=g)).cuda()", "y64.var(0, unbiased=False)",
                 "gamma, 1e-5, 0.1, rm, rv)", "B, H, W, Cin, Cout, k, s, p = case"]
    original = inspect.getsource(TK.test_conv_epilogue_bn_statistics)
    copy = inspect.getsource(TE._bn_case) + inspect.getsource(TE.test_fused_statistics_on_forced_forms)
    have = lambda src: {ln.split("#")[0].strip() for ln in src.splitlines()}      # noqa: E731
    for ln in lines:
        assert ln in have(original), "test_kernels_gpu changed: " + ln
        assert ln in have(copy), "test_conv_exact_gpu differs: " + ln
    for fr in fragments:
        assert fr in original and fr in copy, fr
    assert TE._bn_forms() and TK.BNSTAT_CASES
