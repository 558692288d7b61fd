"""The train-mode kernels of PointRend (csrc/pointrend_train.hip, catseg_pointrend_gather_at), one by one, against tests/_pointrend_train_ref.py:
the device draw bit for bit against the numpy Philox, the candidate uncertainty and the gather at coordinates against fp64 (the project's
measured bar, _yardstick.within), pixel indices and labels exactly, the gather backward against fp64 autograd of F.grid_sample (and two
launches against each other, bit for bit), the scatter with its winner and its backward exactly."""
import os
import sys

import pytest
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _pointrend_ref as PR  # noqa: E402
import _pointrend_train_ref as TR  # noqa: E402
from _yardstick import within  # noqa: E402

pytestmark = pytest.mark.gpu

NESTED = ([(16, 16), (8, 8), (4, 4), (2, 2)], (32, 32))          # the stage sizes of tests/test_pointrend_kernels_gpu.py
CROOKED = ([(17, 23), (9, 12), (5, 6), (3, 3)], (34, 46))


def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")


def _logits(ops, t, ld=None, pad=0.0):
    N, K, h, w = t.shape
    v = ops.new_act(N, h, w, K, "cuda", ld=ld or max(32, (K + 3) // 4 * 4))
    ops.widen(v).fill_(pad)
    v.copy_(t.permute(0, 2, 3, 1))
    return v


def _nhwc(t):
    return t.permute(0, 2, 3, 1).contiguous().cuda()


def _state(seed, layer=0, rank=0, number=0):
    words = [seed & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF, (layer & 0xFFFF) | (rank & 0xFFFF) << 16, number]
    return torch.tensor([w - (1 << 32) if w >= 1 << 31 else w for w in words], dtype=torch.int32).cuda()


def _ties(size):
    """fp32 coordinates x whose product x (size - 1) is exactly k + 0.5 in fp32: the pixel index rounds half to even there"""
    out = []
    for k in range(size - 1):
        x = torch.tensor((k + 0.5) / (size - 1), dtype=torch.float32)
        if float(x * (size - 1)) == k + 0.5:
            out.append(float(x))
    return out


def _points(N, P, h, w, g):
    """[N, P, 2] fp32 in [0, 1): the exact corner (0, 0), the largest value below 1, the outer half cell of the coarsest map (zero
    padding attenuates there), rounding ties of the pixel index, random ones"""
    top = 1.0 - 2.0 ** -24
    tx, ty = _ties(w), _ties(h)
    assert 0.5 in tx or 0.5 in ty or len(tx) + len(ty) >= 2
    special = [(0.0, 0.0), (top, top), (top, 0.0), (0.0, top), (0.02, 0.5), (0.5, 0.98), (0.5, 0.5), (0.01, 0.015)]
    special += [(x, 0.3) for x in tx[:3]] + [(0.7, y) for y in ty[:3]]
    pts = torch.rand(N, P, 2, generator=g)
    n = min(P, len(special))
    pts[:, :n] = torch.tensor(special[:n], dtype=torch.float32)
    return pts


# ------------------------------------------------------------------------------------------------------------ draw
@pytest.mark.parametrize("N", [1, 3])
@pytest.mark.parametrize("M", [1, 5, 144])
def test_draw_equals_the_numpy_philox_and_advances_the_counter_by_one(M, N):
    _need_gpu()
    from miccai2021_cataract_semantic_segmentation_amd import ops
    seed, layer, rank = 0x1234567887654321 + M, 3, 2
    st = _state(seed, layer, rank, 7)
    for number in (7, 8, 9):
        got = ops.pointrend_draw(st, N, M)
        assert torch.equal(got.cpu(), TR.draw(seed, layer, rank, number, N, M))
        assert st.cpu().tolist()[3] == number + 1 and torch.equal(st.cpu()[:3], _state(seed, layer, rank).cpu()[:3])
        assert float(got.min()) >= 0.0 and float(got.max()) < 1.0
    fixed = torch.rand(N, M, 2).cuda()
    assert torch.equal(ops.pointrend_draw(st, N, M, fixed=fixed), fixed)
    assert st.cpu().tolist()[3] == 10                       # the fixed knob leaves the state alone


def test_draw_stream_is_disjoint_from_the_dropout_stream():
    _need_gpu()
    import _dropout_ref as DR
    from miccai2021_cataract_semantic_segmentation_amd import ops
    st = _state(99)
    pts = ops.pointrend_draw(st, 1, 64).cpu().reshape(-1)
    kept, _, _ = DR.mask(99, 0, 0, 0, 0.5, 1, 128)          # counter word 2 = 0: the same seed, layer, rank and draw number
    assert not torch.equal(pts >= 0.5, torch.from_numpy(kept).reshape(-1))


# ------------------------------------------------------------------------------------------------------------ uncertainty, compose, gather at coordinates
@pytest.mark.parametrize("K", [8, 17])
@pytest.mark.parametrize("channels", [(64, 128, 256, 512), (8, 12, 20, 4)])
@pytest.mark.parametrize("sizes,grid", [NESTED, CROOKED], ids=["nested", "non-nested"])
def test_uncertainty_compose_and_gather_at_coordinates(sizes, grid, channels, K):
    _need_gpu()
    from miccai2021_cataract_semantic_segmentation_amd import ops
    g = torch.Generator().manual_seed(sum(channels) + K + grid[1])
    N, (h, w) = 2, grid
    ch, cw = sizes[0]                                       # the coarse logits live at the finest stage's size
    feats = [torch.randn(N, c, hh, ww, generator=g) + 1.5 for c, (hh, ww) in zip(channels, sizes)]
    coarse = torch.randn(N, K, ch, cw, generator=g) * 3 + 2
    M, kb, R = 60, 20, 7
    cand, rest = _points(N, M, h, w, g), _points(N, R, h, w, g)
    cd = _logits(ops, coarse, ld=32, pad=float("inf")) if channels[0] == 8 else _nhwc(coarse)      # padded rows (pad = inf: never read) and dense ones
    # candidate uncertainty
    unc = ops.pointrend_point_uncertainty(cd, cand.cuda())
    within("point_uncertainty", "%s K=%d" % (grid, K), unc, TR.point_uncertainty(coarse.double(), cand), TR.point_uncertainty(coarse, cand))
    # selection + compose: the selected candidates in the selection's order, then the rest; pixel indices and labels exactly
    sel = ops.pointrend_topk(unc, kb)
    Hl, Wl = (4, 4) if K == 8 else (24, 32)
    lbl = torch.randint(0, K, (N, Hl, Wl), generator=g)
    lbl[torch.rand(N, Hl, Wl, generator=g) < 0.2] = K       # ignore pixels pass through
    coords, pix, labels = ops.pointrend_compose(cand.cuda(), sel, rest.cuda(), h, w, lbl.cuda())
    want = torch.cat((torch.gather(cand, 1, sel.cpu().long().unsqueeze(2).expand(-1, -1, 2)), rest), 1)
    assert torch.equal(coords.cpu(), want)
    assert torch.equal(pix.cpu().long(), TR.pixel_index(want, h, w))
    assert torch.equal(labels.cpu(), TR.point_labels(lbl, want)) and bool((labels == K).any())
    # ... and on the special points themselves (corners, ties), without a selection
    c2, pix2, lab2 = ops.pointrend_compose(None, None, cand.cuda(), h, w, lbl.cuda())
    assert torch.equal(c2.cpu(), cand) and torch.equal(pix2.cpu().long(), TR.pixel_index(cand, h, w)) and torch.equal(lab2.cpu(), TR.point_labels(lbl, cand))
    assert int(pix2.min()) == 0 and int(pix2.max()) == h * w - 1
    # gather at coordinates: every source against fp64, the four extreme points tell zero padding from clamping
    Kq = (K + 3) // 4 * 4
    extra = [torch.full((N * M, 12 + Kq), 7.0, device="cuda"), torch.full((N * M, 4 + Kq), 7.0, device="cuda")]
    cfin = _logits(ops, coarse, ld=32) if channels[0] == 8 else _nhwc(coarse)
    out = ops.pointrend_gather_at([_nhwc(f) for f in feats[::-1]] + [cfin], cand.cuda(), extras=[(extra[0], 12), (extra[1], 4)])
    got = out.cpu().view(N, M, -1)
    c0, told = 0, False
    for s in feats[::-1] + [coarse]:
        C = s.shape[1]
        ref64, cpu32 = PR.point_sample(s.double(), cand), PR.point_sample(s, cand)
        mine = got[:, :, c0:c0 + C].permute(0, 2, 1)
        within("gather_at", "%s C=%d map %s" % (grid, C, tuple(s.shape[2:])), mine, ref64, cpu32)
        clamped = PR.point_sample(s.double(), cand, padding_mode="border")
        if float((ref64 - clamped).abs()[:, :, :4].max()) > 1e-3:
            told = True
            assert float((mine.double() - clamped).abs()[:, :, :4].max()) > 1e-3
        c0 += (C + 3) // 4 * 4
    assert told, "no point of this case tells zero padding from clamping"
    assert not bool(got[:, :, c0 - Kq + K:c0].any())        # the pad columns of the coarse block are zero
    for e, o in zip(extra, (12, 4)):
        assert torch.equal(e[:, o:], out[:, c0 - Kq:c0]) and bool((e[:, :o] == 7.0).all())


def test_gather_at_a_cell_centre_agrees_with_the_index_form():
    """The index form derives the cell centre on the device (one fused multiply-add), the coordinate form reads the centre torch formed
    with two roundings: the two x (and y) differ by at most one ulp of a value in [0, 1), 2^-24.  That moves a tap position by at most
    2^-24 max(H, W) cells, and the sample by at most that times the largest difference of two values of a map, once along x and once along
    y; the bar is twice that, for the roundings of the two evaluations themselves."""
    _need_gpu()
    from miccai2021_cataract_semantic_segmentation_amd import ops
    g = torch.Generator().manual_seed(5)
    sizes, (h, w) = CROOKED
    N, K = 2, 17
    maps = [torch.randn(N, c, hh, ww, generator=g) for c, (hh, ww) in zip((20, 12), sizes[1:3])] + [torch.randn(N, K, h, w, generator=g)]
    srcs = [_nhwc(m) for m in maps[:2]] + [_logits(ops, maps[2], ld=32)]
    idx = torch.stack([torch.randperm(h * w, generator=g)[:50] for _ in range(N)])
    a = ops.pointrend_gather(srcs, idx.int().cuda(), h, w)
    b = ops.pointrend_gather_at(srcs, PR.point_coords(idx, h, w).contiguous().cuda())
    bar = 2 * 2 * 2.0 ** -24 * max(h, w) * max(float(m.max() - m.min()) for m in maps)
    print("index form vs coordinate form: max |difference| %.3g, bar %.3g" % (float((a - b).abs().max()), bar))
    assert float((a - b).abs().max()) <= bar
    same = ops.pointrend_gather_at(srcs, PR.point_coords(idx, h, w).contiguous().cuda())
    assert torch.equal(b, same)


# ------------------------------------------------------------------------------------------------------------ selection on clustered values
def test_selection_keeps_ascending_candidate_order():
    _need_gpu()
    from miccai2021_cataract_semantic_segmentation_amd import ops
    g = torch.Generator().manual_seed(11)
    unc = -torch.rand(3, 144, generator=g)
    sel = ops.pointrend_topk(unc.cuda(), 36).cpu().long()
    cand = torch.rand(3, 144, 2, generator=g)
    _, idx = TR.select_points(unc, cand, None, 36)
    assert torch.equal(sel, idx)


# ------------------------------------------------------------------------------------------------------------ gather backward
def _clustered(N, P, h, w, sizes, g):
    """points with >= 3 on one pixel of every map, points that share only some taps, and taps outside the maps"""
    pts = _points(N, P, h, w, g)
    if P >= 7:
        fh, fw = sizes[0]
        pts[:, 3] = pts[:, 4] = pts[:, 2] = torch.tensor([0.4, 0.6])          # three points at one place
        pts[:, 5] = torch.tensor([0.4 + 1.0 / fw, 0.6])                       # one cell of the finest map to the right: shares two of its taps
        pts[:, 6] = torch.tensor([0.4, 0.6 + 0.3 / fh])
    return pts


def _gather_bwd_reference(srcs, pts, dX, dtype):
    leaves = [s.to(dtype).requires_grad_() for s in srcs]
    cols = torch.cat([PR.point_sample(s, pts) for s in leaves], 1)            # [N, sum C, P]
    (cols * dX.to(dtype)).sum().backward()
    return [s.grad for s in leaves]


@pytest.mark.parametrize("N", [1, 3])
@pytest.mark.parametrize("P", [1, 7, 48, 300])
@pytest.mark.parametrize("accumulate", [False, True], ids=["write", "accumulate"])
def test_gather_backward_matches_fp64_autograd_and_itself(accumulate, P, N):
    _need_gpu()
    from miccai2021_cataract_semantic_segmentation_amd import ops
    g = torch.Generator().manual_seed(100 * P + N)
    big = P == 48
    sizes, (h, w) = (NESTED if big else CROOKED)
    channels, K = ((64, 128, 256, 512), 8) if big else ((8, 12, 20, 4), 17)
    shapes = [(c, hh, ww) for c, (hh, ww) in zip(channels, sizes)][::-1] + [(K,) + sizes[0]]          # deepest first, the coarse logits last
    pts = _clustered(N, P, h, w, sizes, g)
    srcs = [torch.randn(N, c, hh, ww, generator=g) for c, hh, ww in shapes]
    dXs = [torch.randn(N, c, P, generator=g) for c, _, _ in shapes]
    cols = sum((c + 3) // 4 * 4 for c, _, _ in shapes)
    dx = torch.full((N * P, cols + 4), float("nan"))                          # (a row stride beyond the blocks, NaN in the pad columns)
    c0 = 0
    for (c, _, _), d in zip(shapes, dXs):
        dx[:, c0:c0 + (c + 3) // 4 * 4] = 0.0
        dx[:, c0:c0 + c] = d.permute(0, 2, 1).reshape(N * P, c)
        c0 += (c + 3) // 4 * 4
    dx[:, c0 - ((K + 3) // 4 * 4) + K:c0] = 123.0                              # the pad columns of the coarse block: whatever they hold stays out
    r64 = _gather_bwd_reference(srcs, pts, torch.cat(dXs, 1), torch.float64)
    r32 = _gather_bwd_reference(srcs, pts, torch.cat(dXs, 1), torch.float32)
    base = [torch.randn(N, hh, ww, c, generator=g) if accumulate else torch.full((N, hh, ww, c), float("nan")) for c, hh, ww in shapes]

    def run():
        dests = []
        for (c, hh, ww), b0 in zip(shapes, base):
            buf = ops.new_act(N, hh, ww, c, "cuda", ld=32 if c == K else None)
            ops.widen(buf).fill_(0.0 if accumulate else float("nan"))
            buf.copy_(b0)
            dests.append((buf, accumulate))
        ops.pointrend_gather_bwd(dx.cuda(), pts.cuda(), dests)
        return [ops.widen(d).clone() for d, _ in dests]

    first, second = run(), run()
    for a, b in zip(first, second):
        assert torch.equal(a, b), "two launches of the gather backward differ"
    for (c, hh, ww), got, a64, a32, b0 in zip(shapes, first, r64, r32, base):
        assert not bool(got[..., c:].cpu().ne(0).any())                       # the pad columns of a padded destination receive zero
        mine = got[..., :c].cpu().permute(0, 3, 1, 2)
        plus = b0.permute(0, 3, 1, 2).double() if accumulate else 0.0
        within("gather_bwd", "P=%d N=%d C=%d map %dx%d %s" % (P, N, c, hh, ww, "acc" if accumulate else "write"), mine, a64 + plus, (a32.double() + plus).float())
        untouched = (a64 == 0).all(1, keepdim=True).expand_as(a64)
        want = b0.permute(0, 3, 1, 2) if accumulate else torch.zeros_like(mine)
        assert torch.equal(mine[untouched], want[untouched])                   # pixels no tap touches: zero, or unchanged under accumulate


def test_gather_backward_sweeps_more_than_one_register_group_of_channels():
    _need_gpu()
    from miccai2021_cataract_semantic_segmentation_amd import ops
    g = torch.Generator().manual_seed(8)
    N, P, C = 1, 7, 2052                                                       # 2048 channels per sweep: the second sweep takes four
    pts = _clustered(N, P, 12, 12, [(3, 3)], g)
    src, dX = torch.randn(N, C, 3, 3, generator=g), torch.randn(N, C, P, generator=g)
    r64, r32 = _gather_bwd_reference([src], pts, dX, torch.float64)[0], _gather_bwd_reference([src], pts, dX, torch.float32)[0]
    dst = torch.full((N, 3, 3, C), float("nan"), device="cuda")
    ops.pointrend_gather_bwd(dX.permute(0, 2, 1).reshape(N * P, C).contiguous().cuda(), pts.cuda(), [(dst, False)])
    within("gather_bwd", "C=2052", dst.cpu().permute(0, 3, 1, 2), r64, r32)


# ------------------------------------------------------------------------------------------------------------ scatter and its backward
@pytest.mark.parametrize("K,h,w,P", [(17, 6, 9, 20), (8, 32, 32, 300), (25, 1, 1, 3)])
def test_scatter_last_point_wins_and_its_backward_is_exact(K, h, w, P):
    _need_gpu()
    from miccai2021_cataract_semantic_segmentation_amd import ops
    g = torch.Generator().manual_seed(K + P)
    N, Kq = 3, (K + 3) // 4 * 4
    seg = torch.randn(N, K, h, w, generator=g)
    pix = torch.randint(0, h * w, (N, P), generator=g)
    if P >= 20:
        pix[:, 5] = pix[:, 17] = pix[:, 2]                                     # three points on one pixel; P = 300 on 1024 pixels has many more
    assert int(torch.stack([torch.bincount(r, minlength=h * w).max() for r in pix]).min()) >= 3
    vals = torch.randn(N, K, P, generator=g)
    sd = _nhwc(seg) if K == 25 else _logits(ops, seg, ld=Kq)                   # dense rows and padded ones
    rd = torch.full((N * P, Kq), 9.0, device="cuda")
    rd[:, :K] = vals.permute(0, 2, 1).reshape(N * P, K).cuda()
    pd = pix.int().cuda()
    ops.pointrend_scatter_last(rd, pd, sd)
    assert torch.equal(sd.cpu().permute(0, 3, 1, 2), TR.scatter_last(seg, pix, vals))
    assert K == 25 or not bool(ops.widen(sd)[..., K:].any())
    # backward: every duplicate receives its pixel's gradient; the gradient of the scattered-into tensor is zero at every scattered pixel
    dpred = torch.randn(N, K, h, w, generator=g)
    leaf_s, leaf_v = seg.clone().requires_grad_(), vals.clone().requires_grad_()
    (TR._ScatterLast.apply(leaf_s, pix, leaf_v) * dpred).sum().backward()
    for acc in (False, True):
        dd = _nhwc(dpred) if K == 25 else _logits(ops, dpred, ld=Kq)
        before = torch.randn(N * P, Kq, generator=g)
        dr = before.clone().cuda()
        ops.pointrend_scatter_bwd(dd, pd, dr, acc)
        want = leaf_v.grad.permute(0, 2, 1).reshape(N * P, K)
        assert torch.equal(dr[:, :K].cpu(), before[:, :K] + want if acc else want)
        assert torch.equal(dr[:, K:].cpu(), before[:, K:])
        assert torch.equal(dd.cpu().permute(0, 3, 1, 2), leaf_s.grad)
