"""The kernels of csrc/pointrend.hip, one by one: upsample x 2 + uncertainty against the bilinear launch (bit for bit) and the top-2 difference, the
top-k selection against the tie rule of tests/_pointrend_ref.py (exact index sets), the point gather against F.grid_sample in fp64
(calibrated by torch-CPU fp32's own distance), the scatter exactly."""
import os
import sys

import pytest
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _pointrend_ref as PR  # noqa: E402

pytestmark = pytest.mark.gpu


def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")


def _logits(ops, t, ld=None, pad=0.0):
    """NCHW CPU logits -> the engine's padded row layout on the device: a [N, h, w, K] view of rows ld floats wide, pad columns = pad"""
    N, K, h, w = t.shape
    v = ops.new_act(N, h, w, K, "cuda", ld=ld or max(32, (K + 3) // 4 * 4))
    ops.widen(v).fill_(pad)
    v.copy_(t.permute(0, 2, 3, 1))
    return v


def _nhwc(t):
    return t.permute(0, 2, 3, 1).contiguous().cuda()


# ------------------------------------------------------------------------------------------------------------ upsample + uncertainty
@pytest.mark.parametrize("N", [1, 3])
@pytest.mark.parametrize("H,W", [(1, 1), (5, 7), (24, 32)])
@pytest.mark.parametrize("K", [2, 8, 17, 25])
def test_upsample2x_equals_the_bilinear_launch_and_the_top2_difference(K, H, W, N):
    _need_gpu()
    from miccai2021_cataract_semantic_segmentation_amd import ops
    g = torch.Generator().manual_seed(1000 * K + 10 * H + N)
    x = torch.randn(N, K, H, W, generator=g) * 3
    x[:, :, 0, 0] = x[:, :1, 0, 0]            # a pixel whose logits are all equal: uncertainty exactly 0
    xd = _logits(ops, x)
    want = ops.bilinear_fwd(xd, 2 * H, 2 * W, False)
    up, unc = ops.pointrend_upsample2x(xd)
    assert up.shape == (N, 2 * H, 2 * W, K) and unc.shape == (N, 2 * H, 2 * W)
    assert torch.equal(up, want)
    top2 = torch.topk(up.cpu(), 2, dim=3)[0]
    assert torch.equal(unc.cpu(), top2[..., 1] - top2[..., 0])
    assert float(unc.max()) <= 0 and float(unc[0, 0, 0]) == 0.0


def test_upsample2x_never_reads_the_pad_columns_into_a_result():
    _need_gpu()
    from miccai2021_cataract_semantic_segmentation_amd import _lib, ops
    x = torch.randn(2, 17, 5, 7, generator=torch.Generator().manual_seed(3))
    clean, dirty = _logits(ops, x), _logits(ops, x, pad=float("inf"))
    (a, ua), (b, ub) = ops.pointrend_upsample2x(clean), ops.pointrend_upsample2x(dirty)
    assert torch.equal(a, b) and torch.equal(ua, ub) and bool(torch.isfinite(ub).all()) and bool(torch.isfinite(b).all())
    wide = ops.new_act(2, 10, 14, 17, "cuda", ld=32)            # the uncertainty kernel on padded rows of its own: +inf beside the 17 logits
    ops.widen(wide).fill_(float("inf"))
    wide.copy_(a)
    uw = torch.empty_like(ua)
    _lib.check(_lib.lib.catseg_pointrend_uncertainty(wide.data_ptr(), 32, uw.data_ptr(), uw.numel(), 17, _lib.stream()))
    assert torch.equal(uw, ua)


# ------------------------------------------------------------------------------------------------------------ selection
def _values(kind, N, n, g):
    if kind == "continuous":
        return torch.randn(N, n, generator=g)
    if kind == "equal":
        return torch.full((N, n), -0.75)
    if kind == "four levels":
        return -torch.randint(0, 4, (N, n), generator=g).float() / 4
    z = torch.zeros(N, n)                      # "signed zeros": -0.0, +0.0 and a few -1
    z[torch.rand(N, n, generator=g) < 0.5] = -0.0
    z[torch.rand(N, n, generator=g) < 0.2] = -1.0
    return z


@pytest.mark.parametrize("kind", ["continuous", "equal", "four levels", "signed zeros"])
@pytest.mark.parametrize("n", [1, 63, 64, 65, 3072, 70001])
def test_topk_selects_the_exact_index_set_under_the_tie_rule(n, kind):
    _need_gpu()
    from miccai2021_cataract_semantic_segmentation_amd import ops
    for N in (1, 3):
        u = _values(kind, N, n, torch.Generator().manual_seed(n + N))
        ud = u.cuda()
        for k in sorted({k for k in (1, n - 1, n, 2 * n, 784) if k >= 1}):
            got = ops.pointrend_topk(ud, k)
            again = ops.pointrend_topk(ud, k)
            want = torch.sort(PR.select(u, k), dim=1)[0]
            assert got.dtype == torch.int32 and got.shape == (N, min(k, n))
            assert torch.equal(got.cpu().long(), want), (n, kind, N, k)      # (ascending: the list itself is pinned, not only the set)
            assert torch.equal(got, again)


# ------------------------------------------------------------------------------------------------------------ gather
NESTED = ([(16, 16), (8, 8), (4, 4), (2, 2)], (32, 32))
CROOKED = ([(17, 23), (9, 12), (5, 6), (3, 3)], (34, 46))


@pytest.mark.parametrize("K", [8, 17])
@pytest.mark.parametrize("channels", [(64, 128, 256, 512), (8, 12, 20, 4)])
@pytest.mark.parametrize("sizes,grid", [NESTED, CROOKED], ids=["nested", "non-nested"])
def test_gather_matches_grid_sample_with_zero_padding(sizes, grid, channels, K):
    _need_gpu()
    from miccai2021_cataract_semantic_segmentation_amd import ops
    g = torch.Generator().manual_seed(sum(channels) + K + grid[1])
    N, (h, w) = 2, grid
    feats = [torch.randn(N, c, hh, ww, generator=g) + 1.5 for c, (hh, ww) in zip(channels, sizes)]     # (a non-zero mean: an attenuated border tap shows)
    seg = torch.randn(N, K, h, w, generator=g) * 3 + 2
    corners = [0, w - 1, (h - 1) * w, h * w - 1]
    edges = [w // 2, (h // 2) * w, (h // 2) * w + w - 1, (h - 1) * w + w // 3, 1, w]
    idx = torch.stack([torch.tensor(corners + edges + torch.randint(0, h * w, (54,), generator=g).tolist()) for _ in range(N)])
    k = idx.shape[1]
    srcs = feats[::-1] + [seg]
    Kq = (K + 3) // 4 * 4
    extra = [torch.full((N * k, 12 + Kq), 7.0, device="cuda"), torch.full((N * k, 4 + Kq), 7.0, device="cuda")]
    # the coarse logits as dense rows of K floats (what the resize launch writes: one channel per lane) or as padded rows (16-byte loads)
    segd = _nhwc(seg) if channels[0] == 8 else _logits(ops, seg, ld=32)
    out = ops.pointrend_gather([_nhwc(f) for f in feats[::-1]] + [segd], idx.int().cuda(), h, w,
                               extras=[(extra[0], 12), (extra[1], 4)])
    assert out.shape == (N * k, sum(channels) + Kq)
    got = out.cpu().view(N, k, -1)
    pts = PR.point_coords(idx, h, w)                       # fp32, as the reference forms them
    c0, told = 0, False
    for s in srcs:
        C = s.shape[1]
        ref64 = PR.point_sample(s.double(), pts)           # the restatement in fp64, fed the fp32 coordinates
        cpu32 = PR.point_sample(s, pts)
        clamped = PR.point_sample(s.double(), pts, padding_mode="border")
        mine = got[:, :, c0:c0 + C].permute(0, 2, 1).double()
        d_kernel, d_torch = float((mine - ref64).abs().max()), float((cpu32.double() - ref64).abs().max())
        bar = 4 * d_torch + 1e-6 * float(s.abs().max())
        print("gather %s C=%d map %s: kernel %.3g, torch-CPU fp32 %.3g from fp64 (ratio %.2f), bar %.3g"
              % (grid, C, tuple(s.shape[2:]), d_kernel, d_torch, d_kernel / max(d_torch, 1e-30), bar))
        assert d_kernel <= bar
        # the four corners lie in the outer half cell of every map coarser than the grid: zero padding attenuates them, clamping would not
        gap = (ref64 - clamped).abs()[:, :, :4]
        if float(gap.max()) > bar:
            told = True
            assert float((mine - clamped).abs()[:, :, :4].max()) > bar
        c0 += (C + 3) // 4 * 4
    assert told, "no point of this case tells zero padding from clamping"
    assert not bool(got[:, :, c0 - Kq + K:c0].any())       # the pad columns of the coarse block are zero
    coarse = out[:, c0 - Kq:c0]
    for e, o in zip(extra, (12, 4)):
        assert torch.equal(e[:, o:], coarse) and bool((e[:, :o] == 7.0).all())


# ------------------------------------------------------------------------------------------------------------ scatter
@pytest.mark.parametrize("K,h,w,k", [(17, 6, 9, 20), (8, 32, 32, 1024), (25, 1, 1, 1)])
def test_scatter_is_exact(K, h, w, k):
    _need_gpu()
    from miccai2021_cataract_semantic_segmentation_amd import ops
    g = torch.Generator().manual_seed(K + k)
    N, Kq = 3, (K + 3) // 4 * 4
    seg = torch.randn(N, K, h, w, generator=g)
    idx = torch.stack([torch.randperm(h * w, generator=g)[:k] for _ in range(N)])
    rows = torch.randn(N, K, k, generator=g)
    want = PR.scatter_points(seg, idx, rows)
    sd = _nhwc(seg) if K == 25 else _logits(ops, seg, ld=Kq)       # dense rows (the resize launch's output) and padded ones
    rd = torch.full((N * k, Kq), 9.0, device="cuda")
    rd[:, :K] = rows.permute(0, 2, 1).reshape(N * k, K).cuda()
    ops.pointrend_scatter(rd, idx.int().cuda(), sd)
    assert torch.equal(sd.cpu().permute(0, 3, 1, 2), want)
    assert K == 25 or not bool(ops.widen(sd)[..., K:].any())
