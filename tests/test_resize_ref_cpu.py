"""The references and case tables of tests/_resize_ref.py, checked without a GPU: the second reference (bilinear_matrix) agrees with
float64 F.interpolate, every case of the tables reaches the launcher route it names (by the transcription of the launchers kept there),
every route of catseg_bilinear_fwd / catseg_bilinear_bwd is named by a case, and every slice of the tables lies inside its buffer."""
import pytest
import torch

import _resize_ref as R


def _sizes():
    s = set()
    for c in R.FWD_CASES:
        _, B, H, W, C, Ho, Wo, ldx, xoff, ldy, yoff, align = c
        s.add((H, W, Ho, Wo, align))
    for c in R.BWD_CASES:
        _, B, H, W, C, Ho, Wo, lddy, align, zero_to, lddx, dxoff = c
        s.add((H, W, Ho, Wo, align))
    return sorted(s)


@pytest.mark.parametrize("size", _sizes(), ids=lambda s: "%dx%d-to-%dx%d-%s" % (s[0], s[1], s[2], s[3], "ac" if s[4] else "hp"))
def test_matrix_reference_agrees_with_float64_interpolate(size):
    H, W, Ho, Wo, align = size
    g = R.gen(H, W, Ho, Wo, align)
    x = torch.randn(2, H, W, 3, generator=g, dtype=torch.float64)
    dy = torch.randn(2, Ho, Wo, 3, generator=g, dtype=torch.float64)
    for name, got, ref in (("forward", R.bilinear_matrix_fwd(x, Ho, Wo, align), R.bilinear_ref(x, Ho, Wo, align, torch.float64)),
                           ("transpose", R.bilinear_matrix_bwd(dy, H, W, align), R.bilinear_bwd_ref(dy, H, W, align, torch.float64))):
        assert got.shape == ref.shape
        err, scale = (got - ref).abs().max().item(), ref.abs().max().item()
        assert err <= 1e-12 * scale, "%s: %g of scale %g" % (name, err, scale)
    # every output pixel's weights sum to 1
    for n_in, n_out in ((H, Ho), (W, Wo)):
        assert (R.bilinear_matrix(n_in, n_out, align).sum(1) - 1).abs().max().item() <= 1e-15


@pytest.mark.parametrize("case", R.FWD_CASES, ids=R.fwd_id)
def test_forward_case_reaches_its_route(case):
    assert R.fwd_route(case)["route"] == case[0], R.fwd_route(case)


@pytest.mark.parametrize("case", R.BWD_CASES, ids=R.bwd_id)
def test_backward_case_reaches_its_route(case):
    r = R.bwd_route(case, 1)
    assert r["route"] == case[0], r
    # with the fused launch switched off every case takes the two passes, with the row kernel of its layout
    r0 = R.bwd_route(case, 0)
    assert r0["route"] == "twopass-forced" and r0["kernel"] == "bilinear_bwd_rows<%d>+cols" % r["mode"], r0
    if r["kernel"].startswith("bilinear_bwd_fused"):
        # what the host's estimate 2 / sh + 8 <= BIL_MAXROWS promises the kernel: its list holds every row with a non-zero weight
        assert R.listed_rows(case) <= R.BIL_MAXROWS, R.listed_rows(case)
        assert 0 < r["lds_floats"] <= R.LDS_CAP


def test_every_route_is_named_by_a_case():
    assert {c[0] for c in R.FWD_CASES} == set(R.FWD_ROUTES)
    assert {c[0] for c in R.BWD_CASES} == set(R.BWD_ROUTES)
    # and by the transcription, not only by the label
    assert {R.fwd_route(c)["route"] for c in R.FWD_CASES} == set(R.FWD_ROUTES)
    assert {R.bwd_route(c, 1)["route"] for c in R.BWD_CASES} == set(R.BWD_ROUTES)
    assert {R.fwd_route(c)["kernel"] for c in R.FWD_CASES} == {"bilinear_fwd<0>", "bilinear_fwd<1>", "bilinear_fwd<2>", "bilinear_fwd_lds"}
    kernels = {R.bwd_route(c, f)["kernel"] for c in R.BWD_CASES for f in (0, 1)}
    assert kernels == {"bilinear_bwd_fused<1>", "bilinear_bwd_fused<2>", "bilinear_bwd_rows<0>+cols", "bilinear_bwd_rows<1>+cols",
                       "bilinear_bwd_rows<2>+cols"}
    # the edges the tables are there for
    bw = {c: R.bwd_route(c, 1) for c in R.BWD_CASES}
    assert any(R.listed_rows(c) == R.BIL_MAXROWS for c, r in bw.items() if r["route"] == "fused1-maxrows"), "no case fills the row list"
    assert any(r["route"] == "fused1-lds-cap" and r["cap_halvings"] == 1 for r in bw.values())
    assert any(r["route"] == "fused1-lds-cap" and r["nseg"] >= 32 for r in bw.values())
    assert any(r["route"] == "fused2-chunks-ragged" and c[4] % 96 == 4 and c[9] > c[4] for c, r in bw.items())
    assert any(r["route"] == "fused2-chunks-ragged" and r["nchunk"] == 3 and c[4] % 96 == 8 for c, r in bw.items())
    assert any(r["route"] == "fused2-seg-above-8" and r["seg"] == 16 for r in bw.values())
    assert any(r.get("ysplit_r", 1) > 1 for r in bw.values()) and any(r.get("ysplit_c", 1) > 1 for r in bw.values())
    assert any(c[4] < 4 and R.fwd_route(c)["kernel"] == "bilinear_fwd<1>" for c in R.FWD_CASES)
    assert any(c[4] < 4 and R.fwd_route(c)["kernel"] == "bilinear_fwd_lds" for c in R.FWD_CASES)


def _ld_seen(shape, ld):
    """the pixel stride ops.ld_of derives from a (B, H, W, C) view: with a single pixel there is no stride to read and it assumes C rounded up to 4"""
    B, H, W, C = shape
    return ld if B * H * W > 1 else (C + 3) // 4 * 4


def test_every_slice_lies_inside_its_buffer():
    for c in R.FWD_CASES:
        _, B, H, W, C, Ho, Wo, ldx, xoff, ldy, yoff, align = c
        assert min(B, H, W, C, Ho, Wo) >= 1 and xoff >= 0 and yoff >= 0
        assert xoff + C <= ldx and yoff + C <= ldy, c
        assert _ld_seen((B, H, W, C), ldx) == ldx and _ld_seen((B, Ho, Wo, C), ldy) == ldy, c
        assert B * max(H * W * ldx, Ho * Wo * ldy) <= 400000, c
    for c in R.BWD_CASES:
        _, B, H, W, C, Ho, Wo, lddy, align, zero_to, lddx, dxoff = c
        assert min(B, H, W, C, Ho, Wo) >= 1 and dxoff >= 0 and zero_to >= 0
        assert C <= lddy and dxoff + max(C, zero_to) <= lddx, c
        assert _ld_seen((B, H, W, C), lddx) == lddx and _ld_seen((B, Ho, Wo, C), lddy) == lddy, c
        assert B * max(H * W * lddx, Ho * Wo * lddy) <= 600000, c
    for c in R.POOL_CASES:
        _, B, S, H, W, C, ldx, xoff, lddx, dxoff = c
        assert 1 <= S <= 64 and xoff + C <= ldx and dxoff + C <= lddx, c
        assert C % 4 == 0 and lddx % 4 == 0 and dxoff % 4 == 0, c          # what catseg_adaptive_avgpool_bwd requires
        assert _ld_seen((B, H, W, C), ldx) == ldx and _ld_seen((B, H, W, C), lddx) == lddx, c
    assert any(c[5] > 256 for c in R.POOL_CASES) and any(c[6] == c[5] + 8 and c[8] == c[5] + 4 for c in R.POOL_CASES)
