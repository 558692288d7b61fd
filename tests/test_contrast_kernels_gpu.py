"""The kernels of the dense contrastive loss (csrc/contrast.hip) one by one on the device: the anchor pick exactly against the integer
restatement, gather / scatter_bwd and rows + finalize + the two products against fp64 with the measured bound of tests/_yardstick.py
(the same lines run in fp32 on the CPU are the yardstick, bar 4 x).  Small shapes: each case takes well under a second on the device."""
import numpy as np
import pytest
import torch

import _contrast_ref as CR
from _yardstick import WORST, within

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SEED, LAYER, RANK = 0x5EED0000BEEF, 0, 2


def _state(draw=0):
    words = [SEED & 0xFFFFFFFF, SEED >> 32, (LAYER & 0xFFFF) | RANK << 16, draw]
    return torch.tensor([w - (1 << 32) if w >= 1 << 31 else w for w in words], dtype=torch.int32, device=DEV)


def _check_pick(lbl, h, w, K, M, u, got):
    idx, lab, n_pos = (t.cpu().numpy().astype(np.int64) for t in got)
    ridx, rlab, rn = CR.pick(lbl, h, w, K, M, u)
    assert np.array_equal(idx, ridx) and np.array_equal(lab, rlab) and int(n_pos[0]) == rn


# ---------------------------------------------------------------------------------------------------------------- pick
def _count_map(B, h, w, K, M, seed, first=0):
    """a label map at the feature resolution whose classes have 0, 1, M - 1, M, M + 1, ... pixels; every other pixel is K, 255 or -1"""
    rng = np.random.default_rng(seed)
    N = B * h * w
    wanted = [0, 1, M - 1, M, M + 1, 3 * M + 1, 2, M + 2]
    wanted = wanted[first:] + wanted[:first]
    flat = rng.choice(np.array([K, 255, -1]), N)
    perm, used, counts = rng.permutation(N), 0, []
    for c in range(K):
        n = min(wanted[c % len(wanted)], N - used)
        flat[perm[used:used + n]] = c
        used += n
        counts.append(n)
    return flat.reshape(B, h, w), counts


@pytest.mark.parametrize("shape,K,M", [((2, 64, 96, 8, 12), 5, 4), ((2, 60, 96, 8, 13), 5, 8), ((1, 257, 1, 257, 1), 2, 64), ((3, 16, 16, 16, 16), 25, 8),
                                       ((3, 16, 16, 16, 16), 25, 64), ((2, 64, 96, 8, 12), 2, 64)])
def test_pick_is_the_restatement(shape, K, M):
    from miccai2021_cataract_semantic_segmentation_amd import ops
    B, H, W, h, w = shape
    A = K * M
    rng = np.random.default_rng(K * 1000 + M)
    if (H, W) == (h, w):
        lbl, counts = _count_map(B, h, w, K, M, K + M, first=4 if K == 2 else 0)      # (two classes: both larger than M, across the chunk border)
        assert len(set(counts)) > 1 and max(counts) > M
    else:
        lbl = rng.integers(-1, K + 2, (B, H, W))
        lbl[lbl == K + 1] = 255
    dl = torch.from_numpy(lbl).to(DEV)
    state = _state(draw=5)
    for launch in range(2):                      # the draws are the restated Philox words; the counter moves by one per launch
        got = ops.contrast_pick(dl, h, w, K, M, state=state)
        _check_pick(lbl, h, w, K, M, CR.draw_u24(SEED, LAYER, RANK, 5 + launch, A), got)
        assert state.tolist() == _state(draw=6 + launch).tolist()
    fixed = rng.integers(0, 1 << 24, A)
    fixed[:2] = (0, (1 << 24) - 1)
    before = state.clone()
    _check_pick(lbl, h, w, K, M, fixed, ops.contrast_pick(dl, h, w, K, M, state=state, fixed_u=torch.from_numpy(fixed.astype(np.int32)).to(DEV)))
    _check_pick(lbl, h, w, K, M, np.full(A, 1 << 23), ops.contrast_pick(dl, h, w, K, M, state=state, eval_mode=True))
    _check_pick(lbl, h, w, K, M, np.full(A, 1 << 23), ops.contrast_pick(dl, h, w, K, M, state=None, eval_mode=True))
    assert torch.equal(state, before)


@pytest.mark.parametrize("fill", ["all_one_class", "nothing_valid"])
def test_pick_degenerate_maps(fill):
    from miccai2021_cataract_semantic_segmentation_amd import ops
    K, M, B, h, w = 5, 8, 2, 9, 31
    lbl = np.full((B, h, w), 3 if fill == "all_one_class" else 255, dtype=np.int64)
    if fill == "nothing_valid":
        lbl[0, :4] = K
        lbl[1, 2] = -1
    state = _state()
    got = ops.contrast_pick(torch.from_numpy(lbl).to(DEV), h, w, K, M, state=state)
    _check_pick(lbl, h, w, K, M, CR.draw_u24(SEED, LAYER, RANK, 0, K * M), got)
    assert int(got[2]) == (M if fill == "all_one_class" else 0)
    assert int((got[1] >= 0).sum()) == (M if fill == "all_one_class" else 0)


def test_pick_refuses_too_many_slots():
    from miccai2021_cataract_semantic_segmentation_amd import ops
    with pytest.raises(ValueError, match="exceed 8192"):
        ops.contrast_pick(torch.zeros((1, 8, 8), dtype=torch.int64, device=DEV), 8, 8, 65, 128, state=_state())


# ---------------------------------------------------------------------------------------------------------------- gather, scatter_bwd
GUARD = 7.25


def _guarded(rows, cols):
    """a [rows, cols] fp32 view in the middle of a buffer of guard values"""
    n = rows * cols
    pad = 64
    buf = torch.full((n + 2 * pad,), GUARD, dtype=torch.float32, device=DEV)
    return buf, buf[pad:pad + n].view(rows, cols)


def _guards_intact(buf, n):
    return bool((buf[:64] == GUARD).all()) and bool((buf[64 + n:] == GUARD).all())


def _features(n_pix, d, seed):
    g = torch.Generator().manual_seed(seed)
    f = torch.randn(n_pix, d, generator=g)
    wide = torch.full((n_pix, d + 4), float("nan"))           # the columns between the rows are never read
    wide[:, :d] = f
    return f, wide.to(DEV)[:, :d]


@pytest.mark.parametrize("d", [4, 6, 128, 132])
def test_gather_normalises_the_anchor_rows(d):
    from miccai2021_cataract_semantic_segmentation_amd import ops
    n_pix, A = 90, 24
    f, fd = _features(n_pix, d, 20 + d)
    f[7] = 0.0
    fd[7] = 0.0
    rng = np.random.default_rng(d)
    perm = rng.permutation(n_pix)
    idx = perm[perm != 7][:A]
    idx[3] = 7                                                 # a zero feature row
    idx[[5, 11, 23]] = -1                                      # empty slots
    di = torch.from_numpy(idx.astype(np.int32)).to(DEV)
    dp = (d + 3) // 4 * 4
    zbuf, Z = _guarded(A, dp)
    nbuf, inv = _guarded(A, 1)
    ops.contrast_gather(fd.view(1, 1, n_pix, d), di, 1e-12, Z=Z, inv_norm=inv.view(-1))
    filled = idx >= 0
    rows = torch.from_numpy(np.where(filled, idx, 0))
    mask = torch.from_numpy(filled)[:, None]
    ref64 = torch.where(mask, torch.nn.functional.normalize(f.double()[rows], dim=1, eps=1e-12), torch.zeros((), dtype=torch.float64))
    ref32 = torch.where(mask, torch.nn.functional.normalize(f[rows], dim=1, eps=1e-12), torch.zeros(()))
    within("contrast_gather", "d=%d" % d, Z[:, :d], ref64, ref32)
    got = Z.cpu()
    assert bool((got[:, d:] == 0).all()) and bool((got[~torch.from_numpy(filled)] == 0).all()) and bool((got[3] == 0).all())
    assert _guards_intact(zbuf, A * dp) and _guards_intact(nbuf, A)
    n64 = f.double()[rows].norm(dim=1)
    gi = inv.view(-1).cpu().double()
    assert bool((gi[~torch.from_numpy(filled)] == 0).all()) and gi[3] == -float(np.float32(1) / np.float32(1e-12))
    ok = torch.from_numpy(filled).clone()
    ok[3] = False
    assert float(((gi[ok] * n64[ok]) - 1).abs().max()) < 4 * 2.0 ** -23


@pytest.mark.parametrize("d,eps", [(4, 1e-12), (6, 1e-12), (128, 1e-12), (132, 1e-12), (6, 2.0)])
def test_scatter_bwd_is_the_adjoint_of_the_normalisation(d, eps):
    from miccai2021_cataract_semantic_segmentation_amd import ops
    n_pix, A, tau, gval = 75, 20, 0.5, 1.3
    f, fd = _features(n_pix, d, 40 + d)
    if eps > 1:                                                # rows on both sides of the clamp
        f[::2] *= 0.05
        fd[::2] *= 0.05
    rng = np.random.default_rng(100 + d)
    idx = rng.permutation(n_pix)[:A]
    idx[[2, 9]] = -1
    di = torch.from_numpy(idx.astype(np.int32)).to(DEV)
    dp = (d + 3) // 4 * 4
    Z, inv = ops.contrast_gather(fd.view(1, 1, n_pix, d), di, eps)
    assert eps < 1 or (bool((inv < 0).any()) and bool((inv > 0).any()))
    dZ = torch.randn(A, dp, generator=torch.Generator().manual_seed(d))
    g = torch.tensor([gval], device=DEV)
    ops.contrast_scatter_bwd(dZ.to(DEV), Z, inv, di, d, g, 1.0 / tau, (1, 1, n_pix, d))      # (the wrapper allocates a dense buffer)
    # ... and once more into a guarded buffer, through the library, to see what is written around it
    from miccai2021_cataract_semantic_segmentation_amd._lib import check, lib, ptr, stream
    obuf, out = _guarded(n_pix, d)
    dZd = dZ.to(DEV)
    check(lib.catseg_contrast_scatter_bwd(ptr(dZd), ptr(Z), dp, ptr(inv), ptr(di), A, d, ptr(g), 1.0 / tau, ptr(out), n_pix, stream()))
    assert _guards_intact(obuf, n_pix * d)
    filled = idx >= 0

    def ref(dt):
        x = f.to(dt).clone().requires_grad_()
        z = torch.nn.functional.normalize(x[torch.from_numpy(idx[filled])], dim=1, eps=eps)
        v = dZ[torch.from_numpy(filled), :d].to(dt) * torch.tensor(gval, dtype=torch.float32).to(dt) * (1.0 / tau)
        (z * v).sum().backward()
        return x.grad
    within("contrast_scatter_bwd", "d=%d eps=%g" % (d, eps), out, ref(torch.float64), ref(torch.float32))
    others = np.setdiff1d(np.arange(n_pix), idx[filled])
    assert bool((out.cpu()[torch.from_numpy(others)] == 0).all())


# ---------------------------------------------------------------------------------------------------------------- rows, finalize, end to end
def _labels(A, K, kind, rng):
    if kind == "single":                                       # one filled slot only
        lab = np.full(A, -1)
        lab[A // 2] = 1
        return lab
    if kind == "one_class":
        lab = np.full(A, 2)
        lab[rng.random(A) < 0.3] = -1
        lab[:2] = 2
        return lab
    lab = rng.integers(1, K - 1, A)                            # class K - 1 is absent
    lab[rng.random(A) < 0.15] = -1                             # empty slots
    lab[0] = 0                                                 # class 0 has ONE anchor: no positive
    lab[1], lab[A - 1] = 1, 1
    return lab


def _run(feat, idx, lab, Wt, tau, eps, g=1.0):
    """the launches of losses/contrast.py on given slots -> (loss, dfeat, G, Z)"""
    from miccai2021_cataract_semantic_segmentation_amd import ops
    n_pix, d = feat.shape
    A = len(idx)
    di, dl = (torch.from_numpy(np.asarray(v).astype(np.int32)).to(DEV) for v in (idx, lab))
    filled = np.asarray(lab) >= 0
    nc = np.bincount(np.asarray(lab)[filled], minlength=1)
    n_pos = torch.tensor([int(nc[nc >= 2].sum())], dtype=torch.int32, device=DEV)
    Z, inv = ops.contrast_gather(feat.view(1, 1, n_pix, d), di, eps)
    dp = Z.shape[1]
    lds = ops.r4(A)
    sbuf, S = _guarded(A, lds)
    ops.gemm(ops.NT, 1, A, A, dp, Z, dp, 0, Z, dp, 0, S, lds, 0)
    ell = ops.contrast_rows(S, A, dl, Wt, 1.0 / tau, n_pos)
    loss = ops.contrast_finalize(ell, n_pos)
    assert _guards_intact(sbuf, A * lds)
    dZ = torch.empty_like(Z)
    ops.gemm(ops.NN, 1, A, d, A, S, lds, 0, Z, dp, 0, dZ, dp, 0, zero_to=dp)
    ops.gemm(ops.TN, 1, A, d, A, S, lds, 0, Z, dp, 0, dZ, dp, 0, zero_to=dp, accumulate=True)
    df = ops.contrast_scatter_bwd(dZ, Z, inv, di, d, torch.tensor([g], device=DEV), 1.0 / tau, (1, 1, n_pix, d))
    return loss, df.view(n_pix, d), S, Z


def _reference(feat, idx, lab, Wt, tau, eps, dt, g=1.0):
    x = feat.cpu().to(dt).clone().requires_grad_()
    loss = CR.loss_torch(x, idx, lab, Wt.cpu().to(dt), tau, eps)
    (loss * g).backward()
    return loss.detach().reshape(1), x.grad


@pytest.mark.parametrize("A,kind,tau,lam", [(4, "mixed", 0.5, 0.0), (8, "mixed", 0.07, 0.7), (8, "single", 0.5, 0.0), (68, "one_class", 0.07, 0.0),
                                            (68, "mixed", 0.5, 0.7), (260, "mixed", 0.07, 0.7), (1028, "mixed", 0.5, 0.0), (1028, "mixed", 0.07, 0.7),
                                            (4100, "mixed", 0.07, 0.7)])
def test_loss_end_to_end_from_given_slots(A, kind, tau, lam):
    K, d = 6, 6
    rng = np.random.default_rng(A + int(100 * tau))
    lab = _labels(A, K, kind, rng)
    n_pix = A + 9
    feat = torch.randn(n_pix, d, generator=torch.Generator().manual_seed(A))
    idx = np.where(lab >= 0, rng.permutation(n_pix)[:A], -1)
    if kind == "mixed" and A >= 8:                             # two identical embeddings among the positives: s = 1 / tau
        feat[idx[A - 1]] = feat[idx[1]]
    m = torch.from_numpy(rng.random((K, K))).float()
    Wt = CR.table(m / m.sum(0, keepdim=True), lam).contiguous()
    assert lam == 0 or not torch.equal(Wt, Wt.t())
    fd, Wd = feat.to(DEV), Wt.to(DEV)
    loss, df, G, Z = _run(fd, idx, lab, Wd, tau, 1e-12, g=0.5)
    l64, g64 = _reference(feat, idx, lab, Wt, tau, 1e-12, torch.float64, g=0.5)
    l32, g32 = _reference(feat, idx, lab, Wt, tau, 1e-12, torch.float32, g=0.5)
    case = "A=%d %s tau=%g lam=%g" % (A, kind, tau, lam)
    within("contrast_loss", case, loss, l64, l32)
    within("contrast_df", case, df, g64, g32)
    if kind == "single":
        assert float(loss) == 0.0 and bool((df == 0).all())
    # the diagonal, the pad columns, empty rows and empty columns of G are +0 (all bits clear)
    Gb = G.view(torch.int32).cpu()
    empty = torch.from_numpy(lab < 0)
    assert bool((Gb.diagonal() == 0).all()) and bool((Gb[:, A:] == 0).all()) and bool((Gb[empty] == 0).all()) and bool((Gb[:A, :A][:, empty] == 0).all())
    assert bool((Gb[0] == 0).all()) or kind != "mixed"         # the class with one anchor: no positive, the row takes no part
    loss2, df2, G2, _ = _run(fd, idx, lab, Wd, tau, 1e-12, g=0.5)
    assert torch.equal(loss, loss2) and torch.equal(df, df2) and torch.equal(G.view(torch.int32), G2.view(torch.int32))


def test_worst_ratios_are_reported():
    """(runs last in this file: prints what the README row quotes)"""
    for k in ("contrast_gather", "contrast_scatter_bwd", "contrast_loss", "contrast_df"):
        if k in WORST:
            print("WORST %-22s ratio %.3f  (%s)" % (k, WORST[k][0], WORST[k][1]))
