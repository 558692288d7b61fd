"""The numpy restatement of the Dropout2d mask generator (tests/_dropout_ref.py, which tests/test_dropout_gpu.py holds the HIP kernel to bit for
bit): Philox4x32-10 against the Random123 known answers, and the conditions the chosen seed has to meet."""
import os

import numpy as np
import pytest

import _dropout_ref as R

KAT = [((0, 0, 0, 0), (0, 0), (0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8)),
       ((0xffffffff,) * 4, (0xffffffff,) * 2, (0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd)),
       ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0), (0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1))]


@pytest.mark.parametrize("ctr,key,want", KAT)
def test_philox_known_answers(ctr, key, want):
    got = R.philox4x32_10([np.uint64(c) for c in ctr], key)
    assert tuple(int(v) for v in got) == want, [hex(int(v)) for v in got]


def test_mask_layout():
    """element i takes word i & 3 of the block i >> 2; the bits and the multipliers say the same; p = 1 drops everything without a division"""
    B, C, p = 3, 64, 0.3
    kept, mult, bits = R.mask(1234, 1, 2, 5, p, B, C)
    for i in (0, 1, 7, 66, B * C - 1):
        w = R.philox4x32_10([np.uint64(i >> 2), np.uint64(5), np.uint64(0), np.uint64(1 | 2 << 16)], (1234, 0))[i & 3]
        u = np.float32(int(w) >> 8) * np.float32(2.0 ** -24)
        assert bool(kept.reshape(-1)[i]) == bool(u >= np.float32(p))
    assert set(np.unique(mult)) <= {np.float32(0), np.float32(1) / (np.float32(1) - np.float32(p))}
    unpacked = (bits[:, :, None] >> np.arange(32, dtype=np.uint32)) & 1
    assert np.array_equal(unpacked.reshape(B, C).astype(bool), kept)
    kept1, mult1, bits1 = R.mask(1234, 0, 0, 0, 1.0, B, C)
    assert not kept1.any() and not mult1.any() and not bits1.any() and np.isfinite(mult1).all()
    assert R.mask(1234, 0, 0, 0, 0.5, 3, 6)[2] is None           # (18 elements: no packed bits)


@pytest.mark.parametrize("p", [0.1, 0.3, 0.5])
def test_seed_1234_conditions(p):
    """64 draws of 8 x 512 on two layers: keep fraction within 4 sigma of the binomial, |correlation| <= 0.01 between the layers and between
    consecutive draws, no image with every channel dropped"""
    B, C, N = 8, 512, 64
    k = np.stack([[R.mask(1234, layer, 0, d, p, B, C)[0] for d in range(N)] for layer in (0, 1)]).astype(np.float64)   # [2, N, B, C]
    n = k[0].size
    sigma = (p * (1 - p) / n) ** 0.5
    for layer in (0, 1):
        assert abs(k[layer].mean() - (1 - p)) <= 4 * sigma, (layer, k[layer].mean())
        assert k[layer].reshape(N * B, C).sum(1).min() > 0
    corr = lambda a, b: float(np.corrcoef(a.reshape(-1), b.reshape(-1))[0, 1])
    assert abs(corr(k[0], k[1])) <= 0.01
    for layer in (0, 1):
        assert abs(corr(k[layer][:-1], k[layer][1:])) <= 0.01


def test_reference_fixture():
    """tests/golden/dropout.npz (the reference's modules in train mode, masks recorded by hooks on their nn.Dropout2d): the fp64 evaluation
    of the restatement with the recorded masks reproduces the reference's logits and gradients.  Bar: the reference computes in fp32; its
    longest sums run over 128 channels or 120 pixels, so n eps = 128 x 6e-8 = 8e-6 of the largest value bounds its error, and 2e-5 leaves 2.5 x"""
    import torch
    path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "dropout.npz")
    g = np.load(path)
    for tag in ("ocr", "interm"):
        y = torch.from_numpy(g[tag + "_y"]).double()                     # [B, C, H, W]: the convolution's output
        B, C, H, W = y.shape
        rows = y.permute(0, 2, 3, 1).reshape(-1, C)
        mean, var = rows.mean(0), rows.var(0, unbiased=False)
        inv = (var + 1e-5).rsqrt()
        gamma, beta = torch.from_numpy(g[tag + "_gamma"]).double(), torch.from_numpy(g[tag + "_beta"]).double()
        wh, bh = torch.from_numpy(g[tag + "_wh"]).double(), torch.from_numpy(g[tag + "_bh"]).double()
        K = wh.shape[0]
        dl = torch.from_numpy(g[tag + "_dlogits"]).double().permute(0, 2, 3, 1).reshape(-1, K)
        mult = g[tag + "_mult"]
        assert set(np.unique(mult)) <= {np.float32(0), R.keep_of(float(g[tag + "_p"]))}
        r = R.head_fp64(rows, mean, inv, gamma, beta, gamma * inv, wh.reshape(K, C), bh, mult, dl, H * W)
        ref = torch.from_numpy(g[tag + "_logits"]).double().permute(0, 2, 3, 1).reshape(-1, K)
        tol = lambda t: 2e-5 * float(t.abs().max())
        assert float((r["logits"] - ref).abs().max()) <= tol(ref)
        for name, got in (("dwh", r["dwh"]), ("dbh", r["dbh"]), ("dgamma", r["dgamma"]), ("dbeta", r["dbeta"])):
            want = torch.from_numpy(g[tag + "_" + name]).double().reshape(got.shape)
            assert float((got - want).abs().max()) <= tol(want), name
        dy = torch.from_numpy(g[tag + "_dy"]).double().permute(0, 2, 3, 1).reshape(-1, C)
        assert float((r["dy"] - dy).abs().max()) <= tol(dy)


def test_layer_state_and_rank_seeding():
    """engine.Dropout2d: no state-dict key, state = {seed lo, seed hi, layer | rank << 16, 0}; dist.seed_dropout_by_rank gives every rank its
    own Philox counter word, for layers seeded before and after the call"""
    import torch
    from torch import nn
    from miccai2021_cataract_semantic_segmentation_amd import dist as D
    from miccai2021_cataract_semantic_segmentation_amd.engine import Dropout2d, dropout_layers
    net = nn.Sequential(Dropout2d(0.3, layer=0), Dropout2d(0.3, layer=1))
    assert list(net.state_dict()) == [] and len(list(net.buffers())) == 2 and len(list(net.parameters())) == 0
    seed = 0xFEDCBA9876543210
    net[0].reseed(seed)
    D.seed_dropout_by_rank(net, 3)
    torch.manual_seed(seed)
    net[1].ensure_seeded()
    for d in dropout_layers(net):
        words = [int(v) & 0xFFFFFFFF for v in d.state.tolist()]
        assert words == [seed & 0xFFFFFFFF, seed >> 32, d.layer | 3 << 16, 0]
    with pytest.raises(ValueError):
        Dropout2d(1.5)
