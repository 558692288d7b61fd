"""PointRend training without a GPU: the opt-in surface (the build-side key config['decoder']['pr_train_on_device']), the restatement's
pieces against torch's own operations, the coordinate stream of the device generator against the numpy Philox of tests/_dropout_ref.py, and
the argument validation of the new entry points (fake pointers: a refusal returns before any launch)."""
import ctypes
import os
import re
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _dropout_ref as DR  # noqa: E402
import _pointrend_ref as PR  # noqa: E402
import _pointrend_train_ref as TR  # noqa: E402

PINNED = "train-mode forward.*get_uncertain_point_coords_with_randomness.*point cross-entropy loss.*backward of the point gather"


def _config(on):
    cfg = PR.model_config(96)
    cfg["decoder"].update(pr_train_num_pts=48)
    if on:
        cfg["decoder"]["pr_train_on_device"] = True
    return cfg


# ------------------------------------------------------------------------------------------------------------ the opt-in surface
def test_the_refusal_names_the_key_and_the_generator_and_keeps_its_pinned_form():
    from miccai2021_cataract_semantic_segmentation_amd.models.EncDec import POINTREND_TRAINING_REFUSAL as msg
    assert re.search(PINNED, msg) and "pr_train_on_device" in msg and "torch.rand" in msg and "device generator" in msg
    assert "missing" not in msg and "\n" not in msg


def test_without_the_key_both_refusals_stand_and_with_it_the_device_check_is_reached(tmp_path):
    from miccai2021_cataract_semantic_segmentation_amd import engine
    from miccai2021_cataract_semantic_segmentation_amd.managers import EncDecManager
    from miccai2021_cataract_semantic_segmentation_amd.models import EncDec
    from miccai2021_cataract_semantic_segmentation_amd.models.EncDec import POINTREND_TRAINING_REFUSAL
    manager_cfg = lambda on: dict(_config(on), mode="training", manager="EncDec", data={"experiment": 2, "batch_size": 2}, log_path=str(tmp_path),
                                  loss={"losses": {"CrossEntropyLoss": 1}}, train={"learning_rate": 1e-4, "epochs": 1})
    off = EncDec(_config(False), 2)
    assert off.training and not off.dec_model.train_on_device
    with pytest.raises(NotImplementedError, match=PINNED):
        off(torch.zeros(1, 3, 64, 64))
    with pytest.raises(NotImplementedError) as e:
        EncDecManager(manager_cfg(False))
    assert str(e.value) == POINTREND_TRAINING_REFUSAL and not os.listdir(str(tmp_path))
    on = EncDec(_config(True), 2)
    assert on.dec_model.train_on_device and isinstance(on.dec_model.sampler, engine.PointSampler)
    with pytest.raises(RuntimeError, match="no CPU fallback"):          # past the refusal, to the engine's device check
        on(torch.zeros(1, 3, 64, 64))
    if not torch.cuda.is_available():
        with pytest.raises(RuntimeError, match="no CPU fallback"):      # ... and so is the training manager
            EncDecManager(manager_cfg(True))
    # the key changes no state-dict key, and the sampler's 16 bytes are not in the state dict
    assert list(on.state_dict().keys()) == list(off.state_dict().keys())
    assert [n for n, _ in on.named_buffers() if n.endswith("sampler.state")] == ["dec_model.sampler.state"]


def test_the_sampler_state_is_seeded_like_a_dropout_layer():
    from miccai2021_cataract_semantic_segmentation_amd import engine
    s, d = engine.PointSampler(layer=3), engine.Dropout2d(0.5, layer=3)
    s.reseed(0xFEDCBA9876543210, rank=2)
    d.reseed(0xFEDCBA9876543210, rank=2)
    assert s.state.tolist() == d.state.tolist() and s.state.tolist()[2] == 3 | 2 << 16 and s.state.tolist()[3] == 0
    assert s.draws() and d.draws()
    s.fixed_points = torch.zeros(1, 4, 2)
    assert not s.draws()
    model = torch.nn.Sequential(s, d, torch.nn.ReLU())
    assert engine.rng_modules(model) == [s, d] and engine.dropout_layers(model) == [d]
    torch.manual_seed(41)
    fresh = engine.PointSampler()
    fresh.ensure_seeded()
    assert fresh.state.tolist()[:2] == [41, 0]


# ------------------------------------------------------------------------------------------------------------ the restatement's pieces
def test_the_coordinate_stream_is_the_numpy_philox_with_counter_word_two_set():
    seed, layer, rank, number, N, M = 0x0123456789ABCDEF, 5, 1, 9, 3, 7
    got = TR.draw(seed, layer, rank, number, N, M).numpy().reshape(-1)
    for i in (0, 1, 5, 17, N * M * 2 - 1):
        words = DR.philox4x32_10((i >> 2, number, 1, layer | rank << 16), (seed & 0xFFFFFFFF, seed >> 32))
        assert got[i] == np.float32(int(words[i & 3]) >> 8) * np.float32(2.0 ** -24)
    assert got.min() >= 0 and got.max() < 1 and got.dtype == np.float32
    # the Dropout2d masks are drawn with counter word 2 = 0: the two streams share no block
    kept, _, _ = DR.mask(seed, layer, rank, number, 0.5, 1, N * M * 2)
    assert not np.array_equal(kept.reshape(-1), got >= 0.5)
    assert not torch.equal(TR.draw(seed, layer, rank, number + 1, N, M), TR.draw(seed, layer, rank, number, N, M))


def test_pixel_index_rounds_half_to_even_and_labels_outside_the_map_are_class_zero():
    pts = torch.tensor([[[0.0, 0.0], [1.0 - 2.0 ** -24, 1.0 - 2.0 ** -24], [0.5, 0.5], [0.5 / 3, 2.5 / 3]]])
    assert TR.pixel_index(pts, 4, 4).tolist() == [[0, 15, 2 * 4 + 2, 2 * 4 + 0]]          # 1.5 -> 2, 0.5 -> 0, 2.5 -> 2
    lbl = torch.arange(1, 17).view(1, 4, 4)
    out = torch.tensor([[[0.5, 0.5], [0.999, 0.999], [1.2, 0.5], [-0.3, -0.3]]])
    assert TR.point_labels(lbl, out).tolist() == [[11, 16, 0, 0]]                          # (1.5, 1.5) -> (2, 2): label 11


def test_scatter_last_and_its_derivative_are_those_of_scatter_on_a_view():
    g = torch.Generator().manual_seed(0)
    coarse = torch.randn(2, 5, 4, 4, generator=g, dtype=torch.float64, requires_grad=True)
    vals = torch.randn(2, 5, 9, generator=g, dtype=torch.float64, requires_grad=True)
    pts = torch.rand(2, 9, 2, generator=g)
    pts[:, 3] = pts[:, 7] = pts[:, 1]
    pix = TR.pixel_index(pts, 16, 16)
    w = torch.randn(2, 5, 16, 16, generator=g, dtype=torch.float64)
    mine = TR._ScatterLast.apply(F.interpolate(coarse, scale_factor=4, mode="bilinear", align_corners=False), pix, vals)
    (mine * w).sum().backward()
    g_mine = (coarse.grad.clone(), vals.grad.clone())
    coarse.grad = vals.grad = None
    seg = F.interpolate(coarse, scale_factor=4, mode="bilinear", align_corners=False)
    ref = seg.reshape(2, 5, 256).scatter_(2, pix.unsqueeze(1).expand(-1, 5, -1), vals).view(2, 5, 16, 16)     # models/PointRend.py:72
    assert ref.data_ptr() == seg.data_ptr()                     # the reshape is a view: seg_logits and pred are one memory
    (ref * w).sum().backward()
    assert torch.equal(mine, ref) and torch.equal(g_mine[0], coarse.grad) and torch.equal(g_mine[1], vals.grad)
    assert torch.equal(vals.grad[:, :, 1], vals.grad[:, :, 7]) and torch.equal(mine.reshape(2, 5, 256)[0, :, pix[0, 1]], vals[0, :, 7])


def test_selection_takes_the_lower_candidate_among_equals_and_appends_the_rest():
    unc = torch.tensor([[-1.0, 0.0, -0.0, -1.0, -0.5]])
    cand = torch.arange(10.0).view(1, 5, 2)
    rest = torch.full((1, 2, 2), 9.0)
    coords, idx = TR.select_points(unc, cand, rest, 3)
    assert idx.tolist() == [[1, 2, 4]] and torch.equal(coords, torch.cat((cand[:, [1, 2, 4]], rest), 1))
    assert TR.counts(48, 3, 0.75) == (144, 36, 12) and TR.counts(2048, 3, 0.75) == (6144, 1536, 512)


# ------------------------------------------------------------------------------------------------------------ the ABI
def test_new_entry_points_validate_before_any_launch():
    from miccai2021_cataract_semantic_segmentation_amd import _lib
    lib, A = _lib.lib, [0x10000 * (i + 1) for i in range(10)]
    err = lambda: lib.catseg_last_error()
    assert lib.catseg_pointrend_draw(A[0] + 4, None, 2, 8, A[1], None) == 1 and b"16-byte aligned" in err()      # a misaligned state
    assert lib.catseg_pointrend_draw(None, None, 2, 8, A[1], None) == 1 and lib.catseg_pointrend_draw(A[0], None, 0, 8, A[1], None) == 1
    assert lib.catseg_pointrend_point_uncertainty(A[0], 4, 1, 4, 4, 1, A[1], 8, A[2], None) == 1 and b"K >= 2" in err()
    assert lib.catseg_pointrend_point_uncertainty(A[0], 16, 1, 4, 4, 17, A[1], 8, A[2], None) == 1 and b"ld" in err()
    # compose: more selected points than candidates, missing rest, a map too large for the reference's fp32 index arithmetic, labels without a map
    assert lib.catseg_pointrend_compose(A[0], 4, A[1], 5, A[2], 1, 8, 16, 16, None, 0, 0, A[3], A[4], None, None) == 1
    assert lib.catseg_pointrend_compose(A[0], 8, A[1], 5, None, 1, 8, 16, 16, None, 0, 0, A[3], A[4], None, None) == 1 and b"random points" in err()
    assert lib.catseg_pointrend_compose(A[0], 8, A[1], 5, A[2], 1, 8, 4096, 4096, None, 0, 0, A[3], A[4], None, None) == 1 and b"2^24" in err()
    assert lib.catseg_pointrend_compose(A[0], 8, A[1], 5, A[2], 1, 8, 16, 16, None, 0, 0, A[3], A[4], A[5], None) == 1
    d = _lib.PointrendGatherDesc()
    d.src[0], d.ld[0], d.H[0], d.W[0], d.C[0] = A[0], 16, 4, 4, 17                                      # rows narrower than the channels
    d.n_sources, d.N, d.k, d.out, d.ld_out = 1, 1, 4, A[2], 20
    assert lib.catseg_pointrend_gather_at(ctypes.byref(d), A[1], None) == 1 and b"source 0" in err()
    d.ld[0] = 20
    assert lib.catseg_pointrend_gather_at(ctypes.byref(d), None, None) == 1 and b"coordinates" in err()
    d.ld_out = 16
    assert lib.catseg_pointrend_gather_at(ctypes.byref(d), A[1], None) == 1 and b"point matrix" in err()
    b = _lib.PointrendGatherBwdDesc()
    b.dst[0], b.ld[0], b.H[0], b.W[0], b.C[0] = A[0], 17, 4, 4, 17                                      # a destination whose rows cannot take 16-byte stores
    b.n_sources, b.coords, b.N, b.P, b.dx, b.ld_dx = 1, A[1], 1, 4, A[2], 20
    assert lib.catseg_pointrend_gather_bwd(ctypes.byref(b), None) == 1 and b"destination 0" in err()
    b.ld[0], b.P = 20, 4000
    assert lib.catseg_pointrend_gather_bwd(ctypes.byref(b), None) == 1 and b"LDS" in err()            # the taps of an image must fit
    b.P, b.ld_dx = 4, 16
    assert lib.catseg_pointrend_gather_bwd(ctypes.byref(b), None) == 1 and b"dX" in err()
    b.ld_dx, b.n_sources = 20, 6
    assert lib.catseg_pointrend_gather_bwd(ctypes.byref(b), None) == 1
    assert lib.catseg_pointrend_scatter_last(A[0], 16, A[1], 1, 4, 64, A[2], 20, 17, None) == 1       # rows narrower than K
    assert lib.catseg_pointrend_scatter_last(A[0], 20, A[1], 1, 20000, 64, A[2], 20, 17, None) == 1 and b"LDS" in err()
    assert lib.catseg_pointrend_scatter_bwd(A[0], 16, A[1], 1, 4, 64, A[2], 20, 17, 0, None) == 1
    assert lib.catseg_pointrend_scatter_bwd(A[0], 20, A[1], 1, 4, 0, A[2], 20, 17, 0, None) == 1


# ------------------------------------------------------------------------------------------------------------ the reference's fixture
def test_restatement_reproduces_the_reference_train_fixture_bit_for_bit(golden):
    import json
    T = torch.from_numpy
    g = golden(TR.FIXTURE)
    spec = json.loads(str(g["spec"]))
    S = PR.fill_state(spec, int(g["seed"]))
    x, lbl, cand, rest, coords = T(g["x"]), T(g["lbl"]), T(g["cand0"]), T(g["rest0"]), T(g["coords0"])
    M, kb, R = TR.counts(TR.FIXTURE_P, TR.FIXTURE_RATIO, TR.FIXTURE_BETA)
    assert cand.shape == (2, M, 2) and rest.shape == (2, R, 2) and bool((lbl == 17).any())
    # the sampler: uncertainties, no tie at the k-th value, the reference's points in its order; the device's order holds the same points
    unc = TR.point_uncertainty(T(g["coarse"]), cand)
    assert torch.equal(unc, T(g["unc"]))
    kth, nxt = PR.kth_values(unc.unsqueeze(1), kb)
    assert bool((kth > nxt).all()) and np.array_equal(np.stack([kth.numpy(), nxt.numpy()]), g["kth"])
    band = TR.band(unc, kth, float(g["scale"])).sum(1) - 1                   # (the candidates other than the k-th itself)
    assert band.tolist() == g["band"].tolist() and int(band.max()) <= 0.05 * kb
    pts, idx = TR.select_points(unc, cand, rest, kb, ascending=False)
    assert torch.equal(pts, coords)
    mine, idx_dev = TR.select_points(unc, cand, rest, kb)
    assert torch.equal(torch.sort(idx, 1)[0], idx_dev) and torch.equal(mine[:, kb:], coords[:, kb:])
    # the network at those points: coarse logits, point logits, pred (stored at the scattered pixels; interpolate elsewhere), labels, losses
    _, coarse, pl, pred, pix = TR.network_forward(S, x, coords)
    assert torch.equal(coarse, T(g["coarse"])) and torch.equal(pl, T(g["point_logits"])) and torch.equal(pix, T(g["pix"]))
    assert int(g["max_points_per_pixel"]) >= 2 and max(int(torch.bincount(r).max()) for r in pix) == int(g["max_points_per_pixel"])
    assert torch.equal(pred, TR.fixture_pred(g))
    assert torch.equal(TR.point_labels(lbl, coords), T(g["point_labels"]))
    lc, lp = TR.manager_losses(pl, pred, lbl, coords)
    assert [float(lc), float(lp)] == g["losses"][0].tolist()
    assert abs(float(g["scale"]) - float(pred.abs().max())) == 0
