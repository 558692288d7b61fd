"""CPU-side checks of the egress: the palette / network-id tables and the numpy forms of the reference-named functions against the REAL
reference's fixture (tests/golden/egress.npz), the restatement the GPU tests use against the same fixture, the binding's prototype and the
argument checks of catseg_egress_u8 before any launch."""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _egress_ref as GR  # noqa: E402

from miccai2021_cataract_semantic_segmentation_amd import utils as U  # noqa: E402
from miccai2021_cataract_semantic_segmentation_amd.utils.classes import CLASS_REMAP, NUM_CLASSES  # noqa: E402


def test_fixture_records_its_conditions(golden):
    g = golden("egress")
    for e in (1, 2, 3):
        assert float(g["e%d_margin" % e]) >= 1e-3
        assert int(g["e%d_excluded" % e]) <= 0.01 * g["e%d_pred" % e].size
        assert g["e%d_logits" % e].shape == (2, NUM_CLASSES[e], 12, 20)
        half = g["e%d_img" % e][:, :, 0] * np.float32(255)
        assert np.all(half - np.floor(half) == 0.5)                   # the rounding ties are there
    assert float(g["band"]) == np.float32(GR.BAND)


@pytest.mark.parametrize("e", [1, 2, 3])
def test_tables_equal_the_reference(golden, e):
    g = golden("egress")
    assert np.array_equal(U.get_cadis_colormap(), g["cadis_colormap"]) and U.get_cadis_colormap().shape == (36, 3)
    assert len(U.CADIS_PALETTE) == 36
    cmap = U.get_remapped_colormap(CLASS_REMAP[e])
    assert list(cmap.keys()) == list(g["e%d_cmap_keys" % e])
    assert np.array_equal(np.array([np.asarray(c) for c in cmap.values()], dtype=np.uint8), g["e%d_cmap_colours" % e])
    lut, pal = GR.tables(golden, e)
    assert np.array_equal(U.network_lut(e), lut)
    assert np.array_equal(U.mask_from_network(np.arange(256), e).astype(np.uint8), lut)
    assert np.array_equal(U.palette_table(cmap), pal) and np.array_equal(U.palette_table(cmap, bgr=True), pal[:, ::-1])


@pytest.mark.parametrize("e", [1, 2, 3])
def test_numpy_forms_equal_the_reference_bytes(golden, e):
    g = golden("egress")
    img, tgt, pred, comb = g["e%d_img" % e], g["e%d_target" % e].astype(np.int64), g["e%d_pred" % e].astype(np.int64), g["e%d_comb" % e]
    W = img.shape[-1]
    cmap = U.get_remapped_colormap(CLASS_REMAP[e])
    for b in range(2):
        got = U.to_comb_image(torch.from_numpy(img[b]), torch.from_numpy(tgt[b].copy()), torch.from_numpy(pred[b].copy()), e)
        assert got.dtype == np.uint8 and np.array_equal(got, comb[b])
        assert np.array_equal(U.mask_to_colormap(tgt[b].copy(), cmap, from_network=True, experiment=e), comb[b][:, W:2 * W])
        assert np.array_equal(U.mask_to_colormap(pred[b].copy(), cmap, from_network=True, experiment=e), comb[b][:, 2 * W:])
        m = tgt[b].copy()
        assert U.mask_from_network(m, e) is m and np.array_equal(m.astype(np.uint8), g["e%d_lut" % e][tgt[b]])
    sm = torch.softmax(torch.from_numpy(g["e%d_logits" % e]), 1)
    for t in (0.5, 0.9):
        ign = NUM_CLASSES[e]
        got = U.clipped_argmax(sm, t, ign)
        keep = ~g["e%d_band_%d" % (e, round(t * 100))]
        assert got.dtype == torch.int64 and np.array_equal(got.numpy()[keep], g["e%d_clipped_%d" % (e, round(t * 100))].astype(np.int64)[keep])
    with pytest.raises(AssertionError):
        U.clipped_argmax(sm, 1.0, 17)


@pytest.mark.parametrize("e", [1, 2, 3])
def test_restatement_reproduces_the_reference_fixture(golden, e):
    g = golden("egress")
    lut, pal = GR.tables(golden, e)
    rows = np.ascontiguousarray(np.moveaxis(g["e%d_logits" % e], 1, -1))
    tgt = g["e%d_target" % e].astype(np.int64)
    r = GR.egress(rows, lut=lut, palette=pal, frame=g["e%d_img" % e], target=tgt)
    assert np.array_equal(r["canvas"], g["e%d_comb" % e]) and np.array_equal(r["labels"], g["e%d_pred" % e])
    r = GR.egress(rows, lut=lut, palette=pal, frame=g["e%d_img_norm" % e], mean=g["mean"], std=g["std"])
    assert np.array_equal(r["canvas"][:, :, :20], g["e%d_img_norm_u8" % e])
    for t in (0.5, 0.9):
        r = GR.egress(rows, threshold=t, ignore_value=NUM_CLASSES[e], lut=lut)
        keep = ~(g["e%d_band_%d" % (e, round(t * 100))] | r["band"])
        assert np.array_equal(r["labels"][keep], g["e%d_clipped_%d" % (e, round(t * 100))][keep])
        assert np.array_equal(r["labels_u8"][keep], g["e%d_clipped_u8_%d" % (e, round(t * 100))][keep])
        assert (r["labels"] == NUM_CLASSES[e]).any() and (r["labels"] != NUM_CLASSES[e]).any()


def test_prototype_and_argument_checks_without_gpu():
    from miccai2021_cataract_semantic_segmentation_amd import _lib, ops
    lib = _lib.lib
    assert "catseg_egress_u8" in _lib.EXPORTS and callable(ops.egress_u8)
    assert len(lib.catseg_egress_u8.argtypes) == 23

    def call(K=25, ld=28, H=12, crop=(2, 2), threshold=0.0, ignore=25, palette=16, frame=None, mean=None, std=None, target=None, rows=16,
             li=16, lu=16, canvas=16):
        return lib.catseg_egress_u8(rows, ld, 2, H, 20, K, 0, crop[0], crop[1], threshold, ignore, 16, palette, frame, 0, mean, std, 0, target,
                                    li, lu, canvas, None)

    three = (ctypes.c_float * 3)(0.5, 0.5, 0.5)
    for kw, msg in ((dict(K=0), b"K <= 64"), (dict(K=65, ld=68), b"K <= 64"), (dict(ld=24), b"ld 24 < K"), (dict(crop=(6, 6)), b"crop"),
                    (dict(crop=(12, 0)), b"crop"), (dict(crop=(-1, 0)), b"crop"), (dict(li=None, lu=None, canvas=None), b"all outputs"),
                    (dict(palette=None), b"palette"), (dict(threshold=1.0), b"threshold"), (dict(threshold=1.5), b"threshold"),
                    (dict(threshold=float("nan")), b"threshold"), (dict(threshold=0.5, ignore=256), b"ignore_value"),
                    (dict(canvas=None, frame=16), b"need a canvas"), (dict(frame=16, mean=three), b"mean and std"),
                    (dict(mean=three, std=three), b"mean and std"), (dict(rows=None), b"without rows")):
        assert call(**kw) == 1, kw                                    # CATSEG_EINVAL, nothing launched
        assert msg in lib.catseg_last_error(), (kw, lib.catseg_last_error())
