"""Host side of the frequency-weighted crop (CropNP, crop_mode 'freq'): the exact integer pick against the offsets the REAL reference
reported (tests/golden/cropfreq.npz, written by tests/golden/make_golden_cropfreq.py), the region arithmetic, the integer weight table, the
opt-in, and the C ABI of include/catseg_cropfreq.h (prototypes against _lib._SIGS, every refusal before a launch)."""
import functools
import os
import random
from fractions import Fraction

import numpy as np
import pytest

import _abi
import _cropfreq_ref as CR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BAND = 2.0 ** -22          # the derived 2^-23 (float32 normalisation of the reference's weights) x 2: DESIGN.md


@functools.lru_cache(maxsize=None)
def _fixture():
    return np.load(os.path.join(ROOT, "tests", "golden", "cropfreq.npz"))


def test_integer_pick_equals_the_reference_on_every_fixture_case():
    """offsets, window edge and draw count of the reference's CropNP('freq'); a condition, not a tolerance: NO case may be set aside for
    lying in the band"""
    from miccai2021_cataract_semantic_segmentation_amd.utils.geometry import (crop_px, freq_m53, freq_weight_table, sample_freq_u)
    g = _fixture()
    cases = g["cases"]
    assert len(cases) >= 40 and float(g["band"]) == BAND
    assert (g["distance"] > BAND).all(), "a fixture case lies in the band: the maker must not have stored it"
    shapes = set()
    for ci, (exp, mi, seed, px, v, h) in enumerate(cases.tolist()):
        lbl = g["map%d" % mi]
        shapes.add(lbl.shape)
        wq, _ = freq_weight_table(g["class_frequencies_e%d" % exp])
        rng = random.Random(seed)
        u = sample_freq_u(1, rng)
        assert u[0] == g["u"][ci] and rng.random() == g["next_random"][ci], "one random() per frame, as random.choices(k=1)"
        assert crop_px(float(g["size"]), *lbl.shape) == px
        got = CR.integer_pick(lbl, px, wq, freq_m53(u)[0])
        assert got[:2] == (v, h), (ci, got, (v, h))
    assert shapes == {(96, 160), (80, 72), (192, 320)} and set(cases[:, 0].tolist()) == {1, 2}


def test_region_arithmetic():
    from miccai2021_cataract_semantic_segmentation_amd.utils.geometry import crop_freq_region, crop_px
    assert crop_freq_region(96, 160, 32) == (16, 64, 64)             # W > H: the columns are sliced with the height (img_h quirk)
    assert crop_freq_region(80, 72, 32) == (16, 48, 48)
    assert crop_freq_region(80, 40, 32) == (16, 48, 24)              # W < H - margin: numpy clips the column slice at W
    assert crop_px(0.4, 540, 960) == 192 and crop_freq_region(540, 960, 192) == (96, 348, 348)
    assert crop_px(0.4, 1080, 1920) == 416 and crop_freq_region(1080, 1920, 416) == (208, 664, 664)
    assert crop_freq_region(64, 64, 64) == (32, 0, 0)              # a window as tall as the canvas: nothing to pick from
    for h, w, px in ((96, 160, 32), (80, 72, 32), (80, 40, 32), (33, 47, 33)):
        margin, rh, rw = crop_freq_region(h, w, px)
        assert np.zeros((h, w))[margin:h - margin, margin:h - margin].shape == (rh, rw) == CR.region(h, w, px)[1:]


def test_class_table_is_the_reference_s():
    from miccai2021_cataract_semantic_segmentation_amd.utils.geometry import class_frequencies
    g = _fixture()
    for exp in (1, 2):
        f = class_frequencies(g["class_sums"], exp)
        assert f.dtype == np.float32 and np.array_equal(f, g["class_frequencies_e%d" % exp])
    f3 = class_frequencies(g["class_sums"], 3)        # unpinned: the reference raises KeyError(25) for experiment 3; the evident intent
    sums = g["class_sums"].astype(np.float64)
    assert f3.shape == (26,) and np.allclose(f3[:25], sums[:25] / sums.sum(), rtol=1e-6) and np.isclose(f3[25], sums[25:].sum() / sums.sum(), rtol=1e-6)


def test_weight_table_is_exact_and_large_sums_are_refused():
    from miccai2021_cataract_semantic_segmentation_amd.utils.geometry import check_freq_weights, freq_weight_table
    g = _fixture()
    for freqs in (g["class_frequencies_e1"], g["class_frequencies_e2"], np.array([0.5, 0.25, 0.25], dtype=np.float32)):
        wq, s = freq_weight_table(freqs)
        w = np.float32(1) / np.asarray(freqs, dtype=np.float32)
        assert all(isinstance(q, int) for q in wq) and [Fraction(q) / s for q in wq] == [Fraction(float(x)) for x in w]
        assert any(q % 2 for q in wq), "s is the SMALLEST power of two"
        assert (wq, s) == CR.weights_of(freqs)
        check_freq_weights(wq, 664 * 664)
    assert freq_weight_table(np.array([0.5, 0.25, 0.25], dtype=np.float32)) == ([1, 2, 2], Fraction(1, 2))
    with pytest.raises(ValueError, match="2\\^62"):
        check_freq_weights([1 << 44], 1 << 18)
    check_freq_weights([(1 << 44) - 1], 1 << 18)
    for bad in ([0.0, 1.0], [-0.5, 1.5], [], [np.nan, 1.0]):
        with pytest.raises(ValueError):
            freq_weight_table(np.array(bad, dtype=np.float32))


def test_freq_is_opt_in():
    from miccai2021_cataract_semantic_segmentation_amd.utils.geometry import check_crop, geometry_from_transforms
    g = _fixture()
    with pytest.raises(NotImplementedError, match="freq.*crop_freq_on_device"):
        geometry_from_transforms(["crop"], {"crop_size": 0.4, "crop_mode": "freq"})
    with pytest.raises(NotImplementedError, match="freq"):
        check_crop({"size": 0.4, "mode": "freq", "class_frequencies": g["class_frequencies_e2"]})
    with pytest.raises(ValueError, match="class table"):
        geometry_from_transforms(["crop"], {"crop_size": 0.4, "crop_mode": "freq", "crop_freq_on_device": True})
    geo = geometry_from_transforms(["pad", "crop"], {"crop_size": 0.4, "crop_mode": "freq", "crop_freq_on_device": True, "experiment": 2,
                                                     "class_sums": g["class_sums"].tolist()})
    assert geo["crop"]["mode"] == "freq" and geo["crop"]["on_device"] is True and geo["pad"] == (0, 0)
    assert np.array_equal(geo["crop"]["class_frequencies"], g["class_frequencies_e2"])
    geo = geometry_from_transforms(["crop"], {"crop_size": 0.4, "crop_mode": "freq", "crop_freq_on_device": True,
                                              "class_frequencies": g["class_frequencies_e1"]})
    assert geo["crop"]["class_frequencies"] is not None
    with pytest.raises(ValueError, match="not recognised"):
        check_crop({"mode": "centre", "on_device": True})


# ---- the C ABI of include/catseg_cropfreq.h
def test_ext_signature_table_matches_the_header():
    """the header declares the crop pick's two entry points; each has the header's signature in _lib._SIGS and is exported"""
    from miccai2021_cataract_semantic_segmentation_amd import _lib
    protos = _abi.prototypes("catseg_cropfreq.h")
    assert sorted(protos) == ["catseg_crop_freq_pick", "catseg_crop_freq_workspace"]
    for name, (res, args, _) in protos.items():
        assert _lib._SIGS[name] == (res, args), "%s: header %r, _lib._SIGS %r" % (name, (res, args), _lib._SIGS[name])
        assert hasattr(_lib.lib, name)


EINVAL, EWORKSPACE = 1, 3
A = [0x10000 * (i + 1) for i in range(12)]     # fake device pointers: a refusal returns before anything is launched


def _pick_args(**kw):
    """arguments of catseg_crop_freq_pick that are valid (a 48 x 80 frame on its 96 x 160 canvas, px 32) but for kw"""
    f = dict(lbl=A[0], B=2, H=48, W=80, lut=A[1], flips=A[2], minv=A[3], Hc=96, Wc=160, px=32, wq=A[4], m53=A[5], origin=A[6], total=A[7],
             flat=A[8], workspace=A[9], workspace_bytes=2 * 64 * 8, stream=None)
    f.update(kw)
    return tuple(f.values())


PICK_DEFECTS = [
    ("an empty region", dict(Hc=64, Wc=64, px=64, minv=A[3]), b"empty region"),
    ("px wider than the canvas", dict(Hc=96, Wc=24, px=32), b"px outside the canvas"),
    ("px taller than the canvas", dict(px=128), b"px outside the canvas"),
    ("px = 0", dict(px=0), b"px outside the canvas"),
    ("a NULL table", dict(wq=None), b"weight table is NULL"),
    ("a NULL label map", dict(lbl=None), b"label map is NULL"),
    ("no origin", dict(origin=None), b"origin are required"),
    ("no m53", dict(m53=None), b"origin are required"),
    ("no matrix, canvas != frame", dict(minv=None), b"without a matrix"),
    ("a misaligned table", dict(wq=A[4] + 4), b"alignment"),
    ("B = 0", dict(B=0), b"bad dims"),
    ("a frame beyond the limit", dict(H=20000), b"16384"),
]


@pytest.mark.parametrize("what,fields,message", PICK_DEFECTS, ids=[c[0] for c in PICK_DEFECTS])
def test_crop_freq_pick_rejects_one_defect(what, fields, message):
    from miccai2021_cataract_semantic_segmentation_amd import _lib
    rc = _lib.lib.catseg_crop_freq_pick(*_pick_args(**fields))
    err = _lib.lib.catseg_last_error()
    assert rc == EINVAL and err.startswith(b"catseg_crop_freq_pick:") and message in err, (what, rc, err)


def test_crop_freq_workspace_query_and_too_small_workspace():
    from miccai2021_cataract_semantic_segmentation_amd import _lib
    lib = _lib.lib
    assert lib.catseg_crop_freq_workspace(2, 96, 160, 32) == 2 * 64 * 8
    assert lib.catseg_crop_freq_workspace(8, 1080, 1920, 416) == 8 * 664 * 8
    assert lib.catseg_crop_freq_workspace(2, 64, 64, 64) == 0 and lib.catseg_crop_freq_workspace(2, 96, 160, 128) == 0
    assert lib.catseg_crop_freq_workspace(0, 96, 160, 32) == 0
    for fields in (dict(workspace_bytes=2 * 64 * 8 - 1), dict(workspace=None), dict(workspace=A[9] + 4)):
        rc = lib.catseg_crop_freq_pick(*_pick_args(**fields))
        err = lib.catseg_last_error()
        assert rc == EWORKSPACE and err.startswith(b"catseg_crop_freq_pick:") and b"workspace too small" in err, (fields, rc, err)
