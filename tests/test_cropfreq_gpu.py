"""catseg_crop_freq_pick (csrc/cropfreq.hip: the window origins of CropNP's crop_mode 'freq', picked on the device from the warped labels)
against the exact integer restatement of tests/_cropfreq_ref.py, which tests/test_cropfreq_cpu.py holds to the reference's own offsets:
every comparison exact, no tolerance.  The labels the restatement weighs come from the dense float64 restatement of the warp
(tests/_warp_ref.py), not from the device."""
import functools
import os
import random

import numpy as np
import pytest
import torch

import _cropfreq_ref as CR
import _warp_ref as WR

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "cropfreq.npz")
M_LAST = (1 << 53) - 1


def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")


@functools.lru_cache(maxsize=None)
def _weights(exp):
    from miccai2021_cataract_semantic_segmentation_amd.utils.geometry import freq_weight_table
    return tuple(freq_weight_table(np.load(GOLDEN)["class_frequencies_e%d" % exp])[0])


def _mats48():
    """three frame -> canvas matrices for 48 x 80 frames on the 96 x 160 canvas: the reference's 'affine' draws for two frames, and a plain
    shift that leaves the frame in the canvas' upper half (region rows below it lie outside the frame: label 0)"""
    from miccai2021_cataract_semantic_segmentation_amd.utils.geometry import geometry_from_transforms, sample_affine
    params = geometry_from_transforms(["affine"])["affine"]
    mats = sample_affine(3, (48, 80), params, np.random.RandomState(5))[1]
    mats[2] = np.identity(3)
    mats[2][0:2, 2] = 30, 4          # 30 columns right, 4 rows down
    return mats


# name -> (experiment, B, H, W, size, flip flags, affine, labels: "raw" ids 0..35 with some 255 | "single")
CASES = {
    "96x160": (2, 3, 96, 160, 0.4, (1, 2, 3), False, "raw"),
    "96x160, other flips": (2, 3, 96, 160, 0.4, (0, 3, 1), False, "raw"),
    "80x72 (W < H)": (1, 2, 80, 72, 0.4, (0, 1), False, "raw"),
    "48x80 warped onto 96x160": (2, 3, 48, 80, 0.4, (0, 1, 2), True, "raw"),
    "352x352, region 320x320": (1, 1, 352, 352, 0.1, (3,), False, "raw"),
    "single class": (2, 2, 96, 160, 0.4, (0, 1), False, "single"),
}


@functools.lru_cache(maxsize=None)
def _case(name):
    """inputs, the restatement's canvas labels and the region's running sums for one case: computed once, shared, never written to"""
    from miccai2021_cataract_semantic_segmentation_amd.utils import CLASS_REMAP, remap_lut
    from miccai2021_cataract_semantic_segmentation_amd.utils.geometry import crop_px
    exp, B, H, W, size, flags, affine, kind = CASES[name]
    rng = np.random.RandomState(H * W + B)
    if kind == "single":
        lbl = np.full((B, H, W), 5, dtype=np.uint8)
    else:
        lbl = rng.randint(0, 36, (B, H, W)).astype(np.uint8)                 # raw CaDIS ids, per pixel
        lbl[:, H // 3:H // 2, W // 4:W // 2] = 255                            # a value outside the dataset's ids: lut sends it to the last class
        lbl[:, :H // 4, : W // 3] = 4                                         # and a blob
    lut = remap_lut(exp)
    assert lut[255] == len(CLASS_REMAP[exp]) - 1
    mats = _mats48() if affine else None
    Hc, Wc = (2 * H, 2 * W) if affine else (H, W)
    px = crop_px(size, Hc, Wc)
    zero = np.zeros((H, W, 3), dtype=np.uint8)
    canvas = np.stack([WR.augment_frame(zero, lbl[b], lut, flags[b], mats[b] if affine else None, len(CLASS_REMAP[exp]))[1] for b in range(B)])
    assert canvas.shape == (B, Hc, Wc)
    c = {"exp": exp, "lbl": lbl, "lut": lut, "flags": np.array(flags, dtype=np.int32), "mats": mats, "canvas": (Hc, Wc), "px": px,
         "labels": canvas, "wq": _weights(exp)}
    for v in c.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return c


def _pick(c, m53):
    from miccai2021_cataract_semantic_segmentation_amd import ops
    from miccai2021_cataract_semantic_segmentation_amd.utils.geometry import affine_inverse
    dev = torch.device("cuda")
    minv = affine_inverse(c["mats"]) if c["mats"] is not None else None
    out = ops.crop_freq_pick(torch.from_numpy(c["lbl"].copy()).to(dev), torch.from_numpy(c["lut"].copy()).to(dev),
                             torch.from_numpy(c["flags"].copy()).to(dev), minv, c["canvas"], c["px"], list(c["wq"]), m53, return_debug=True)
    torch.cuda.synchronize()
    return [t.cpu().numpy() for t in out]


def _expect(c, m53):
    rows = [CR.integer_pick(c["labels"][b], c["px"], list(c["wq"]), m53[b]) for b in range(len(m53))]
    return (np.array([r[:2] for r in rows], dtype=np.int32), np.array([r[2] for r in rows], dtype=np.int64),
            np.array([r[3] for r in rows], dtype=np.int64))


def _cum(c, b):
    """running sum of the integer weights over frame b's region, and the region's shape"""
    margin, rh, rw = CR.region(*c["canvas"], c["px"])
    Hc = c["canvas"][0]
    table = np.zeros(256, dtype=np.int64)
    table[:len(c["wq"])] = c["wq"]
    return np.cumsum(table[c["labels"][b][margin:Hc - margin, margin:Hc - margin].reshape(-1)]), rh, rw


@pytest.mark.parametrize("name", list(CASES))
def test_device_pick_equals_the_integer_restatement(name):
    """random draws, the first and the last pixel (m = 0, m = 2^53 - 1), and per frame an m whose T equals a running sum EXACTLY (the strict
    > must then take the next pixel); origins, totals and flat indices, twice with identical bits"""
    _need_gpu()
    c = _case(name)
    B = c["lbl"].shape[0]
    pyrng = random.Random(len(name))
    draws = [[int(pyrng.random() * 2.0 ** 53) for _ in range(B)] for _ in range(3)] + [[0] * B, [M_LAST] * B]
    exact, row_end = [], []
    for b in range(B):
        cum, rh, rw = _cum(c, b)
        row = (rh * (b + 1)) // (B + 2)
        i = row * rw + min(rw - 2, 300)                                 # (a column past the first 256 where rows are that long)
        exact.append(CR.m_with_threshold(int(cum[-1]), int(cum[i])))
        row_end.append(CR.m_with_threshold(int(cum[-1]), int(cum[(rh - 1 - row) * rw - 1])))    # the sum up to a row's end: the next row's first pixel
    draws += [exact, row_end]
    for m53 in draws:
        got, want = _pick(c, m53), _expect(c, m53)
        for g, w in zip(got, want):
            assert g.dtype == w.dtype and np.array_equal(g, w), (name, m53, got, want)
        again = _pick(c, m53)
        assert all(np.array_equal(a, g) for a, g in zip(again, got)), "two launches differ"
    # what the special draws mean, beyond agreeing with the restatement
    cum, rh, rw = _cum(c, 0)
    assert tuple(_expect(c, [0] * B)[0][0]) == (0, 0) and _expect(c, [M_LAST] * B)[2][0] == rh * rw - 1
    flat = _expect(c, exact)[2]
    for b in range(B):
        cum, rh, rw = _cum(c, b)
        T = (exact[b] * int(cum[-1])) >> 53
        assert cum[flat[b] - 1] == T and cum[flat[b]] > T, "T sits on a running sum: the pick is the NEXT pixel"
        assert flat[b] % rw == min(rw - 2, 300) + 1
    assert (_expect(c, row_end)[2] % rw == 0).all() and (_expect(c, row_end)[2] > 0).all()
    margin = c["px"] // 2
    if name.startswith("48x80"):
        reg = c["labels"][2][margin:c["canvas"][0] - margin, margin:c["canvas"][0] - margin]
        assert (reg[-8:] == 0).all() and (reg[:8, 30:] != 0).any(), "part of frame 2's region lies outside the frame's footprint"
    if name.startswith("352"):
        assert (rh, rw) == (320, 320)
    if name.startswith("96x160"):
        assert (rh, rw, c["px"]) == (64, 64, 32)


def test_all_weights_zero_and_out_of_range_draws_take_the_last_pixel():
    """the cap of random.choices (hi = n - 1), straight through the C ABI past ops' checks: a table of zeros (total 0), and m >= 2^53"""
    _need_gpu()
    from miccai2021_cataract_semantic_segmentation_amd import _lib, ops
    dev = torch.device("cuda")
    c = _case("96x160")
    lbl = torch.from_numpy(c["lbl"].copy()).to(dev)
    lut = torch.from_numpy(c["lut"].copy()).to(dev)
    nbytes = _lib.lib.catseg_crop_freq_workspace(3, 96, 160, 32)
    ws = torch.empty(nbytes // 8, dtype=torch.int64, device=dev)
    for table, m in ((torch.zeros(256, dtype=torch.int64, device=dev), [5, 1 << 52, M_LAST]),
                     (ops.crop_freq_table(c["wq"], dev), [1 << 53, (1 << 63) - 1, -1])):
        m_d = torch.tensor(m, dtype=torch.int64, device=dev)
        origin = torch.full((3, 2), -7, dtype=torch.int32, device=dev)
        _lib.check(_lib.lib.catseg_crop_freq_pick(lbl.data_ptr(), 3, 96, 160, lut.data_ptr(), None, None, 96, 160, 32, table.data_ptr(),
                                                  m_d.data_ptr(), origin.data_ptr(), None, None, ws.data_ptr(), nbytes, _lib.stream()))
        torch.cuda.synchronize()
        assert origin.cpu().tolist() == [[63, 63]] * 3


def test_ops_refuses_bad_tables_and_draws():
    _need_gpu()
    from miccai2021_cataract_semantic_segmentation_amd import ops
    dev = torch.device("cuda")
    lbl = torch.zeros((1, 96, 160), dtype=torch.uint8, device=dev)
    with pytest.raises(ValueError, match="2\\^62"):
        ops.crop_freq_pick(lbl, None, None, None, None, 32, [1, 1 << 50], [0])
    for m in ([1 << 53], [-1], [0, 0]):
        with pytest.raises(ValueError, match="m53"):
            ops.crop_freq_pick(lbl, None, None, None, None, 32, [1, 2], m)
    with pytest.raises(ops._lib.CatsegError, match="empty region"):
        ops.crop_freq_pick(torch.zeros((1, 64, 64), dtype=torch.uint8, device=dev), None, None, None, None, 64, [1, 2], [0])


def test_gpu_ingest_freq_form_equals_the_restated_origins():
    """GpuIngest(crop={'mode': 'freq', ...}) = pick + warp on the device equals GpuIngest(crop=(restated origins, px)): images and labels,
    bit for bit, with an affine and flips"""
    _need_gpu()
    from miccai2021_cataract_semantic_segmentation_amd.utils import GpuIngest
    from miccai2021_cataract_semantic_segmentation_amd.utils.geometry import freq_m53
    c = _case("48x80 warped onto 96x160")
    B, H, W = c["lbl"].shape
    img = torch.from_numpy(np.random.RandomState(3).randint(0, 256, (B, H, W, 3)).astype(np.uint8))
    lbl = torch.from_numpy(c["lbl"].copy())
    u = np.array([0.03125, 0.6180339887498949, 0.9999999], dtype=np.float64)
    origins = _expect(c, freq_m53(u))[0]
    ingest = GpuIngest(c["exp"], pad=(0, 0))
    for nhwc4 in (False, True):
        x, labels = ingest(img, lbl, c["flags"].copy(), nhwc4=nhwc4, affine=c["mats"], crop={"mode": "freq", "u": u, "px": c["px"], "table": list(c["wq"])})
        xr, lr = ingest(img, lbl, c["flags"].copy(), nhwc4=nhwc4, affine=c["mats"], crop=(origins, c["px"]))
        assert x.shape == xr.shape and labels.shape == (B, c["px"], c["px"]) and torch.equal(x, xr) and torch.equal(labels, lr)
    for b in range(B):          # and the labels against the restatement's canvas
        v, h = origins[b]
        assert np.array_equal(labels[b].cpu().numpy(), c["labels"][b][v:v + c["px"], h:h + c["px"]])
    with pytest.raises(ValueError, match="needs labels"):
        ingest(img, None, c["flags"].copy(), affine=c["mats"], crop={"mode": "freq", "u": u, "px": c["px"], "table": list(c["wq"])})


class _Frames:
    """four deterministic 48 x 80 frames (module level: picklable / inheritable by loader workers)"""

    def __len__(self):
        return 4

    def __getitem__(self, i):
        rng = np.random.RandomState(700 + i)
        return rng.randint(0, 256, (48, 80, 3)).astype(np.uint8), rng.randint(0, 36, (48, 80)).astype(np.uint8)


def test_pinned_frame_loader_freq_crop():
    """'affine' + 'crop' in mode 'freq' through the loader: one random() per frame from the epoch's Python stream, the windows equal to the
    restatement's; the same seed reproduces them, the next epoch draws others"""
    _need_gpu()
    from miccai2021_cataract_semantic_segmentation_amd.utils import (CLASS_REMAP, GpuIngest, PinnedFrameLoader, crop_px, geometry_from_transforms,
                                                                      remap_lut, sample_affine, sample_freq_u)
    from miccai2021_cataract_semantic_segmentation_amd.utils.geometry import freq_m53
    from miccai2021_cataract_semantic_segmentation_amd.utils.ingest import sample_flips
    g = np.load(GOLDEN)
    with pytest.raises(NotImplementedError, match="freq"):
        PinnedFrameLoader(_Frames(), batch_size=2, experiment=2, crop={"size": 0.4, "mode": "freq"})
    geo = geometry_from_transforms(["flip", "pad", "affine", "crop"], {"crop_size": 0.4, "crop_mode": "freq", "crop_freq_on_device": True,
                                                                        "experiment": 2, "class_sums": g["class_sums"].tolist()})
    ds = _Frames()
    loader = PinnedFrameLoader(ds, batch_size=2, experiment=2, seed=4, shuffle=False, pad=geo["pad"], affine=geo["affine"], crop=geo["crop"])
    first = [(x.clone(), l.clone()) for x, l in loader]
    second = [(x.clone(), l.clone()) for x, l in loader]                  # the loader's next epoch
    fresh = PinnedFrameLoader(ds, batch_size=2, experiment=2, seed=4, shuffle=False, pad=geo["pad"], affine=geo["affine"], crop=geo["crop"])
    again = [(x.clone(), l.clone()) for x, l in fresh]
    assert len(first) == len(second) == 2
    assert all(torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]) for a, b in zip(first, again)), "the same seed and epoch reproduce the windows"
    assert not all(torch.equal(a[1], b[1]) for a, b in zip(first, second)), "the next epoch draws other windows"
    s = 4 * 1000003 + 1
    rng, pyrng = np.random.RandomState(s), random.Random(s)
    flips = [sample_flips(2, (0.0, 0.5), rng) for _ in range(2)]
    px, wq, lut = crop_px(0.4, 96, 160), list(_weights(2)), remap_lut(2)
    assert px == 32
    for bi, (x, labels) in enumerate(first):
        mats = sample_affine(2, (48, 80), geo["affine"], rng)[1]
        m53 = freq_m53(sample_freq_u(2, pyrng))
        img = np.stack([ds[i][0] for i in range(bi * 2, bi * 2 + 2)])
        lbl = np.stack([ds[i][1] for i in range(bi * 2, bi * 2 + 2)])
        canvas = [WR.augment_frame(img[b], lbl[b], lut, flips[bi][b], mats[b], len(CLASS_REMAP[2])) for b in range(2)]
        origins = np.array([CR.integer_pick(canvas[b][1], px, wq, m53[b])[:2] for b in range(2)], dtype=np.int32)
        for b in range(2):
            v, h = origins[b]
            assert np.array_equal(labels[b].cpu().numpy(), canvas[b][1][v:v + px, h:h + px])
            assert np.array_equal(x[b].cpu().numpy(), WR.to_tensor(canvas[b][0][v:v + px, h:h + px]))
        xr, lr = GpuIngest(2, pad=(0, 0))(torch.from_numpy(img), torch.from_numpy(lbl), flips[bi], affine=mats, crop=(origins, px))
        assert torch.equal(x, xr) and torch.equal(labels, lr)
