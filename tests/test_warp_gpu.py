"""catseg_ingest_warp_u8 (remap / flip / affine warp / crop window / reflect pad / ToTensor / Normalize in one launch) against the dense
float64 restatement of the reference's AffineNP + CropNP + PadNP sequence (tests/_warp_ref.py): every comparison exact, no tolerance."""
import functools
import os
import random

import numpy as np
import pytest
import torch

import _warp_ref as WR

pytestmark = pytest.mark.gpu

MEAN, STD = [0.485, 0.456, 0.406], [0.229, 0.224, 0.225]
FRAMES = {(3, 7, 13, 8): (1, [1, 2, 3]), (2, 10, 14, 17): (2, [0, 3]), (2, 33, 47, 25): (3, [2, 1])}    # (B, H, W, K) -> experiment, flip flags


def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")


def _mats(B):
    """the reference's own draws (fixture, 10 x 14 frames): 'affine' for even frames, rot + shift + shear for odd ones"""
    g = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "geometry.npz"))
    return np.stack([g["mats"][3 if b % 2 == 0 else 4, 0, b, 3] for b in range(B)])


@functools.lru_cache(maxsize=None)
def _case(shape):
    """inputs and the restatement's full canvas for one frame set: computed once, shared by the tests, never written to"""
    from miccai2021_cataract_semantic_segmentation_amd.utils import CLASS_REMAP, NUM_CLASSES, remap_lut
    B, H, W, K = shape
    exp, flags = FRAMES[shape]
    assert NUM_CLASSES[exp] == K
    rng = np.random.RandomState(H * W)
    img = rng.randint(0, 256, (B, H, W, 3)).astype(np.uint8)
    lbl = rng.randint(0, 36, (B, H, W)).astype(np.uint8)              # raw CaDIS ids
    lut, mats = remap_lut(exp), _mats(B)
    frames = [WR.augment_frame(img[b], lbl[b], lut, flags[b], mats[b], len(CLASS_REMAP[exp])) for b in range(B)]
    c = {"exp": exp, "img": img, "lbl": lbl, "flags": np.array(flags, dtype=np.int32), "mats": mats,
         "canvas_img": np.stack([f[0] for f in frames]), "canvas_lbl": np.stack([f[1] for f in frames])}
    for v in c.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return c


def _run(c, origin, window, pad=(0, 0), normalise=False, outputs=("nchw", "nhwc4", "u8"), image=True, label=True, minv="affine", canvas=None):
    from miccai2021_cataract_semantic_segmentation_amd import ops
    from miccai2021_cataract_semantic_segmentation_amd.utils import remap_lut
    from miccai2021_cataract_semantic_segmentation_amd.utils.geometry import affine_inverse
    dev = torch.device("cuda")
    B, H, W = c["lbl"].shape
    if isinstance(minv, str):
        minv = affine_inverse(c["mats"])
    if canvas is None:
        canvas = (2 * H, 2 * W)
    mean = torch.tensor(MEAN, device=dev) if normalise else None
    std = torch.tensor(STD, device=dev) if normalise else None
    out = ops.ingest_warp_u8(torch.from_numpy(c["img"].copy()).to(dev) if image else None, torch.from_numpy(c["lbl"].copy()).to(dev) if label else None,
                             torch.from_numpy(remap_lut(c["exp"])).to(dev), torch.from_numpy(c["flags"].copy()).to(dev), minv, canvas, origin, window,
                             pad[0], pad[1], mean, std, outputs=outputs)
    return {k: (v.cpu().numpy() if v is not None else None) for k, v in out.items()}


def _windows(H, W, B):
    """name -> (origins [B,2] or None, (Hw, Ww)) on the 2H x 2W canvas"""
    Hc, Wc = 2 * H, 2 * W
    return {"full": (None, (Hc, Wc)),
            "interior": (np.array([[1 + b, 2 + b] for b in range(B)]), (H, W + 3)),
            "corner": (np.array([[Hc - (H + 2), Wc - (W + 3)]] * B), (H + 2, W + 3)),          # flush with the bottom-right corner
            "outside": (np.array([[Hc - 2, Wc - 3]] * B), (2, 3))}                              # wholly outside the frame's footprint


def _expect(c, origin, window):
    B = c["lbl"].shape[0]
    o = np.zeros((B, 2), dtype=np.int64) if origin is None else origin
    img = np.stack([c["canvas_img"][b, o[b, 0]:o[b, 0] + window[0], o[b, 1]:o[b, 1] + window[1]] for b in range(B)])
    lbl = np.stack([c["canvas_lbl"][b, o[b, 0]:o[b, 0] + window[0], o[b, 1]:o[b, 1] + window[1]] for b in range(B)])
    assert img.shape[1:3] == tuple(window)
    return img, lbl


def _check_image_forms(got, img_u8, normalise):
    want = WR.to_tensor(img_u8, MEAN if normalise else None, STD if normalise else None)
    assert np.array_equal(got["u8"], img_u8)
    assert np.array_equal(got["nchw"], want)
    assert np.array_equal(got["nhwc4"][..., :3], np.moveaxis(want, 1, -1)) and not got["nhwc4"][..., 3].any()


@pytest.mark.parametrize("normalise", [False, True])
@pytest.mark.parametrize("shape", list(FRAMES))
def test_affine_windows_match_the_restatement(shape, normalise):
    """every window of the canvas, all three image forms and the labels in one launch; all four flip flags over the frame sets; raw labels
    through the experiment's LUT; a window wholly outside the footprint is colour 0 (normalised: (0 - mean) / std) and label 0"""
    _need_gpu()
    c = _case(shape)
    B, H, W, K = shape
    assert c["canvas_img"].any() and c["canvas_lbl"].any() and int(c["canvas_lbl"].max()) < K + 1
    for name, (origin, window) in _windows(H, W, B).items():
        img_u8, lbl = _expect(c, origin, window)
        got = _run(c, origin, window, normalise=normalise)
        _check_image_forms(got, img_u8, normalise)
        assert got["labels"].dtype == np.int64 and np.array_equal(got["labels"], lbl), name
        if name == "outside":
            assert not img_u8.any() and not lbl.any() and not got["labels"].any() and not got["u8"].any()
            zero = WR.to_tensor(np.zeros((1, 1, 1, 3), dtype=np.uint8), MEAN if normalise else None, STD if normalise else None).reshape(3)
            assert all(np.array_equal(got["nchw"][:, ch], np.full_like(got["nchw"][:, ch], zero[ch])) for ch in range(3))
        elif name != "full":
            assert img_u8.any() and lbl.any(), name               # the window does show a part of the frame


def test_image_only_and_label_only_calls():
    _need_gpu()
    shape = (3, 7, 13, 8)
    c = _case(shape)
    origin, window = _windows(7, 13, 3)["interior"]
    img_u8, lbl = _expect(c, origin, window)
    got = _run(c, origin, window, normalise=True, outputs=("nchw",), label=False)
    assert got["labels"] is None and set(got) == {"nchw", "labels"} and np.array_equal(got["nchw"], WR.to_tensor(img_u8, MEAN, STD))
    got = _run(c, origin, window, outputs=("u8",), label=False)
    assert np.array_equal(got["u8"], img_u8)
    got = _run(c, origin, window, image=False)
    assert set(got) == {"labels"} and np.array_equal(got["labels"], lbl)


def test_pad_on_the_full_canvas_and_plain_crop_of_the_frame():
    """PadNP((2, 2), 'reflect') of the canvas rows after an affine (GpuIngest's own pad); no matrix, canvas = frame, a crop window: the numpy
    crop of catseg_ingest_u8's own output, bit for bit"""
    _need_gpu()
    from miccai2021_cataract_semantic_segmentation_amd.utils import GpuIngest
    shape = (2, 10, 14, 17)
    c = _case(shape)
    img, lbl = torch.from_numpy(c["img"].copy()), torch.from_numpy(c["lbl"].copy())
    x, labels = GpuIngest(2, pad=(2, 2), normalise=True)(img, lbl, c["flags"].copy(), affine=c["mats"])
    want_img = np.pad(c["canvas_img"], ((0, 0), (2, 2), (0, 0), (0, 0)), mode="reflect")
    want_lbl = np.pad(c["canvas_lbl"], ((0, 0), (2, 2), (0, 0)), mode="reflect")
    assert x.shape == (2, 3, 24, 28) and np.array_equal(x.cpu().numpy(), WR.to_tensor(want_img, MEAN, STD))
    assert np.array_equal(labels.cpu().numpy(), want_lbl)
    x4, _ = GpuIngest(2, pad=(2, 2))(img, lbl, c["flags"].copy(), affine=c["mats"], nhwc4=True)
    assert np.array_equal(x4.cpu().numpy()[..., :3], np.moveaxis(WR.to_tensor(want_img), 1, -1))
    # asymmetric pad through the op itself
    got = _run(c, None, (20, 28), pad=(3, 1))
    assert np.array_equal(got["u8"], np.pad(c["canvas_img"], ((0, 0), (3, 1), (0, 0), (0, 0)), mode="reflect"))
    assert np.array_equal(got["labels"], np.pad(c["canvas_lbl"], ((0, 0), (3, 1), (0, 0)), mode="reflect"))
    # crop without an affine: square through GpuIngest (px = 6), a non-square window through the op
    full_x, full_l = GpuIngest(2, pad=(0, 0), normalise=True)(img, lbl, c["flags"].copy())
    origins = np.array([[3, 7], [4, 0]], dtype=np.int32)
    x, labels = GpuIngest(2, pad=(2, 2), normalise=True)(img, lbl, c["flags"].copy(), crop=(origins, 6))     # (a crop drops the padding)
    assert x.shape == (2, 3, 6, 6) and labels.shape == (2, 6, 6)
    for b, (v, h) in enumerate(origins):
        assert torch.equal(x[b], full_x[b, :, v:v + 6, h:h + 6]) and torch.equal(labels[b], full_l[b, v:v + 6, h:h + 6])
    got = _run(c, origins, (5, 7), normalise=True, minv=None, canvas=(10, 14))
    for b, (v, h) in enumerate(origins):
        assert np.array_equal(got["nchw"][b], full_x[b, :, v:v + 5, h:h + 7].cpu().numpy())
        assert np.array_equal(got["labels"][b], full_l[b, v:v + 5, h:h + 7].cpu().numpy())


def test_identity_half_pixel_ties_and_label_ties():
    _need_gpu()
    from miccai2021_cataract_semantic_segmentation_amd import ops
    from miccai2021_cataract_semantic_segmentation_amd.utils import GpuIngest
    dev = torch.device("cuda")
    c = _case((2, 10, 14, 17))
    img, lbl = torch.from_numpy(c["img"].copy()), torch.from_numpy(c["lbl"].copy())
    # identity on the 2H x 2W canvas: the frame in the top-left corner, zeros elsewhere
    full_x, full_l = GpuIngest(2, pad=(0, 0))(img, lbl, c["flags"].copy())
    x, labels = GpuIngest(2, pad=(0, 0))(img, lbl, c["flags"].copy(), affine=np.stack([np.identity(3)] * 2))
    assert x.shape == (2, 3, 20, 28) and torch.equal(x[:, :, :10, :14], full_x) and torch.equal(labels[:, :10, :14], full_l)
    assert not x[:, :, 10:].any() and not x[:, :, :, 14:].any() and not labels[:, 10:].any() and not labels[:, :, 14:].any()
    # half-pixel shift: every interior colour is a k + 0.5 tie for some pixel (np.round: half to even)
    half = np.array([[[1, 0, .5], [0, 1, .5], [0, 0, 1]]], dtype=np.float64)
    rng = np.random.RandomState(8)
    im8 = rng.randint(0, 256, (1, 8, 8, 3)).astype(np.uint8)
    lb8 = rng.randint(0, 5, (1, 8, 8)).astype(np.uint8)
    want_img, want_lbl = WR.affine_np(im8[0], lb8[0].astype(np.int32), half[0], 5)
    sums = (im8[0, :-1, :-1].astype(int) + im8[0, :-1, 1:] + im8[0, 1:, :-1] + im8[0, 1:, 1:])
    assert (sums % 4 == 2).any()                                        # ties are there
    got = ops.ingest_warp_u8(torch.from_numpy(im8).to(dev), torch.from_numpy(lb8).to(dev), None, None, np.linalg.inv(half[0])[None], (16, 16),
                             None, None, outputs=("u8",))
    assert np.array_equal(got["u8"][0].cpu().numpy(), want_img) and np.array_equal(got["labels"][0].cpu().numpy(), want_lbl)
    # two-class checkerboard (ids 1 and 2, no LUT) under the same shift: every interior pixel is a 512 : 512 tie -> the smaller id
    yy, xx = np.mgrid[0:8, 0:8]
    board = (1 + (yy + xx) % 2).astype(np.uint8)[None]
    want_lbl = WR.affine_np(im8[0], board[0].astype(np.int32), half[0], 3)[1]
    assert (want_lbl[1:8, 1:8] == 1).all() and set(np.unique(want_lbl)) == {0, 1, 2}
    got = ops.ingest_warp_u8(None, torch.from_numpy(board).to(dev), None, None, np.linalg.inv(half[0])[None], (16, 16), None, None)
    assert np.array_equal(got["labels"][0].cpu().numpy(), want_lbl)


def test_coordinates_are_not_contracted_into_fma():
    """at canvas (27, 5) the separately rounded ((a x + b y) + c) * 32 is 323.5 + -> 324; a fused multiply-add gives 323.4999... -> 323 (found
    with exact rationals); source row 5 alternates 0 / 255, so the colour shows which one the kernel computed"""
    _need_gpu()
    from miccai2021_cataract_semantic_segmentation_amd import ops
    dev = torch.device("cuda")
    minv = np.array([[[float.fromhex("0x1.285425ed097b4p+5"), -198.0, 0.0], [0.0, 1.0, 0.0], [0.0, 0.0, 1.0]]])
    X, Y = WR.fixed_point_coords(minv[0], 12, 28)
    assert X[5, 27] == 324 and Y[5, 27] == 160
    img = np.zeros((1, 6, 14, 3), dtype=np.uint8)
    img[0, 5, 1::2] = 255
    lbl = np.zeros((1, 6, 14), dtype=np.uint8)
    want = WR.affine_np(img[0], lbl[0].astype(np.int32), None, 2, minv=minv[0])[0]
    assert want[5, 27, 0] == 32                                         # (255 * 4 * 32 / 1024 = 31.875; the fused result would be 24)
    got = ops.ingest_warp_u8(torch.from_numpy(img).to(dev), None, None, None, minv, (12, 28), None, None, outputs=("u8",))["u8"][0].cpu().numpy()
    assert got[5, 27, 0] == 32 and np.array_equal(got, want)


def test_host_values_are_checked_and_bad_device_values_yield_zeros():
    """ops.ingest_warp_u8 refuses non-finite matrices and windows outside the canvas; the kernel itself guards every read: matrices that
    map every canvas pixel far away (or to NaN) give zeros"""
    _need_gpu()
    from miccai2021_cataract_semantic_segmentation_amd import _lib, ops
    dev = torch.device("cuda")
    c = _case((3, 7, 13, 8))
    img, lbl = torch.from_numpy(c["img"].copy()).to(dev), torch.from_numpy(c["lbl"].copy()).to(dev)
    ident = np.stack([np.identity(3)] * 3)
    bad = ident.copy()
    bad[1, 0, 2] = np.inf
    with pytest.raises(ValueError, match="finite"):
        ops.ingest_warp_u8(img, lbl, None, None, bad, (14, 26))
    for origin in ([[0, 0], [0, 0], [11, 0]], [[0, -1], [0, 0], [0, 0]], [[0, 0], [0, 21], [0, 0]]):
        with pytest.raises(ValueError, match="inside"):
            ops.ingest_warp_u8(img, lbl, None, None, ident, (14, 26), np.array(origin), (4, 6))
    far = ident.copy()
    far[:, 0, 2], far[:, 1, 2] = 1e300, -1e300
    got = ops.ingest_warp_u8(img, lbl, None, None, far, (14, 26), outputs=("u8",))
    assert not got["u8"].any() and not got["labels"].any()
    # past ops' checks, straight through the C ABI: NaN matrices and an origin far outside the canvas
    nan = torch.full((3, 6), float("nan"), dtype=torch.float64, device=dev)
    org = torch.tensor([[1 << 30, -(1 << 30)], [-5, 0], [13, 25]], dtype=torch.int32, device=dev)
    u8 = torch.full((3, 4, 6, 3), 7, dtype=torch.uint8, device=dev)
    lab = torch.full((3, 4, 6), 7, dtype=torch.int64, device=dev)
    for minv in (nan, torch.from_numpy(ident[:, :2].reshape(3, 6).copy()).to(dev)):
        u8.fill_(7)
        lab.fill_(7)
        _lib.check(_lib.lib.catseg_ingest_warp_u8(img.data_ptr(), lbl.data_ptr(), 3, 7, 13, None, None, minv.data_ptr(), 14, 26, org.data_ptr(), 4, 6,
                                                  0, 0, None, None, None, None, u8.data_ptr(), lab.data_ptr(), _lib.stream()))
        if minv is nan:
            assert not u8.any() and not lab.any()
        else:       # identity: frame 1's window starts 5 rows above the canvas (rows 0..3 outside), frame 2's window is beyond the frame
            assert not u8[0].any() and not u8[1].any() and not u8[2].any() and not lab.any()


class _Frames:
    """six deterministic 80 x 140 frames (module level: picklable / inheritable by loader workers)"""

    def __len__(self):
        return 6

    def __getitem__(self, i):
        rng = np.random.RandomState(500 + i)
        return rng.randint(0, 256, (80, 140, 3)).astype(np.uint8), rng.randint(0, 36, (80, 140)).astype(np.uint8)


@pytest.mark.parametrize("extras", [False, True])
def test_pinned_frame_loader_affine_and_crop(extras):
    """'affine' + 'crop' 0.4 through the loader: 64 x 64 windows (the crop size comes from the 160-row canvas), equal to GpuIngest with the
    same draws (flips, [blur radii,] affine from the epoch's numpy stream; crops from Python's random); same seed and epoch -> identical.
    extras: with 'blur' and 'colorjitter' on as well"""
    _need_gpu()
    from miccai2021_cataract_semantic_segmentation_amd.utils import (GpuIngest, PinnedFrameLoader, crop_px, geometry_from_transforms, sample_affine,
                                                                      sample_blur, sample_color_jitter, sample_crops)
    from miccai2021_cataract_semantic_segmentation_amd.utils.ingest import sample_flips
    geo = geometry_from_transforms(["flip", "pad", "affine", "crop"] + (["blur", "colorjitter"] if extras else []),
                                   {"crop_size": 0.4, "crop_mode": "random", "experiment": 3})
    assert geo["pad"] == (0, 0)
    ds = _Frames()

    def epoch():
        loader = PinnedFrameLoader(ds, batch_size=3, experiment=3, seed=9, shuffle=False, pad=geo["pad"], affine=geo["affine"], crop=geo["crop"],
                                   blur=extras, colorjitter=extras)
        return [(x.clone(), l.clone()) for x, l in loader]

    out = epoch()
    assert len(out) == 2
    s = 9 * 1000003 + 1
    rng, gen, pyrng = np.random.RandomState(s), torch.Generator().manual_seed(s), random.Random(s)
    flips = [sample_flips(3, (0.0, 0.5), rng) for _ in range(2)]
    blurs = [sample_blur(3, random=rng) if extras else None for _ in range(2)]
    jit = [sample_color_jitter(3, generator=gen) if extras else None for _ in range(2)]
    px = crop_px(0.4, 160, 280)
    assert px == 64
    for bi, (x, labels) in enumerate(out):
        assert x.shape == (3, 3, 64, 64) and labels.shape == (3, 64, 64) and labels.dtype == torch.int64
        mats = sample_affine(3, (80, 140), geo["affine"], rng)[1]
        origins = sample_crops(3, (160, 280), px, pyrng)
        ids = range(bi * 3, bi * 3 + 3)
        img = torch.from_numpy(np.stack([ds[i][0] for i in ids]))
        lbl = torch.from_numpy(np.stack([ds[i][1] for i in ids]))
        xr, lr = GpuIngest(3, pad=(0, 0))(img, lbl, flips[bi], blur_radii=blurs[bi], jitter=jit[bi], affine=mats, crop=(origins, px))
        assert torch.equal(x, xr) and torch.equal(labels, lr)
        xp, lp = GpuIngest(3, pad=(0, 0))(img, lbl, flips[bi], affine=mats, crop=(origins, px))
        assert torch.equal(labels, lp) and (torch.equal(x, xp) != extras)        # the label side ignores blur / jitter, the image does not
        if bi == 0 and not extras:      # and the whole chain against the restatement, once
            from miccai2021_cataract_semantic_segmentation_amd.utils import CLASS_REMAP, remap_lut
            for b in range(3):
                wi, wl = WR.augment_frame(img[b].numpy(), lbl[b].numpy(), remap_lut(3), flips[bi][b], mats[b], len(CLASS_REMAP[3]), origins[b], (px, px))
                assert np.array_equal(x[b].cpu().numpy(), WR.to_tensor(wi)) and np.array_equal(labels[b].cpu().numpy(), wl)
    again = epoch()
    assert all(torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]) for a, b in zip(out, again))
