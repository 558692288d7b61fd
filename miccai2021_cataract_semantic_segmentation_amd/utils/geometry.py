"""Host side of the geometric augmentations (numpy only; importable without libcatseg_hip.so).

Restatement of what the reference does with the `rot` / `shift` / `shear` / `affine` / `crop` / `pad` keywords of its `transforms`
config list: the keyword table of ``parse_transform_list`` (utils/utils.py:356-401), the random draws and matrices of ``AffineNP``
(utils/transforms.py:38-105) and the window of ``CropNP`` in mode 'random' (:270-303).  The pixels themselves are computed on the
device: ``ops.ingest_warp_u8`` / ``GpuIngest(..., affine=, crop=)`` (csrc/warp.hip).  Pinned bit for bit against
tests/golden/geometry.npz, which the reference's own methods wrote.

``CropNP`` in mode 'freq' (:282-293) picks its window from the warped labels, so the pick itself runs on the device
(``ops.crop_freq_pick``, csrc/cropfreq.hip); this module holds its host side: the region, the class table of ``CropNP.__init__``, the
exact integer weights and the one uniform per frame.  The device pick is the reference's wherever that uniform lies farther than 2^-22
from every cumulative fraction; it is opt-in for that reason (``crop['on_device']``).  Pinned against
tests/golden/cropfreq.npz, which the reference's ``CropNP`` wrote."""
import random as _random
from fractions import Fraction

import numpy as np


def geometry_from_transforms(transform_list, transform_values=None):
    """The reference's keyword table (utils/utils.py:356-388) and its pad rule (:394-398) ->
    ``{"affine": None | params of AffineNP, "crop": None | {"size", "mode"}, "pad": (top, bottom)}``.
    crop_mode 'freq' needs ``transform_values['crop_freq_on_device'] = True`` (the device pick, see check_crop) and the class table as
    ``transform_values['class_sums']`` (the 36 per-raw-class pixel counts, with ``transform_values['experiment']``) or
    ``transform_values['class_frequencies']``"""
    transform_values = transform_values or {}
    rotation, rot_centre_offset, shift, shear, shear_centre_offset = 0, (.2, .2), 0, (0, 0), (.2, .2)
    set_affine = False
    if 'rot' in transform_list:
        rotation, set_affine = 15, True
    if 'shift' in transform_list:
        shift, set_affine = .1, True
    if 'shear' in transform_list:
        shear, set_affine = (.1, .1), True
    if 'affine' in transform_list:        # applied last: overrides 'rot'
        rotation, shear, rot_centre_offset, set_affine = 10, (.1, .1), (.1, .1), True
    affine = None
    if set_affine:
        affine = {"crop_to_fit": False, "rotation": rotation, "rot_centre_offset": rot_centre_offset, "shift": shift, "shear": shear,
                  "shear_centre_offset": shear_centre_offset}
    crop = None
    if 'crop' in transform_list:
        crop = {"size": transform_values['crop_size'], "mode": transform_values['crop_mode']}
        if transform_values.get('crop_freq_on_device', False):
            crop["on_device"] = True
            if 'class_frequencies' in transform_values:
                crop["class_frequencies"] = transform_values['class_frequencies']
            elif 'class_sums' in transform_values:
                crop["class_frequencies"] = class_frequencies(transform_values['class_sums'], transform_values['experiment'])
        check_crop(crop)
    pad = (2, 2) if ('pad' in transform_list and 'crop' not in transform_list) else (0, 0)   # padding only if nothing was cropped
    return {"affine": affine, "crop": crop, "pad": pad}


def check_affine(params):
    if params.get("crop_to_fit", False):
        raise NotImplementedError("AffineNP(crop_to_fit=True) is not supported: the reference's transform wiring never passes it "
                                  "(utils/utils.py:377), and it needs cv2.resize of the inscribed rectangle")


def check_crop(params):
    mode = params.get("mode", "random")
    if mode == "freq":
        if not params.get("on_device", False):
            raise NotImplementedError("crop_mode 'freq' is not supported without crop['on_device'] = True (transform_values["
                                      "'crop_freq_on_device']): the reference's pick is a sequential float64 accumulate over float32 class "
                                      "weights (random.choices); the device evaluates it in exact integers, which is the reference's "
                                      "pick only where the draw lies farther than 2^-22 from every cumulative fraction")
        if params.get("class_frequencies") is None and params.get("class_sums") is None:
            raise ValueError("crop_mode 'freq' needs the class table: crop['class_sums'] (per raw class pixel counts, with "
                             "crop['experiment']) or crop['class_frequencies']")
        return
    if mode != "random":
        raise ValueError("Crop mode '{}' not recognised.".format(mode))


def _shift_matrix(ver, hor):
    matrix = np.identity(3)
    matrix[0:2, 2] = hor, ver
    return matrix


def rot_matrix(rot_vals):
    """get_rot_matrix: rot_vals = (centre_ver, centre_hor, degrees)"""
    matrix = np.identity(3)
    rot = np.radians(rot_vals[2])
    matrix[0:2, 0:2] = [[np.cos(rot), -np.sin(rot)], [np.sin(rot), np.cos(rot)]]
    return _shift_matrix(rot_vals[0], rot_vals[1]) @ matrix @ _shift_matrix(-rot_vals[0], -rot_vals[1])


def shift_matrix(shift_vals):
    """get_shift_matrix: shift_vals = (ver, hor)"""
    return _shift_matrix(shift_vals[0], shift_vals[1])


def shear_matrix(shear_vals):
    """get_shear_matrix: shear_vals = (centre_ver, centre_hor, shear_ver, shear_hor)"""
    matrix = np.identity(3)
    matrix[1, 0] = shear_vals[2]
    matrix[0, 1] = shear_vals[3]
    return _shift_matrix(shear_vals[0], shear_vals[1]) @ matrix @ _shift_matrix(-shear_vals[0], -shear_vals[1])


def sample_affine(batch, frame, params, random=np.random):
    """AffineNP's nine draws per frame from ``random.rand()``, in its order (rotation angle, rotation centre ver / hor; shift ver / hor;
    shear ver / hor, shear centre ver / hor), consumed even where the parameter is 0.
    Returns (values, matrices): values = {"rot": [B,3] (centre_ver, centre_hor, degrees), "shift": [B,2] (ver, hor),
    "shear": [B,4] (centre_ver, centre_hor, shear_ver, shear_hor)} as float64, matrices float64 [B,3,3] = shift @ rot @ shear
    (frame -> canvas, x = column first)."""
    check_affine(params)
    H, W = int(frame[0]), int(frame[1])
    rotation, rco = params["rotation"], params["rot_centre_offset"]
    shift, shear, sco = params["shift"], params["shear"], params["shear_centre_offset"]
    vals = {"rot": np.zeros((batch, 3)), "shift": np.zeros((batch, 2)), "shear": np.zeros((batch, 4))}
    mats = np.zeros((batch, 3, 3))
    for b in range(batch):
        rot = rotation * (2 * random.rand() - 1)
        rot_centre_ver = int(np.round(H * (.5 + rco[0] * (2 * random.rand() - 1))))
        rot_centre_hor = int(np.round(W * (.5 + rco[1] * (2 * random.rand() - 1))))
        shift_ver = int(np.round(H * shift * random.rand()))
        shift_hor = int(np.round(W * shift * random.rand()))
        shear_ver = shear[0] * (2 * random.rand() - 1)
        shear_hor = shear[1] * (2 * random.rand() - 1)
        shear_centre_ver = int(np.round(H * (.5 + sco[0] * (2 * random.rand() - 1))))
        shear_centre_hor = int(np.round(W * (.5 + sco[1] * (2 * random.rand() - 1))))
        vals["rot"][b] = rot_centre_ver, rot_centre_hor, rot
        vals["shift"][b] = shift_ver, shift_hor
        vals["shear"][b] = shear_centre_ver, shear_centre_hor, shear_ver, shear_hor
        mats[b] = (shift_matrix((shift_ver, shift_hor)) @ rot_matrix((rot_centre_ver, rot_centre_hor, rot))
                   @ shear_matrix((shear_centre_ver, shear_centre_hor, shear_ver, shear_hor)))
    return vals, mats


def affine_inverse(matrices):
    """canvas -> frame matrices (float64, np.linalg.inv per frame): what the warp kernel evaluates per canvas pixel"""
    matrices = np.asarray(matrices, dtype=np.float64)
    assert matrices.shape[-2:] == (3, 3)
    return np.stack([np.linalg.inv(m) for m in matrices.reshape(-1, 3, 3)]).reshape(matrices.shape)


def crop_px(size, h, w):
    """CropNP's window edge for an h x w array (after an affine: the 2H x 2W canvas): a multiple of 32 taken from the HEIGHT, cut to
    min(h, w) where that is not below both dimensions"""
    px = int(32 * ((size * h) // 32))
    if px >= h or px >= w:
        px = min(h, w)
    return px


def sample_crops(batch, canvas, px, random=_random):
    """CropNP 'random': per frame ``randint(0, h - px)`` then ``randint(0, w - px)`` of Python's random module, each drawn only if its
    range is non-empty.  Returns int32 [B, 2] = (v, h) origins."""
    h, w = int(canvas[0]), int(canvas[1])
    out = np.zeros((batch, 2), dtype=np.int32)
    for b in range(batch):
        v_max, h_max = h - px, w - px
        out[b, 0] = random.randint(0, v_max) if v_max > 0 else 0
        out[b, 1] = random.randint(0, h_max) if h_max > 0 else 0
    return out


def crop_freq_region(h, w, px):
    """CropNP 'freq' (utils/transforms.py:287-288): (margin, rows, columns) of the region ``lbl[margin:h - margin, margin:h - margin]`` the
    pick is drawn from.  The reference slices the COLUMNS with the height too: with w > h the right part of the frame is never picked, with
    w < h numpy clips the slice at w.  The picked pixel's index in the region is used as the window's upper-left corner as it is."""
    h, w, px = int(h), int(w), int(px)
    margin = px // 2
    return margin, max(h - 2 * margin, 0), max(min(h - margin, w) - margin, 0)


def class_frequencies(class_sums, experiment):
    """CropNP.__init__'s table (utils/transforms.py:264-268): per network class the sum of the per-raw-class pixel counts `class_sums` (36
    entries: what a label table carries for the repeat-factor sampler) over the experiment's remap list, as float32, divided by their
    float32 sum.  The class after the last key of the remap is the ignore class and takes key 255.
    Experiment 3 is NOT pinned to the reference: its CropNP.__init__ raises KeyError(25) in every mode (it looks class 17 up under 255 and
    class 25 under 25); this is the evident intent -- class i from key i, the last class from key 255."""
    from .classes import CLASS_REMAP
    remap = CLASS_REMAP[experiment]
    counts = np.array(class_sums)
    sums = np.zeros(len(remap), 'f')
    for i in range(len(remap)):
        sums[i] = np.sum(counts[remap[i if i in remap else 255]])
    return sums / np.sum(sums)


def freq_weight_table(freqs):
    """(wq, s): the weights w_c = float32(1) / f_c of CropNP 'freq' as exact Python integers wq_c = w_c * s, s (a Fraction) the smallest
    power of two that makes every one an integer (a float32 is an integer over a power of two).  The pick only sees ratios: s cancels."""
    f = np.asarray(freqs, dtype=np.float32)
    with np.errstate(divide="ignore"):
        w = np.float32(1) / f
    if f.ndim != 1 or f.size == 0 or f.size > 256 or not np.isfinite(w).all() or (w <= 0).any():
        raise ValueError("freq_weight_table: 1 to 256 positive class frequencies whose float32 reciprocals are finite")
    fr = [Fraction(float(v)) for v in w]
    e = max(d.denominator.bit_length() - 1 for d in fr)        # denominators are powers of two: every w * 2^e is an integer
    wq = [int(d * (1 << e)) for d in fr]
    while all(q % 2 == 0 for q in wq):                         # (all of them multiples of two: a smaller power serves)
        wq, e = [q // 2 for q in wq], e - 1
    s = Fraction(2) ** e
    assert all(Fraction(q) / s == d for q, d in zip(wq, fr))
    return wq, s


def check_freq_weights(wq, region_pixels):
    """the device sums the weights of a region in 64 bits: refuse tables that could reach 2^62"""
    if max(wq) * max(int(region_pixels), 1) >= 1 << 62:
        raise ValueError("crop_mode 'freq': max(wq) * region pixels = %d * %d reaches 2^62: the class frequencies span too many binades "
                         "for the integer pick" % (max(wq), region_pixels))


def sample_freq_u(batch, random=_random):
    """CropNP 'freq': ONE ``random.random()`` of Python's random module per frame -- what ``random.choices(..., k=1)`` consumes -- in place
    of the two ``randint`` of mode 'random'.  Returns float64 [B]; the device takes m = int(u * 2 ** 53), which is exact."""
    return np.array([random.random() for _ in range(batch)], dtype=np.float64)


def freq_m53(u):
    """the integers int(u * 2^53) of the uniforms (exact: random.random() is a multiple of 2^-53)"""
    return [int(float(v) * 9007199254740992.0) for v in np.asarray(u, dtype=np.float64).reshape(-1)]
