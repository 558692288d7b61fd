"""Host side of the geometric augmentations (numpy only; importable without libcatseg_hip.so).

Restatement of what the reference does with the `rot` / `shift` / `shear` / `affine` / `crop` / `pad` keywords of its `transforms`
config list: the keyword table of ``parse_transform_list`` (utils/utils.py:356-401), the random draws and matrices of ``AffineNP``
(utils/transforms.py:38-105) and the window of ``CropNP`` in mode 'random' (:270-303).  The pixels themselves are computed on the
device: ``ops.ingest_warp_u8`` / ``GpuIngest(..., affine=, crop=)`` (csrc/warp.hip).  Pinned bit for bit against
tests/golden/geometry.npz, which the reference's own methods wrote."""
import random as _random

import numpy as np


def geometry_from_transforms(transform_list, transform_values=None):
    """The reference's keyword table (utils/utils.py:356-388) and its pad rule (:394-398) ->
    ``{"affine": None | params of AffineNP, "crop": None | {"size", "mode"}, "pad": (top, bottom)}``"""
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
        raise NotImplementedError("crop_mode 'freq' is not supported: the pick depends on the warped labels (a sequential float64 "
                                  "accumulate over float32 class weights, random.choices); only crop_mode 'random' runs on the device")
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
