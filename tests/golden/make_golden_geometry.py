"""Geometric-augmentation fixtures from the REAL reference: the keyword table of utils.parse_transform_list, the draws and matrices of
utils.transforms.AffineNP (get_*_vals, get_*_matrix) and the windows of CropNP('random'), see make_golden.py.  The warp itself
(cv2.warpPerspective) cannot be recorded: the harness stubs cv2.

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_geometry.py
"""
import os
import random
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
import ref_harness  # noqa: E402

R = ref_harness.load()
from utils import parse_transform_list            # noqa: E402  (the reference's utils package)
from utils.transforms import AffineNP, CropNP, get_rot_matrix, get_shear_matrix, get_shift_matrix   # noqa: E402

KEYSETS = (("rot",), ("shift",), ("shear",), ("affine",), ("rot", "shift", "shear"), ("rot", "affine"))
FRAMES = ((10, 14), (540, 960))
SEEDS = (3, 17, 101)
out = {"keysets": np.array(["+".join(k) for k in KEYSETS]), "frames": np.array(FRAMES, dtype=np.int64), "seeds": np.array(SEEDS, dtype=np.int64)}

NK, NF, NS = len(KEYSETS), len(FRAMES), len(SEEDS)
out["params"] = np.zeros((NK, 9))
out["rot"], out["shift"], out["shear"] = np.zeros((NK, NF, NS, 3)), np.zeros((NK, NF, NS, 2)), np.zeros((NK, NF, NS, 4))
out["mats"] = np.zeros((NK, NF, NS, 4, 3, 3))          # rot, shift, shear, shift @ rot @ shear
for ki, keys in enumerate(KEYSETS):
    common = parse_transform_list(list(keys), {}, 25)["train"]["common"]
    assert len(common) == 1 and isinstance(common[0], AffineNP)
    aff = common[0]
    # the parameters the reference's own wiring gave its AffineNP: rotation, rot centre offset (2), shift, shear (2), shear centre offset (2), crop_to_fit
    out["params"][ki] = [aff.rotation, *aff.rot_centre_offset, aff.shift, *aff.shear, *aff.shear_centre_offset, float(aff.crop_to_fit)]
    for fi, (H, W) in enumerate(FRAMES):
        arr = np.zeros((H, W, 3), dtype=np.uint8)
        for si, seed in enumerate(SEEDS):
            np.random.seed(seed)
            rot_vals = aff.get_rot_vals(arr)          # the order of AffineNP.__call__ (utils/transforms.py:39-45)
            rot_matrix = get_rot_matrix(rot_vals)
            shift_vals = aff.get_shift_vals(arr)
            shift_matrix = get_shift_matrix(shift_vals)
            shear_vals = aff.get_shear_vals(arr)
            shear_matrix = get_shear_matrix(shear_vals)
            matrix = shift_matrix @ rot_matrix @ shear_matrix
            out["rot"][ki, fi, si], out["shift"][ki, fi, si], out["shear"][ki, fi, si] = rot_vals, shift_vals, shear_vals
            out["mats"][ki, fi, si] = np.stack([rot_matrix, shift_matrix, shear_matrix, matrix])

# pad rule and crop wiring of the keyword table: which transforms each list ends up with
LISTS = (("pad",), ("pad", "crop"), ("pad", "affine"), ("pad", "affine", "crop"), ("flip", "rot"))
rows = []
for keys in LISTS:
    d = parse_transform_list(list(keys), {"crop_size": 0.4, "crop_mode": "random", "experiment": 2}, 25)["train"]
    names = [type(t).__name__ for t in d["common"]]
    rows.append([int("AffineNP" in names), int("CropNP" in names), int(any(type(t).__name__ == "PadNP" for t in d["img"]))])
out["lists"] = np.array(["+".join(k) for k in LISTS])
out["lists_affine_crop_pad"] = np.array(rows, dtype=np.int64)


def pattern(h, w):
    """low-entropy frames (the fixture stays a few KB): every pixel distinct enough that a wrong offset shows"""
    y, x = np.mgrid[0:h, 0:w]
    img = np.stack([(7 * y + 3 * x) % 256, (5 * y + 11 * x + 1) % 256, (13 * y + x + 2) % 256], axis=-1).astype(np.uint8)
    lbl = ((y // 3 + 2 * (x // 5)) % 25).astype(np.int32)
    return img, lbl


# CropNP('random'): size 0.4 on two frame sizes; a size that exceeds a dimension (the min(h, w) branch, and the horizontal randint range
# is empty); a square frame where both ranges are empty
CROPS = ((0.4, 80, 140, 5), (0.4, 160, 280, 6), (0.4, 160, 280, 7), (0.9, 80, 40, 8), (1.0, 64, 64, 9))
out["crop_cases"] = np.array(CROPS, dtype=np.float64)
for ci, (size, h, w, seed) in enumerate(CROPS):
    img, lbl = pattern(h, w)
    random.seed(seed)
    ic, lc, meta = CropNP(size, "random", 2)((img, lbl, {}))   # (experiment 2: CropNP.__init__ raises a KeyError for experiment 3)
    after = random.random()                          # pins how many draws the call consumed
    out["c%d_offsets" % ci] = np.array(meta["crop_offsets"], dtype=np.int64)
    out["c%d_px" % ci] = np.array(meta["crop_size"], dtype=np.int64)
    out["c%d_img" % ci], out["c%d_lbl" % ci] = ic, lc
    out["c%d_next_random" % ci] = np.array(after, dtype=np.float64)
    print("crop", size, h, w, meta["crop_offsets"], meta["crop_size"])
np.savez_compressed(os.path.join(HERE, "geometry.npz"), **out)
print("wrote geometry.npz %.1f KB" % (os.path.getsize(os.path.join(HERE, "geometry.npz")) / 1024))
