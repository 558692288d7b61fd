"""Fixtures for RandAugment's photometric operations beyond ColorJitter's (autocontrast, equalize, posterize, solarize, sharpness), generated
with Pillow itself.  Run in the build container:  python tests/golden/make_golden_randaugment.py   -> tests/golden/randaugment.npz
(torchvision is not installed: the operations are spelled out with the PIL calls torchvision.transforms.functional makes for PIL images)"""
import os

import numpy as np
import PIL
from PIL import Image, ImageEnhance, ImageOps

from make_golden_augment import tv_adjust

HERE = os.path.dirname(os.path.abspath(__file__))
POSTERIZE_BITS = (1, 4, 7, 8)
SOLARIZE_T = (0, 93.5, 178.5, 255, 256)
SHARPNESS_F = (0.1, 0.55, 1.0, 1.45, 1.9)


def pil_op(img, op, value):
    """op codes of utils/augment.py: -1 none, 0 ... 3 ColorJitter's, 4 autocontrast, 5 equalize, 6 posterize, 7 solarize, 8 sharpness"""
    if op < 0:
        return img
    if op < 4:
        return tv_adjust(img, op, value)
    if op == 4:
        return ImageOps.autocontrast(img)
    if op == 5:
        return ImageOps.equalize(img)
    if op == 6:
        return ImageOps.posterize(img, int(value))
    if op == 7:
        return ImageOps.solarize(img, value)
    return ImageEnhance.Sharpness(img).enhance(value)


def main():
    rng = np.random.default_rng(11)
    out = {"pil_version": np.array(PIL.__version__)}
    imgs = np.empty((3, 40, 56, 3), dtype=np.uint8)
    imgs[0] = rng.integers(0, 256, (40, 56, 3), dtype=np.uint8)                    # uniform
    imgs[1] = (rng.random((40, 56, 3)) ** 4 * 255).astype(np.uint8)                # skewed: long empty tail of the histogram
    imgs[2] = rng.integers(40, 200, (40, 56, 3), dtype=np.uint8)                   # a constant band plus 0 / 255 pixels
    imgs[2, ..., 1] = 77
    imgs[2, 3, 5], imgs[2, 17, 20, 0], imgs[2, 39, 55, 2] = (0, 77, 255), 255, 0
    tiny = rng.integers(0, 256, (2, 2, 7, 3), dtype=np.uint8)                      # no interior pixel; fewer than 255 pixels
    # per batch ONE array [case][image][H][W][3], case 0 = the input itself; the cases whose output equals the input follow it directly, so that
    # the archive's deflate window (32 KB > one batch) finds them as repeats
    cases = [("posterize_8", 6, 8), ("solarize_256", 7, 256), ("sharpness_1.0", 8, 1.0), ("autocontrast", 4, 0.0), ("equalize", 5, 0.0)]
    cases += [("posterize_%d" % b, 6, b) for b in POSTERIZE_BITS if b != 8]
    cases += [("solarize_%s" % t, 7, t) for t in SOLARIZE_T if t != 256]
    cases += [("sharpness_%s" % f, 8, f) for f in SHARPNESS_F if f != 1.0]
    out["case_names"] = np.array(["input"] + [c[0] for c in cases])
    out["case_ops"] = np.array([-1] + [c[1] for c in cases])
    out["case_values"] = np.array([0.0] + [float(c[2]) for c in cases])
    for name, batch in (("imgs", imgs), ("tiny", tiny)):
        out[name] = np.stack([batch] + [np.stack([np.asarray(pil_op(Image.fromarray(im), op, value)) for im in batch]) for _, op, value in cases])
    # one three-step sequence, a different operation per image and step, legacy and new codes mixed (hue values are hue factors)
    seq_ops = np.array([[1, 5, 8], [8, 3, 4], [7, -1, 2]])
    seq_values = np.array([[1.31, 0.0, 1.73], [0.46, -0.04, 0.0], [178.5, 0.0, 1.27]])
    seq = []
    for im, ops, values in zip(imgs, seq_ops, seq_values):
        p = Image.fromarray(im)
        for op, v in zip(ops, values):
            p = pil_op(p, int(op), float(v))
        seq.append(np.asarray(p))
    out["seq_ops"], out["seq_values"], out["seq_out"] = seq_ops, seq_values, np.stack(seq)
    path = os.path.join(HERE, "randaugment.npz")
    np.savez_compressed(path, **out)
    print("wrote randaugment.npz with", len(out), "arrays,", os.path.getsize(path), "bytes, Pillow", PIL.__version__)


if __name__ == "__main__":
    main()
