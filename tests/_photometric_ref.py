"""numpy restatement of the five RandAugment photometric operations that csrc/augment.hip serves behind catseg_aug_color_op (op codes
4 ... 8), as Pillow computes them on RGB uint8 images [H, W, 3]: ImageOps.autocontrast (cutoff 0), ImageOps.equalize, ImageOps.posterize,
ImageOps.solarize, ImageEnhance.Sharpness.  tests/test_randaugment_cpu.py holds it against Pillow itself; the GPU tests use it at the
sizes the fixture does not cover.  The four ColorJitter operations (codes 0 ... 3) are oracle/augment.py's."""
import numpy as np

AUTOCONTRAST, EQUALIZE, POSTERIZE, SOLARIZE, SHARPNESS = 4, 5, 6, 7, 8


def _band_luts(a, lut_of):
    out = np.empty_like(a)
    for c in range(a.shape[-1]):
        h = np.bincount(a[..., c].ravel(), minlength=256)
        out[..., c] = lut_of(h).astype(np.uint8)[a[..., c]]
    return out


def _autocontrast_lut(h):
    nz = np.nonzero(h)[0]
    lo, hi = int(nz[0]), int(nz[-1])
    if hi <= lo:
        return np.arange(256)
    scale = 255.0 / (hi - lo)                 # double arithmetic, two roundings per entry (plain x86-64 code)
    offset = -lo * scale
    return np.array([min(255, max(0, int(i * scale + offset))) for i in range(256)])


def _equalize_lut(h):
    nzv = h[h > 0]
    if len(nzv) <= 1:
        return np.arange(256)
    step = (int(h.sum()) - int(nzv[-1])) // 255
    if step == 0:
        return np.arange(256)
    lut = np.empty(256, dtype=np.int64)
    n = step // 2
    for i in range(256):
        lut[i] = min(255, n // step)          # (the point table is clipped to a byte)
        n += int(h[i])
    return lut


def autocontrast(a):
    return _band_luts(a, _autocontrast_lut)


def equalize(a):
    return _band_luts(a, _equalize_lut)


def posterize(a, bits):
    return a & np.uint8((0xFF << (8 - int(bits))) & 0xFF)


def solarize(a, threshold):
    return np.where(a < threshold, a, 255 - a).astype(np.uint8)


def smooth(a):
    """ImageFilter.SMOOTH (libImaging/Filter.c, 3 x 3): float32 weights (1,1,1, 1,5,1, 1,1,1) / 13; per channel ss = 0.5, then the nine
    products are added in float32 (no contraction), kernel rows top to bottom; clip8((int)ss); the one-pixel border keeps the source"""
    H, W, _ = a.shape
    out = a.copy()
    if H < 3 or W < 3:
        return out
    k = (np.array([1, 1, 1, 1, 5, 1, 1, 1, 1], dtype=np.float32) / np.float32(13)).astype(np.float32)
    f = a.astype(np.float32)
    ss = np.full((H - 2, W - 2, a.shape[2]), np.float32(0.5), dtype=np.float32)
    for dy in range(3):
        for dx in range(3):
            ss = ss + f[dy:dy + H - 2, dx:dx + W - 2] * k[dy * 3 + dx]
    out[1:-1, 1:-1] = np.clip(ss.astype(np.int64), 0, 255).astype(np.uint8)
    return out


def blend(deg, img, f):
    """Image.blend(deg, img, f) (libImaging/Blend.c): float32, product rounded before the add; truncation inside [0, 1], clipped outside"""
    d, i, f = deg.astype(np.float32), img.astype(np.float32), np.float32(f)
    t = d + f * (i - d)
    if 0 <= f <= 1:
        return t.astype(np.uint8)
    return np.where(t <= 0, 0, np.where(t >= 255, 255, t)).astype(np.uint8)


def sharpness(a, f):
    return blend(smooth(a), a, f)


def apply(a, op, value):
    """one operation by its code, -1 ... 8 (codes 0 ... 3: oracle.augment.adjust with the enhance factor / hue factor itself)"""
    if op < 0:
        return a.copy()
    if op < 4:
        from oracle import augment as A
        return A.adjust(a, int(op), float(value))
    return {AUTOCONTRAST: lambda: autocontrast(a), EQUALIZE: lambda: equalize(a), POSTERIZE: lambda: posterize(a, int(value)),
            SOLARIZE: lambda: solarize(a, np.float32(value)), SHARPNESS: lambda: sharpness(a, value)}[int(op)]()
