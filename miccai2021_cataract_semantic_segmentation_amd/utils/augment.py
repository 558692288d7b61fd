"""The PIL-based training augmentations of the reference's image pipeline, on the GPU and on uint8 batches.

Mirror of ``BlurPIL(probability=.05, kernel_limits=(3, 7))`` (utils/transforms.py:242-251) and torchvision's
``ColorJitter(brightness=(2/3, 1.5), contrast=(2/3, 1.5), saturation=(2/3, 1.5), hue=(-.05, .05))`` as the reference wires them
(utils/utils.py:412-417: after ``PadNP`` / ``FlipNP`` and ``ToPILImage``, before ``ToTensor``).  The kernels (csrc/augment.hip)
reproduce Pillow's integer / float arithmetic bit for bit (tests/golden/augment.npz is generated with Pillow);
the random draws happen on the host: ``sample_blur`` follows ``BlurPIL.__call__``'s numpy draws, ``sample_color_jitter`` the
order of torchvision >= 0.9 ``ColorJitter.get_params`` (torchvision is not installed here: that order is unpinned).

RandAugment's photometric subset (Identity, Brightness, Color, Contrast, Sharpness, Posterize, Solarize, AutoContrast, Equalize) runs on the
same kernels: ``sample_randaugment`` draws per frame and slot one entry and its magnitude, ``GpuAugment.color_ops`` applies any mix of the
op codes -1 ... 8 in one launch per slot (tests/golden/randaugment.npz is generated with Pillow).  Its draw order restates torchvision's
``RandAugment.forward`` and is unpinned for the same reason; its geometric entries are ``affine``'s business (labels move with them)."""
import math

import numpy as np
import torch

BRIGHTNESS, CONTRAST, SATURATION, HUE = 0, 1, 2, 3
AUTOCONTRAST, EQUALIZE, POSTERIZE, SOLARIZE, SHARPNESS = 4, 5, 6, 7, 8


def gaussian_box_params(radius):
    """(int radius, ww, fw) of libImaging/BoxBlur.c for ImageFilter.GaussianBlur(radius): three box passes per direction"""
    sigma2 = float(radius * radius) / 3
    L = math.sqrt(12.0 * sigma2 + 1.0)
    l = math.floor((L - 1.0) / 2.0)
    a = (2 * l + 1) * (l * (l + 1) - 3 * sigma2)
    a /= 6 * (sigma2 - (l + 1) * (l + 1))
    fr = np.float32(l + a)
    r = int(fr)
    ww = int(np.float32(1 << 24) / (fr * np.float32(2) + np.float32(1)))        # (UINT32)(1 << 24) / (floatRadius * 2 + 1): float arithmetic
    fw = ((1 << 24) - (r * 2 + 1) * ww) // 2
    return r, ww & 0xFFFFFFFF, fw & 0xFFFFFFFF


def sample_blur(batch, probability=0.05, kernel_limits=(3, 7), random=np.random):
    """BlurPIL.__call__'s draws per frame: one uniform, then (if it fires) np.random.randint(*kernel_limits); 0 = no blur"""
    radii = np.zeros(batch, dtype=np.int32)
    for i in range(batch):
        if random.random() < probability:
            radii[i] = random.randint(*kernel_limits)
    return radii


def pseudo_jitter_ranges(strength=2):
    """the ColorJitter arguments of the 'pseudo_colorjitter' transform keyword (utils/utils.py:419-436): (1 - 0.25 s, 1 + 0.25 s) for
    brightness, contrast and saturation, hue +-0.02 s; s in {1, 2, 3} ({'strength': s} in the transform list), default 2.  The reference
    wraps that ColorJitter in RandomApply(p=0.7): sample_color_jitter(..., apply_probability=PSEUDO_JITTER_PROBABILITY)"""
    s = 2 if strength is None else strength
    assert s in [1, 2, 3]
    extent = (1 - s * 0.25, 1 + s * 0.25)
    return {"brightness": extent, "contrast": extent, "saturation": extent, "hue": (-.02 * s, .02 * s)}


PSEUDO_JITTER_PROBABILITY = 0.7


def pseudo_jitter_strength(transform_list):
    """the strength the reference reads off its `transforms` config list (utils/utils.py:421-429): None without the 'pseudo_colorjitter'
    keyword, else the 'strength' of the first dict entry that has one (1, 2 or 3), default 2 -- for PinnedFrameLoader(pseudo_colorjitter=)"""
    if 'pseudo_colorjitter' not in transform_list:
        return None
    for e in transform_list:
        if isinstance(e, dict) and 'strength' in e:
            assert e['strength'] in [1, 2, 3]
            return e['strength']
    return 2


def sample_color_jitter(batch, brightness=(2 / 3, 1.5), contrast=(2 / 3, 1.5), saturation=(2 / 3, 1.5), hue=(-0.05, 0.05), generator=None,
                        apply_probability=None):
    """per frame: a permutation of the four operations, then one uniform factor each in the order brightness, contrast,
    saturation, hue (torchvision >= 0.9 ColorJitter.get_params).  Returns (orders int32 [B, 4], factors float64 [B, 4]).
    apply_probability = p: RandomApply([ColorJitter], p) -- one uniform per frame FIRST; where p is below it the frame is skipped:
    nothing else is drawn for it and its orders are -1, which GpuAugment.color_jitter treats as no operation"""
    orders = np.zeros((batch, 4), dtype=np.int32)
    factors = np.zeros((batch, 4), dtype=np.float64)
    for i in range(batch):
        if apply_probability is not None and apply_probability < float(torch.rand(1, generator=generator)):
            orders[i] = -1        # (RandomApply.forward: `if self.p < torch.rand(1): return img`)
            continue
        orders[i] = torch.randperm(4, generator=generator).numpy()
        for k, (lo, hi) in enumerate((brightness, contrast, saturation, hue)):
            factors[i, k] = float(torch.empty(1).uniform_(lo, hi, generator=generator))
    return orders, factors


def randaugment_space(bins=31):
    """torchvision's RandAugment._augmentation_space on the photometric subset, in its order: a list of (name, op code, magnitudes float64
    [bins] or None, signed).  Signed entries apply the factor 1 +- magnitude; Posterize's magnitude is the bit count, Solarize's the
    threshold.  The tables are computed as torchvision computes them (torch.linspace / arange in float32)"""
    bins = int(bins)
    unit = torch.linspace(0.0, 0.9, bins).double().numpy()
    bits = (8 - (torch.arange(bins) / ((bins - 1) / 4)).round().int()).double().numpy()
    threshold = torch.linspace(255.0, 0.0, bins).double().numpy()
    return [("Identity", -1, None, False), ("Brightness", BRIGHTNESS, unit, True), ("Color", SATURATION, unit, True),
            ("Contrast", CONTRAST, unit, True), ("Sharpness", SHARPNESS, unit, True), ("Posterize", POSTERIZE, bits, False),
            ("Solarize", SOLARIZE, threshold, False), ("AutoContrast", AUTOCONTRAST, None, False), ("Equalize", EQUALIZE, None, False)]


def sample_randaugment(batch, num_ops=2, magnitude=9, bins=31, generator=None, apply_probability=None):
    """per frame and slot: torch.randint(9, (1,)) picks the entry of randaugment_space; for the four signed entries only, torch.randint(2,
    (1,)) picks the sign (1 = negative), as torchvision's RandAugment.forward does (torchvision is not installed here: that order is
    unpinned).  Returns (ops int32 [B, num_ops], values float64 [B, num_ops]): the op codes of GpuAugment.color_ops and their parameters
    (enhance factor, bits, threshold; 0 where the operation takes none).
    apply_probability = p: one uniform per frame FIRST, as in sample_color_jitter; where p is below it nothing else is drawn for the frame
    and its codes are -1"""
    space = randaugment_space(bins)
    ops = np.full((batch, num_ops), -1, dtype=np.int32)
    values = np.zeros((batch, num_ops), dtype=np.float64)
    for i in range(batch):
        if apply_probability is not None and apply_probability < float(torch.rand(1, generator=generator)):
            continue
        for k in range(num_ops):
            _, code, magnitudes, signed = space[int(torch.randint(len(space), (1,), generator=generator))]
            m = float(magnitudes[magnitude]) if magnitudes is not None else 0.0
            if signed:
                if int(torch.randint(2, (1,), generator=generator)):
                    m = -m
                m = 1.0 + m
            ops[i, k], values[i, k] = code, m
    return ops, values


RANDAUGMENT_DEFAULTS = {"num_ops": 2, "magnitude": 9, "bins": 31, "p": None, "frames": "all"}


def check_randaugment(config):
    """the 'randaugment' dict with its defaults filled in ({num_ops, magnitude, bins, p, frames: "all" | "pseudo"}); True / None / {} = the
    defaults.  ValueError, quoting the value, for unknown keys, magnitude outside [0, bins), num_ops < 1, p outside [0, 1], other frames"""
    config = {} if config is None or config is True else config
    if not isinstance(config, dict):
        raise ValueError("randaugment: expected a dict {num_ops, magnitude, bins, p, frames}, got %r" % (config,))
    unknown = sorted(set(config) - set(RANDAUGMENT_DEFAULTS))
    if unknown:
        raise ValueError("randaugment: unknown keys %r (known: %s)" % (unknown, ", ".join(RANDAUGMENT_DEFAULTS)))
    c = dict(RANDAUGMENT_DEFAULTS, **config)
    for key in ("num_ops", "magnitude", "bins"):
        if isinstance(c[key], bool) or not isinstance(c[key], (int, np.integer)):
            raise ValueError("randaugment: %s must be an integer, got %r" % (key, c[key]))
    if c["num_ops"] < 1:
        raise ValueError("randaugment: num_ops must be at least 1, got %r" % (c["num_ops"],))
    if c["bins"] < 2:
        raise ValueError("randaugment: bins must be at least 2, got %r" % (c["bins"],))
    if not 0 <= c["magnitude"] < c["bins"]:
        raise ValueError("randaugment: magnitude must lie in [0, bins = %d), got %r" % (c["bins"], c["magnitude"]))
    if c["p"] is not None and (isinstance(c["p"], bool) or not isinstance(c["p"], (int, float)) or not 0 <= c["p"] <= 1):
        raise ValueError("randaugment: p must be None or lie in [0, 1], got %r" % (c["p"],))
    if c["frames"] not in ("all", "pseudo"):
        raise ValueError("randaugment: frames must be 'all' or 'pseudo', got %r" % (c["frames"],))
    return c


def randaugment_from_transforms(transform_list, transform_values=None):
    """None without the 'randaugment' keyword in the `transforms` config list, else transform_values['randaugment'] checked and completed
    (check_randaugment) -- for PinnedFrameLoader(randaugment=)"""
    if 'randaugment' not in transform_list:
        return None
    return check_randaugment((transform_values or {}).get('randaugment'))


class GpuAugment:
    """``blur(img_u8 [B,H,W,3], radii)``, ``color_jitter(img_u8, orders, factors)`` and ``color_ops(img_u8, ops, values)`` on device tensors;
    all return new tensors"""

    def __init__(self, device="cuda"):
        self.device = torch.device(device)

    def _dev(self, a, dtype):
        return torch.as_tensor(np.ascontiguousarray(a), dtype=dtype).to(self.device, non_blocking=True)

    def blur(self, img, radii):
        from .. import ops
        radii = np.asarray(radii)
        if not (radii > 0).any():
            return img
        prm = np.array([gaussian_box_params(int(r)) if r > 0 else (-1, 0, 0) for r in radii], dtype=np.int64)
        return ops.aug_gaussian_blur(img, self._dev(prm[:, 0], torch.int32), self._dev(prm[:, 1].astype(np.uint32).view(np.int32), torch.int32),
                                     self._dev(prm[:, 2].astype(np.uint32).view(np.int32), torch.int32))

    def color_jitter(self, img, orders, factors):
        from .. import ops
        orders, factors = np.asarray(orders), np.asarray(factors, dtype=np.float64)
        out = img.clone()
        for step in range(orders.shape[1]):
            op = orders[:, step].astype(np.int32)
            f = np.array([factors[b, o] if o >= 0 else 0.0 for b, o in enumerate(op)], dtype=np.float64)
            hue = op == HUE
            f[hue] = [float(int(v * 255) & 0xFF) for v in f[hue]]      # np.uint8(hue_factor * 255): truncation in double, uint8 wrap-around
            ops.aug_color_op(out, self._dev(op, torch.int32), self._dev(f.astype(np.float32), torch.float32))
        return out

    def color_ops(self, img, ops_, values):
        """ops_ int [B, n], values [B, n]: per image and step one op code -1 ... 8 (-1 = none) and its parameter -- the enhance factor
        (brightness, contrast, saturation, sharpness), the hue factor (converted as color_jitter does), the bits (posterize), the threshold
        (solarize).  One aug_color_op launch per step; its workspace follows the codes of the step: without a code >= 4 it is color_jitter's,
        so such calls stay the launches they are today"""
        from .. import ops
        ops_, values = np.asarray(ops_), np.asarray(values, dtype=np.float64)
        if ops_.ndim != 2 or ops_.shape != values.shape or ops_.shape[0] != img.shape[0]:
            raise ValueError("color_ops: ops and values must both be [B = %d, n], got %s and %s" % (img.shape[0], ops_.shape, values.shape))
        if ops_.size and (ops_.min() < -1 or ops_.max() > SHARPNESS):
            raise ValueError("color_ops: op codes must lie in -1 ... %d, got [%d, %d]" % (SHARPNESS, ops_.min(), ops_.max()))
        out = img.clone()
        for step in range(ops_.shape[1]):
            op = ops_[:, step].astype(np.int32)
            if not (op >= 0).any():
                continue
            f = values[:, step].copy()
            hue = op == HUE
            f[hue] = [float(int(v * 255) & 0xFF) for v in f[hue]]
            extended = "full" if (op == SHARPNESS).any() else ("lut" if (op >= AUTOCONTRAST).any() else None)
            ops.aug_color_op(out, self._dev(op, torch.int32), self._dev(f.astype(np.float32), torch.float32), extended=extended)
        return out
