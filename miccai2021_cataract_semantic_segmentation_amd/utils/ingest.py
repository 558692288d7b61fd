"""Raw CaDIS frames -> network input on the GPU (one HIP kernel per batch).

Mirror of what ``DatasetFromDF.__getitem__`` (datasets/Dataset_from_df.py:31-69 of the reference) does per frame on the
host: ``remap_mask(..., to_network=True)`` (utils/utils.py:23-47), ``FlipNP`` (utils/transforms.py:222-240),
``PadNP(ver=(2, 2), hor=(0, 0), 'reflect')`` (utils/transforms.py:8-20, wired at utils/utils.py:394-401), ``ToTensor`` and the
optional ``Normalize`` (utils/utils.py:440-447); optionally the PIL blur / colour jitter between pad and ToTensor (utils/augment.py).
The affine / crop augmentations (``AffineNP`` with crop_to_fit=False, ``CropNP`` 'random': utils/transforms.py:23-105, 254-303) run in the
same launch (csrc/warp.hip): ``GpuIngest(...)(..., affine=matrices, crop=(origins, px))``, parameters drawn by utils/geometry.py.
``CropNP`` 'freq' (:282-293) picks its origins from the warped labels on the device first (csrc/cropfreq.hip):
``crop={"mode": "freq", "u": uniforms, "px": px, "table": integer class weights}``; they never visit the host."""
import numpy as np
import torch

from .classes import CLASS_REMAP

TORCHVISION_MEAN, TORCHVISION_STD = [0.485, 0.456, 0.406], [0.229, 0.224, 0.225]   # utils/utils.py:445-447


def remap_lut(experiment):
    """256-entry table equal to remap_mask(mask, CLASS_INFO[experiment][0], to_network=True) (utils/utils.py:23-47)"""
    remap = CLASS_REMAP[experiment]
    lut = np.full(256, 255, dtype=np.uint8)
    for key, raw in remap.items():
        for v in raw:
            lut[v] = key
    lut[lut == 255] = len(remap) - 1
    return lut


def sample_flips(batch, probability=(0.0, 0.5), random=np.random):
    """FlipNP's draws (utils/transforms.py:227-239): per frame one uniform for the vertical, then one for the horizontal
    flip.  Returns int32 flags, bit 0 = horizontal, bit 1 = vertical."""
    flags = np.zeros(batch, dtype=np.int32)
    for i in range(batch):
        if random.random() < probability[0]:
            flags[i] |= 2
        if random.random() < probability[1]:
            flags[i] |= 1
    return flags


def label_tables_of(experiment):
    """uint8 [2, 256]: row 0 = remap_lut(experiment) (raw CaDIS ids -> network ids), row 1 = the identity (label maps that hold network ids
    already: pseudo labels, DatasetFromDF(labels_remaped=True), datasets/Dataset_from_df.py:49-53)"""
    return np.stack([remap_lut(experiment), np.arange(256, dtype=np.uint8)])


def check_label_tables(label_tables, batch, tables=2):
    """a per-frame table index as the ingest launches take it: HOST integers [batch] in [0, tables) -> int32 array (ValueError otherwise;
    the kernels clamp regardless, but a clamped index is a wrong label map, not a fault)"""
    t = np.asarray(label_tables)
    if t.dtype == np.bool_ or not np.issubdtype(t.dtype, np.integer):
        raise ValueError("label_tables must be integers (one table row per frame), got dtype %s" % t.dtype)
    if t.shape != (batch,):
        raise ValueError("label_tables must hold one table row per frame: shape (%d,), got %s" % (batch, t.shape))
    if t.size and (t.min() < 0 or t.max() >= tables):
        raise ValueError("label_tables must lie in [0, %d), got [%d, %d]" % (tables, int(t.min()), int(t.max())))
    return np.ascontiguousarray(t, dtype=np.int32)


def _jitters(jitter):
    """jitter: None, one (orders, factors) pair, or a list of pairs applied in turn (colorjitter, then pseudo_colorjitter); photometric=
    takes the same forms with (ops, values) pairs"""
    if jitter is None:
        return []
    return list(jitter) if isinstance(jitter, list) else [jitter]


class GpuIngest:
    """``ingest(img_u8 [B,H,W,3], lbl_u8 [B,H,W], flips) -> (x float32 [B,3,H',W], labels int64 [B,H',W])``"""

    def __init__(self, experiment, pad=(2, 2), normalise=False, device="cuda"):
        self.device = torch.device(device)
        self.pad = pad
        self.luts = torch.from_numpy(label_tables_of(experiment)).to(self.device)     # [2, 256]
        self.lut = self.luts[0]
        self.mean = torch.tensor(TORCHVISION_MEAN, device=self.device) if normalise else None
        self.std = torch.tensor(TORCHVISION_STD, device=self.device) if normalise else None

    def __call__(self, img, lbl, flips=None, nhwc4=False, blur_radii=None, jitter=None, affine=None, crop=None, label_tables=None,
                 photometric=None):
        """label_tables: HOST int [B] (None = 0 everywhere), per frame 0 = the label map holds raw CaDIS ids and is remapped, 1 = it holds
        network ids already (a pseudo-labelled frame) and passes through: a mixed batch is still one launch.
        affine: float64 [B,3,3] frame -> canvas matrices (utils.geometry.sample_affine): the frame is warped onto the reference's
        2H x 2W canvas; crop: (origins int32 [B,2] = (v, h), px) (utils.geometry.crop_px / sample_crops): only that px x px window of
        the canvas (without an affine: of the frame) is computed, and -- the reference's pad rule -- the rows are not padded.
        crop may also be {"mode": "freq", "u": float64 [B] (utils.geometry.sample_freq_u), "px": px, "table": the integer class weights of
        utils.geometry.freq_weight_table, or ops.crop_freq_table of them}: the origins are picked on the device from the warped labels
        (CropNP 'freq'; needs lbl) by two small launches ahead of the ingest's, on the same stream.
        blur_radii: per-frame GaussianBlur radius (0 = none; utils.augment.sample_blur); jitter: (orders, factors) of
        utils.augment.sample_color_jitter, or a list of such pairs applied in turn.  With either, the image takes the reference's order of operations on uint8
        (flip + reflect pad -> blur -> colour jitter -> ToTensor / Normalize: utils/utils.py:394-447) in a few more kernels.
        photometric: (ops, values) of utils.augment.sample_randaugment (any op codes -1 ... 8 of GpuAugment.color_ops), or a list of such
        pairs; applied after jitter, on the same uint8 frames."""
        img = img.to(self.device, non_blocking=True) if img is not None else None
        lbl = lbl.to(self.device, non_blocking=True) if lbl is not None else None
        if flips is not None:
            flips = torch.as_tensor(np.asarray(flips, dtype=np.int32)).to(self.device, non_blocking=True)
        ref = img if img is not None else lbl
        lut = tables = None
        if label_tables is not None and lbl is not None:
            tables = torch.from_numpy(check_label_tables(label_tables, int(ref.shape[0]), int(self.luts.shape[0]))).to(self.device, non_blocking=True)
        lut = self.luts if tables is not None else self.lut
        from .. import ops   # needs libcatseg_hip.so; the table / flag helpers above do not
        if affine is not None or crop is not None:
            return self._warped(ops, img, lbl, flips, nhwc4, blur_radii, jitter, affine, crop, lut, tables, photometric)
        if img is not None and (blur_radii is not None or jitter is not None or photometric is not None):
            from .augment import GpuAugment
            aug = GpuAugment(self.device)
            u8 = ops.aug_pad_flip_u8(img.contiguous(), flips, self.pad[0], self.pad[1])
            if blur_radii is not None:
                u8 = aug.blur(u8, blur_radii)
            for orders, factors in _jitters(jitter):
                u8 = aug.color_jitter(u8, orders, factors)
            for codes, values in _jitters(photometric):
                u8 = aug.color_ops(u8, codes, values)
            x = ops.ingest_u8(u8, None, self.lut, None, 0, 0, self.mean, self.std, nhwc4=nhwc4)[0]
            labels = ops.ingest_u8(None, lbl, lut, flips, self.pad[0], self.pad[1], self.mean, self.std, tables=tables)[1] if lbl is not None \
                else None
            return x, labels
        return ops.ingest_u8(img, lbl, lut, flips, self.pad[0], self.pad[1], self.mean, self.std, nhwc4=nhwc4, tables=tables)

    def _warped(self, ops, img, lbl, flips, nhwc4, blur_radii, jitter, affine, crop, lut, tables, photometric=None):
        """one warp launch for image and labels; with blur / jitter / photometric the image leaves it as uint8 and goes on as in __call__"""
        from .geometry import affine_inverse
        ref = img if img is not None else lbl
        H, W = int(ref.shape[1]), int(ref.shape[2])
        minv = affine_inverse(affine) if affine is not None else None
        canvas = (2 * H, 2 * W) if affine is not None else (H, W)
        if isinstance(crop, dict):
            from .geometry import freq_m53
            if crop.get("mode") != "freq" or lbl is None:
                raise ValueError("GpuIngest: a crop given as a dict is the 'freq' form {'mode': 'freq', 'u', 'px', 'table'} and needs labels")
            origin = ops.crop_freq_pick(lbl.contiguous(), lut, flips, minv, canvas, int(crop["px"]), crop["table"], freq_m53(crop["u"]),
                                        tables=tables)
            window = (int(crop["px"]), int(crop["px"]))
        else:
            origin, window = (crop[0], (int(crop[1]), int(crop[1]))) if crop is not None else (None, canvas)
        pad = self.pad if crop is None else (0, 0)          # utils/utils.py:396: padding only if no cropping has happened
        staged = img is not None and (blur_radii is not None or jitter is not None or photometric is not None)
        form = "u8" if staged else ("nhwc4" if nhwc4 else "nchw")
        out = ops.ingest_warp_u8(img.contiguous() if img is not None else None, lbl.contiguous() if lbl is not None else None, lut, flips,
                                 minv, canvas, origin, window, pad[0], pad[1], self.mean, self.std, outputs=(form,), tables=tables)
        x = out.get(form)
        if staged:
            from .augment import GpuAugment
            aug = GpuAugment(self.device)
            if blur_radii is not None:
                x = aug.blur(x, blur_radii)
            for orders, factors in _jitters(jitter):
                x = aug.color_jitter(x, orders, factors)
            for codes, values in _jitters(photometric):
                x = aug.color_ops(x, codes, values)
            x = ops.ingest_u8(x, None, self.lut, None, 0, 0, self.mean, self.std, nhwc4=nhwc4)[0]
        return x, out["labels"]
