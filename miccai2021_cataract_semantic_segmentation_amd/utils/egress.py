"""Network output -> label images and coloured uint8 frames on the GPU (one HIP kernel per batch): the counterpart of ``GpuIngest``.

Mirror of what the reference does per frame on the host after the forward pass (managers/BaseManager.py:690-741): ``argmax(Softmax2d(out))``,
``mask_to_colormap(..., from_network=True)`` (utils/utils.py:114-142), ``np.round(frame * 255)`` and the side-by-side concatenation
(``to_comb_image`` utils/utils.py:202-211), plus ``clipped_argmax`` (utils/torch_utils.py:7-21), the confidence-thresholded pseudo-labels.
The table functions (palette, remapped colour map, network id -> dataset id) and the numpy forms of the mapping functions need no library;
with CUDA tensors the same names go through ``ops.egress_u8``."""
import numpy as np
import torch

from .classes import CADIS_PALETTE, CLASS_REMAP, NUM_CLASSES
from .ingest import TORCHVISION_MEAN, TORCHVISION_STD


def get_cadis_colormap():
    """utils/utils.py:67-111: the 36 RGB colours of the raw CaDIS classes"""
    return np.asarray(CADIS_PALETTE)


def get_remapped_colormap(class_remapping):
    """utils/utils.py:50-64: {remapped class: colour of its first raw id}; key 255 (ignored) is black"""
    colormap = get_cadis_colormap()
    return {key: ([0, 0, 0] if key == 255 else colormap[val[0]]) for key, val in class_remapping.items()}


def network_ignore_id(experiment):
    """the network id mask_from_network sends to 255 (utils/utils.py:121-122: len(CLASS_INFO[experiment][1]) - 1), None for experiment 1"""
    return NUM_CLASSES[experiment] if experiment in (2, 3) else None


def network_lut(experiment):
    """256-entry table equal to mask_from_network (utils/utils.py:114-123): identity, the ignore id of experiments 2 and 3 -> 255"""
    lut = np.arange(256, dtype=np.uint8)
    if network_ignore_id(experiment) is not None:
        lut[network_ignore_id(experiment)] = 255
    return lut


def palette_table(colormap, bgr=False):
    """uint8 [256, 3]: the colour of each id of a {id: colour} map in the output channel order; ids the map does not name stay 0"""
    pal = np.zeros((256, 3), dtype=np.uint8)
    for key, colour in colormap.items():
        pal[int(key)] = np.asarray(colour, dtype=np.uint8)
    return np.ascontiguousarray(pal[:, ::-1]) if bgr else pal


def _is_cuda(x):
    return isinstance(x, torch.Tensor) and x.is_cuda


def _rows_of(nchw):
    """NCHW logits -> the NHWC view the kernels read (the engine's outputs already are NHWC memory: no copy)"""
    rows = nchw.permute(0, 2, 3, 1)
    B, H, W, _ = rows.shape
    if rows.dtype != torch.float32 or rows.stride(-1) != 1 or not (H == 1 or W == 1 or rows.stride(1) == W * rows.stride(2)) or \
            not (B == 1 or rows.stride(0) == H * W * rows.stride(2)):
        rows = rows.float().contiguous()
    return rows


def mask_from_network(mask, experiment):
    """utils/utils.py:114-123 (in place, as the reference): the network's ignore id of experiments 2 and 3 becomes 255"""
    if experiment == 2 or experiment == 3:
        mask[mask == network_ignore_id(experiment)] = 255
    return mask


def mask_to_colormap(mask, colormap, from_network=None, experiment=None):
    """utils/utils.py:126-142: [H, W] (or [B, H, W]) ids -> uint8 [..., 3].  numpy in, numpy out; a CUDA tensor goes through the egress
    kernel's target panel and comes back as a CUDA tensor (the mask itself is left as it was)."""
    if _is_cuda(mask):
        from .. import ops
        m = mask.long()
        m = (m[None] if m.dim() == 2 else m).contiguous()
        lut = torch.from_numpy(network_lut(experiment if from_network else 1)).to(mask.device)
        pal = torch.from_numpy(palette_table(colormap)).to(mask.device)
        canvas = ops.egress_u8(None, lut=lut, palette=pal, target=m)[2]
        return canvas[0] if mask.dim() == 2 else canvas
    if from_network:
        mask = mask_from_network(mask, experiment)
    return palette_table(colormap)[np.asarray(mask).astype(np.uint8)] if _fits_u8(mask) else _colour_loop(mask, colormap)


def _fits_u8(mask):
    m = np.asarray(mask)
    return m.size == 0 or (m.min() >= 0 and m.max() <= 255)


def _colour_loop(mask, colormap):
    mask = np.asarray(mask)
    rgb = np.zeros(mask.shape + (3,), dtype=np.uint8)
    for label, colour in colormap.items():
        rgb[mask == label] = colour
    return rgb


def to_comb_image(img, lbl, lbl_pred, experiment):
    """utils/utils.py:202-211: img float [3, H, W] in [0, 1], lbl and lbl_pred [H, W] network ids -> uint8 [H, 3 W, 3] RGB
    image | ground truth | prediction.  CUDA tensors stay on the device (from logits, GpuEgress writes the three panels in one launch)."""
    colormap = get_remapped_colormap(CLASS_REMAP[experiment])
    if _is_cuda(img):
        from .. import ops
        lut = torch.from_numpy(network_lut(experiment)).to(img.device)
        pal = torch.from_numpy(palette_table(colormap)).to(img.device)
        left = ops.egress_u8(None, lut=lut, palette=pal, frame=img.float()[None].contiguous(), target=lbl.long()[None].contiguous())[2]
        right = ops.egress_u8(None, lut=lut, palette=pal, target=lbl_pred.long()[None].contiguous())[2]
        return torch.cat((left, right), dim=2)[0]
    img, lbl, lbl_pred = (t.detach().cpu().numpy() if isinstance(t, torch.Tensor) else np.asarray(t) for t in (img, lbl, lbl_pred))
    img = np.round(np.moveaxis(img, 0, -1) * 255).astype("uint8")
    lbl = mask_to_colormap(lbl, colormap, from_network=True, experiment=experiment)
    lbl_pred = mask_to_colormap(lbl_pred, colormap, from_network=True, experiment=experiment)
    return np.concatenate((img, lbl, lbl_pred), axis=1)


def clipped_argmax(softmax_pred, t, ignore_value):
    """utils/torch_utils.py:7-21: [N, C, H, W] probabilities -> [N, H, W] int64 argmax, ignore_value where the maximum is < t"""
    assert (0 <= t < 1), "threshold must be in [0,1) instead got {}".format(t)
    assert (ignore_value)
    if _is_cuda(softmax_pred):
        from .. import ops
        return ops.egress_u8(_rows_of(softmax_pred), probs=True, threshold=t, ignore_value=ignore_value, want_i64=True, want_canvas=False)[0]
    scores, indices = torch.max(softmax_pred, dim=1)
    return torch.where(scores < t, torch.full_like(indices, ignore_value), indices)


class GpuEgress:
    """``egress(out [B,K,H,W], frame, target) -> {"canvas": uint8 [B,H',n_panels*W,3], "labels": int64 [B,H',W], "labels_u8": uint8 [B,H',W]}``

    crop: rows dropped at the top / bottom (the inverse of the ingest's PadNP(ver=(2, 2))); bgr: channel order of the canvas;
    threshold / ignore_value: clipped_argmax on the softmax score (ignore_value defaults to the experiment's ignore id);
    normalised: the frames carry torchvision's Normalize, undone before the bytes are taken (un_normalise, utils/utils.py:453).
    The tables live on the device from construction on."""

    def __init__(self, experiment, crop=(2, 2), bgr=False, threshold=None, ignore_value=None, normalised=False, device="cuda"):
        self.device = torch.device(device)
        self.experiment, self.crop, self.bgr = experiment, tuple(crop), bool(bgr)
        self.threshold = float(threshold) if threshold else 0.0
        if ignore_value is None:
            ignore_value = NUM_CLASSES[experiment]
        self.ignore_value = int(ignore_value)
        self.lut = torch.from_numpy(network_lut(experiment)).to(self.device)
        self.palette = torch.from_numpy(palette_table(get_remapped_colormap(CLASS_REMAP[experiment]), bgr=self.bgr)).to(self.device)
        self.mean = TORCHVISION_MEAN if normalised else None
        self.std = TORCHVISION_STD if normalised else None

    def __call__(self, out, frame=None, target=None, want=("canvas",), probs=False):
        """out: NCHW logits, or probabilities (the Ensemble's output) with probs=True; frame: float NCHW or NHWC-4; target: [B, H, W] network
        ids.  Returns the one tensor asked for, or a tuple in the order of `want` (names: 'canvas', 'labels', 'labels_u8')."""
        from .. import ops   # needs libcatseg_hip.so; the table functions above do not
        want = (want,) if isinstance(want, str) else tuple(want)
        assert want and set(want) <= {"canvas", "labels", "labels_u8"}, want
        if frame is not None:
            frame = frame.to(self.device).float().contiguous()
        if target is not None:
            target = target.to(self.device).long().contiguous()
        li, lu, canvas = ops.egress_u8(_rows_of(out), probs=probs, crop=self.crop, threshold=self.threshold, ignore_value=self.ignore_value,
                                       lut=self.lut, palette=self.palette, frame=frame if "canvas" in want else None,
                                       mean=self.mean if frame is not None and "canvas" in want else None,
                                       std=self.std if frame is not None and "canvas" in want else None, bgr=self.bgr,
                                       target=target if "canvas" in want else None, want_i64="labels" in want, want_u8="labels_u8" in want,
                                       want_canvas="canvas" in want)
        got = {"canvas": canvas, "labels": li, "labels_u8": lu}
        return got[want[0]] if len(want) == 1 else tuple(got[w] for w in want)
