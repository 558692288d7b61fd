"""SoftIoU and GenDiceLoss -- losses/SoftIoU.py and losses/GenDiceLoss.py of the reference (same constructor keys, defaults and
arithmetic), computed by the fused HIP kernels of csrc/overlap.hip: one streaming pass forward (softmax, per-class sums, fp64
finalize into per-class gradient coefficients), one backward (softmax recomputed, multiplied by autograd's upstream scalar).

Classes: c = 8 (experiment 1) or 17 / 25 (experiments 2 / 3, whose 'ignore' one-hot column is dropped: a pixel labelled 17 / 25 enters
sum_p p_pc -- the union, the divisor -- but not the intersection, the dividend).

Two documented divergences from the reference:
  * invalid labels -- anything outside [0, c) other than the ignore label of experiments 2 / 3 -- make the reference raise (scatter out
    of bounds).  On the device that would need a host sync, so such pixels are dropped instead: they add nothing to any sum (zero loss
    contribution, zero gradient row).  The last call's count is the device tensor ``invalid_labels``.
  * when the non-naive mean excludes a class (union / divisor exactly 0), the reference's autograd evaluates 0 / 0 in the backward of the
    division and every logit gradient becomes nan; here the excluded class contributes zero gradient (the derivative of the loss as
    written).  The loss values, and every naive-form nan, are the reference's.
"""
import torch
from torch import nn

from .. import ops
from ..utils import IGNORE_LABEL, NUM_CLASSES
from ._common import as_pixel_rows

_CLASS_INFO_LEN = {1: 8, 2: 18, 3: 26}     # len(CLASS_INFO[experiment][1]) of the reference (its num_classes, ignore class included)


class _OverlapFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, pred, target, kind, ignore, naive, weight_mode, weights, out):
        rows = as_pixel_rows(pred.detach())
        lbl = target.reshape(-1)
        if lbl.dtype != torch.int64:
            lbl = lbl.long()
        lbl = lbl.contiguous()
        loss, coef, invalid = ops.overlap_fwd(rows, lbl, kind, ignore, naive, weight_mode, weights)
        out["invalid_labels"] = invalid
        ctx.rows, ctx.lbl, ctx.coef = (rows, lbl, coef) if pred.requires_grad else (None, None, None)
        ctx.ignore, ctx.shape = ignore, pred.shape
        return loss.reshape(())

    @staticmethod
    def backward(ctx, g):
        up = g.reshape(1)
        if up.dtype != torch.float32 or not up.is_contiguous():
            up = up.float().contiguous()
        dl = ops.overlap_bwd(ctx.rows, ctx.lbl, ctx.coef, up, ctx.ignore)
        ctx.rows = ctx.lbl = ctx.coef = None
        B, K, H, W = ctx.shape
        return dl.view(B, H, W, K).permute(0, 3, 1, 2), None, None, None, None, None, None, None


def check_shapes(logit, target, channels=None):
    """the reference fails on these; here a ValueError before anything touches the device"""
    if logit.dim() != 4:
        raise ValueError("expected NCHW logits, got shape %s" % (tuple(logit.shape),))
    B, K, H, W = logit.shape
    if tuple(target.shape) != (B, H, W):
        raise ValueError("labels of shape %s do not match logits %s (B x H x W expected)" % (tuple(target.shape), tuple(logit.shape)))
    if channels is not None and K != channels:
        raise ValueError("%d logit channels, the experiment has %d classes" % (K, channels))


class _Overlap(nn.Module):
    kind = None

    def __init__(self, config):
        super().__init__()
        self.experiment = config["experiment"]
        self.num_classes = _CLASS_INFO_LEN[self.experiment]
        self.naive = False if "naive" not in config else config["naive"]
        self.channels = NUM_CLASSES[self.experiment]
        ig = IGNORE_LABEL[self.experiment]
        self.ignore = -1 if ig is None else ig
        self.invalid_labels = None

    def _weights(self):
        return 0, None

    def forward(self, logit, target):
        check_shapes(logit, target, self.channels)
        mode, w = self._weights()
        out = {}
        loss = _OverlapFn.apply(logit, target, self.kind, self.ignore, bool(self.naive), mode, w, out)
        self.invalid_labels = out["invalid_labels"]
        return loss


class SoftIoU(_Overlap):
    """losses/SoftIoU.py: -mean_c inter_c / union_c, inter_c = sum_p p_pc [y_p = c], union_c = sum_p p_pc + n_c - inter_c; the mean runs
    over the classes with union != 0 (naive: over all c classes, nan where 0 / 0)."""
    kind = 0


class GenDiceLoss(_Overlap):
    """losses/GenDiceLoss.py: 1 - 2 mean_c (w_c dividend_c) / (w_c divisor_c), dividend_c = sum_p p_pc [y_p = c], divisor_c = sum_p p_pc + n_c;
    weights None, 'auto' (1 / n_c^2, 1 where n_c = 0) or a list of c values; the mean runs over the classes whose WEIGHTED divisor is
    non-zero (a weight of 0 excludes its class; naive: every class, nan where 0 / 0)."""
    kind = 1

    def __init__(self, config):
        super().__init__(config)
        self.weights = config["weights"] if "weights" in config else None
        if self.weights is not None and not (isinstance(self.weights, str) and self.weights == "auto"):
            if len(self.weights) != self.channels:
                raise ValueError("Number of weights does not match number of logit channels")

    def _weights(self):
        if self.weights is None:
            return 0, None
        if isinstance(self.weights, str) and self.weights == "auto":
            return 1, None
        return 2, [float(x) for x in self.weights]
