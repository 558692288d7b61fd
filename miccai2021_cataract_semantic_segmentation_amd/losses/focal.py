"""FocalLoss -- losses/FocalLoss.py of the reference (same keys and defaults: gamma = 2, optional per-class alpha registered as a
buffer), computed by the fused HIP kernels of csrc/overlap.hip: loss = mean over all N*H*W pixels of -alpha_y (1 - p_y)^gamma log p_y,
p_y from the UNWEIGHTED log-softmax; forward one pass + an fp64 finalize, backward one pass with autograd's upstream scalar.
gamma = 0 gives the cross-entropy gradient scaled by alpha (torch's pow backward has no term for a zero exponent).

Invalid labels -- outside [0, K), which includes the ignore label of experiments 2 / 3 -- make the reference raise (gather out of bounds).
On the device that would need a host sync, so such pixels contribute zero loss and a zero gradient row and stay in the mean's
denominator; the last call's count is the device tensor ``invalid_labels``.  alpha is passed to the kernels by value: the values given
to the constructor are the ones used (the buffer carries them for .to() / state dicts, as in the reference)."""
import torch
from torch import nn

from .. import ops
from ._common import as_pixel_rows
from .overlap import check_shapes


class _FocalFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, pred, target, gamma, alpha, out):
        rows = as_pixel_rows(pred.detach())
        lbl = target.reshape(-1)
        if lbl.dtype != torch.int64:
            lbl = lbl.long()
        lbl = lbl.contiguous()
        loss, invalid = ops.focal_fwd(rows, lbl, gamma, alpha)
        out["invalid_labels"] = invalid
        ctx.rows, ctx.lbl = (rows, lbl) if pred.requires_grad else (None, None)
        ctx.gamma, ctx.alpha, ctx.shape = gamma, alpha, pred.shape
        return loss.reshape(())

    @staticmethod
    def backward(ctx, g):
        up = g.reshape(1)
        if up.dtype != torch.float32 or not up.is_contiguous():
            up = up.float().contiguous()
        dl = ops.focal_bwd(ctx.rows, ctx.lbl, ctx.gamma, ctx.alpha, up)
        ctx.rows = ctx.lbl = None
        B, K, H, W = ctx.shape
        return dl.view(B, H, W, K).permute(0, 3, 1, 2), None, None, None, None


class FocalLoss(nn.Module):
    def __init__(self, config):
        super().__init__()
        self.gamma = 2 if "gamma" not in config else config["gamma"]
        if "alpha" in config:
            self.register_buffer("alpha", torch.tensor(config["alpha"]))
            self._alpha_host = [float(a) for a in config["alpha"]]
        else:
            self.alpha = None
            self._alpha_host = None
        self.invalid_labels = None

    def forward(self, prediction, target):
        check_shapes(prediction, target)
        K = prediction.shape[1]
        alpha = None
        if self._alpha_host is not None:
            if len(self._alpha_host) < K:
                raise ValueError("alpha has %d entries for %d classes" % (len(self._alpha_host), K))
            alpha = self._alpha_host[:K]
        out = {}
        loss = _FocalFn.apply(prediction, target, float(self.gamma), alpha, out)
        self.invalid_labels = out["invalid_labels"]
        return loss
