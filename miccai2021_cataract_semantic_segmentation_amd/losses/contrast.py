"""DenseContrastiveLoss -- the loss the reference's LossWrapper, managers and Projector are wired for (losses/LossWrapper.py:50-54,
managers/OCRNet_Manager.py:124-131) but whose source the reference does not ship.  The call surface is the reference's
(``loss(labels, deep_features)``, ``update_confusion_matrix(col_normalised)``); the arithmetic is a build-side definition, held by the
tests to an fp64 restatement under autograd (tests/_contrast_ref.py):

  anchors   A = K * M slots (K classes, M = max_anchors_per_class), filled per class from the low-resolution labels in ascending pixel
            order, by integer strata and one device draw per slot where a class has more than M pixels (include/ext/catseg_contrast.h)
  z_a       = f_a / max(|f_a|, eps) for a filled slot;  s_ij = z_i . z_j / temperature;  pairs i != j of filled slots;  P(i): same label
  l_i       = -(1 / |P(i)|) sum_{p in P(i)} s_ip + log sum_{j != i} w_ij exp(s_ij),  w_ij = 1 for the same label, else W[y_i, y_j]
  loss      = sum_{i: |P(i)| >= 1} l_i / max(n_pos, 1),  n_pos = the number of anchors that have a positive
  W[a, b]   = 1 + confusion_weight * m[b, a] after update_confusion_matrix(m), all ones before

Config keys (build-side): temperature (0.1), max_anchors_per_class (128), confusion_weight (0.0), eps (1e-12).  The class count is the
experiment's (utils.num_classes) unless config['num_classes'] gives it.

Kernels: csrc/contrast.hip (pick, gather, rows, finalize, scatter_bwd) and catseg_gemm_batched for S = Z Z^T and dZ = (G + G^T) Z.  No host
synchronisation and no data-dependent shape: a captured step replays it.  S / G lives in a buffer cached by the module from the forward
to the backward: one pass of a loss object is in flight at a time."""
import torch
from torch import nn

from .. import ops
from ..utils import num_classes


class _ContrastFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, feats, mod, labels, sampler, eval_mode):
        # feats: the [B, d, h, w] view of the engine's NHWC output (any pixel stride); a contiguous NCHW tensor is re-laid once
        f = feats.detach().permute(0, 2, 3, 1)
        if f.stride(3) != 1 or not _rows_dense(f):
            f = f.contiguous()
        B, h, w, d = f.shape
        K, M, A = mod.K, mod.M, mod.K * mod.M
        fixed = sampler.fixed_u
        if fixed is not None:
            fixed = fixed.to(device=f.device, dtype=torch.int32).contiguous()
            if fixed.numel() != A:
                raise ValueError("AnchorSampler.fixed_u must hold K * M = %d values, got %d" % (A, fixed.numel()))
        elif not eval_mode:
            sampler.ensure_seeded()
        idx, lab, n_pos = ops.contrast_pick(labels, h, w, K, M, state=sampler.state, fixed_u=fixed, eval_mode=eval_mode)
        Z, inv_norm = ops.contrast_gather(f, idx, mod.eps)
        S = mod._workspace(A, f.device)
        ops.gemm(ops.NT, 1, A, A, Z.shape[1], Z, Z.shape[1], 0, Z, Z.shape[1], 0, S, S.stride(0), 0)
        ell = ops.contrast_rows(S, A, lab, mod.W, mod.inv_tau, n_pos)
        loss = ops.contrast_finalize(ell, n_pos)
        mod.last = {"idx": idx, "label": lab, "n_pos": n_pos}
        ctx.saved = (Z, inv_norm, idx, S) if feats.requires_grad else None
        ctx.mod, ctx.shape = mod, (B, h, w, d)
        return loss.reshape(())

    @staticmethod
    def backward(ctx, g):
        Z, inv_norm, idx, G = ctx.saved
        ctx.saved = None
        up = g.reshape(1)
        if up.dtype != torch.float32 or not up.is_contiguous():
            up = up.float().contiguous()
        A, dp = Z.shape
        d = ctx.shape[3]
        dZ = torch.empty_like(Z)
        lds = G.stride(0)
        ops.gemm(ops.NN, 1, A, d, A, G, lds, 0, Z, dp, 0, dZ, dp, 0, zero_to=dp)
        ops.gemm(ops.TN, 1, A, d, A, G, lds, 0, Z, dp, 0, dZ, dp, 0, zero_to=dp, accumulate=True)
        df = ops.contrast_scatter_bwd(dZ, Z, inv_norm, idx, d, up, ctx.mod.inv_tau, ctx.shape)
        return df.permute(0, 3, 1, 2), None, None, None, None


def _rows_dense(f):
    """[B, h, w, d] whose pixels are evenly spaced rows: pixel q = (b h + i) w + j starts q * ld floats behind the first"""
    B, h, w, d = f.shape
    ld = f.stride(2) if w > 1 else (f.stride(1) if h > 1 else (f.stride(0) if B > 1 else d))
    return (w == 1 or f.stride(2) == ld) and (h == 1 or f.stride(1) == w * ld) and (B == 1 or f.stride(0) == h * w * ld) and ld >= d


class DenseContrastiveLoss(nn.Module):
    def __init__(self, config):
        super().__init__()
        self.temperature = float(config.get("temperature", 0.1))
        self.M = int(config.get("max_anchors_per_class", 128))
        self.confusion_weight = float(config.get("confusion_weight", 0.0))
        self.eps = float(config.get("eps", 1e-12))
        if "num_classes" in config:
            self.K = int(config["num_classes"])
        elif "experiment" in config:
            self.K = num_classes(config["experiment"])
        else:
            raise ValueError("DenseContrastiveLoss: the class count comes from config['experiment'] or config['num_classes']")
        if not self.temperature > 0.0:
            raise ValueError("DenseContrastiveLoss: temperature must be positive, got %r" % (config.get("temperature"),))
        if not self.eps > 0.0:
            raise ValueError("DenseContrastiveLoss: eps must be positive, got %r" % (config.get("eps"),))
        if self.K < 1 or self.M < 1:
            raise ValueError("DenseContrastiveLoss: num_classes and max_anchors_per_class must be positive, got %d and %d" % (self.K, self.M))
        if self.K * self.M > ops.CONTRAST_MAX_ANCHORS:
            raise ValueError("DenseContrastiveLoss: %d classes x %d anchors = %d slots exceed %d" % (self.K, self.M, self.K * self.M,
                                                                                                     ops.CONTRAST_MAX_ANCHORS))
        self.inv_tau = 1.0 / self.temperature
        # W[a, b] = 1 + confusion_weight * m[b, a]; a buffer that update_confusion_matrix copies into, so a captured step reads the new values
        # (LossWrapper keeps its losses in a plain dict, which .to() does not reach: the table starts on config['device'] where that is given)
        self.register_buffer("W", torch.ones((self.K, self.K), dtype=torch.float32, device=config.get("device")), persistent=False)
        self.sampler = None         # an engine.AnchorSampler: the managers bind the projector's; unbound, a private one is made on first use
        self.last = None            # {"idx", "label", "n_pos"} of the last forward (device int32)
        self._S = None

    def update_confusion_matrix(self, m):
        """m: the [K, K] column-normalised confusion matrix of the epoch (utils.metrics.t_normalise_confusion_matrix(cm, 'col'))"""
        if tuple(m.shape) != (self.K, self.K):
            raise ValueError("update_confusion_matrix: expected a [%d, %d] matrix, got %s" % (self.K, self.K, tuple(m.shape)))
        with torch.no_grad():
            self.W.copy_(1.0 + self.confusion_weight * m.detach().to(device=self.W.device, dtype=torch.float32).t())

    def _workspace(self, A, device):
        if self._S is None or self._S.device != device or self._S.shape[0] != A:
            self._S = torch.empty((A, ops.r4(A)), dtype=torch.float32, device=device)
        return self._S

    def _sampler(self, device):
        if self.sampler is None:
            if device.type == "cuda" and torch.cuda.is_current_stream_capturing():
                raise RuntimeError("DenseContrastiveLoss: no AnchorSampler is bound and the first use is inside a stream capture; bind the "
                                   "projector's (loss.sampler = model.projector_model.sampler) or run one step before capturing")
            from ..engine import AnchorSampler
            self.sampler = AnchorSampler().to(device)
        return self.sampler

    def forward(self, labels, deep_features):
        if deep_features is None or deep_features.dim() != 4:
            raise ValueError("DenseContrastiveLoss: deep_features must be the [B, d, h, w] output of a projector, got %s"
                             % (None if deep_features is None else tuple(deep_features.shape),))
        if labels.dim() != 3 or labels.shape[0] != deep_features.shape[0]:
            raise ValueError("DenseContrastiveLoss: labels must be [B, H, W] with the features' batch size, got %s for features %s"
                             % (tuple(labels.shape), tuple(deep_features.shape)))
        if labels.dtype.is_floating_point:
            raise ValueError("DenseContrastiveLoss: labels must be integers, got %s" % labels.dtype)
        if deep_features.shape[2] > labels.shape[1] or deep_features.shape[3] > labels.shape[2]:
            raise ValueError("DenseContrastiveLoss: the feature map %s is larger than the label map %s"
                             % (tuple(deep_features.shape[2:]), tuple(labels.shape[1:])))
        if not deep_features.is_cuda:
            raise RuntimeError("DenseContrastiveLoss runs on an MI355X device tensor (no CPU fallback)")
        if self.W.device != deep_features.device:
            self.W = self.W.to(deep_features.device)
        lbl = labels if labels.dtype == torch.int64 else labels.long()
        sampler = self._sampler(deep_features.device)
        # eval mode (the module's, or a pass without gradients: validate() runs under no_grad): the mid-stratum anchors, no draw
        eval_mode = not (self.training and torch.is_grad_enabled())
        return _ContrastFn.apply(deep_features, self, lbl.contiguous(), sampler, eval_mode)
