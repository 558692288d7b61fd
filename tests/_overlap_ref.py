"""Torch restatement of SoftIoU / GenDiceLoss / FocalLoss in any dtype (fp64 = the oracle of the large-shape GPU tests, fp32 = the
calibration of their bar), with the project's rules where the reference raises or divides 0 / 0 in its backward:
  * labels outside [0, K) (and, for the overlap losses, other than the ignore label of experiments 2 / 3) are dropped: zero loss, zero
    gradient; FocalLoss keeps them in the mean's denominator;
  * a class excluded from the non-naive mean contributes zero gradient (the reference's autograd gives nan everywhere there).
Gradients come from torch autograd on these expressions."""
import torch
import torch.nn.functional as F

IGNORE = {1: None, 2: 17, 3: 25}


def overlap_loss(logits, target, kind, experiment, naive=False, weights=None):
    """kind 'SoftIoU' or 'GenDiceLoss'; logits NCHW of the dtype to evaluate in, target int64 B x H x W"""
    B, K, H, W = logits.shape
    t = target.long()
    cls = (t >= 0) & (t < K)
    ig = IGNORE[experiment]
    keep_px = cls | (t == ig) if ig is not None else cls
    p = torch.softmax(logits, 1) * keep_px.unsqueeze(1).to(logits.dtype)
    oh = F.one_hot(t.clamp(0, K - 1), K).permute(0, 3, 1, 2).to(logits.dtype) * cls.unsqueeze(1).to(logits.dtype)
    inter = (p * oh).sum((0, 2, 3))
    s = p.sum((0, 2, 3))
    n = oh.sum((0, 2, 3))
    if kind == "SoftIoU":
        num, den = inter, s + n - inter
    else:
        if weights is None:
            w = torch.ones_like(n)
        elif isinstance(weights, str) and weights == "auto":
            w = torch.where(n == 0, torch.ones_like(n), 1.0 / (n * n))
        else:
            w = torch.tensor([float(x) for x in weights], dtype=logits.dtype, device=logits.device)
        num, den = w * inter, w * (s + n)
    if naive:
        mean = (num / den).mean()
    else:
        keep = den != 0
        frac = num / torch.where(keep, den, torch.ones_like(den))
        mean = frac[keep].sum() / keep.sum()
    return -mean if kind == "SoftIoU" else 1 - 2 * mean


def focal_loss(logits, target, gamma=2, alpha=None):
    B, K, H, W = logits.shape
    rows = logits.permute(0, 2, 3, 1).reshape(-1, K)
    t = target.reshape(-1).long()
    ok = (t >= 0) & (t < K)
    tc = t.clamp(0, K - 1)
    logpt = torch.log_softmax(rows, 1).gather(1, tc.unsqueeze(1)).view(-1)
    pt = logpt.exp()
    if alpha is not None:
        logpt = logpt * torch.tensor([float(a) for a in alpha], dtype=logits.dtype, device=logits.device)[tc]
    loss = -1 * (1 - pt) ** gamma * logpt
    return torch.where(ok, loss, torch.zeros_like(loss)).sum() / t.numel()


def loss_of(name, config, logits, target):
    if name == "FocalLoss":
        return focal_loss(logits, target, config.get("gamma", 2), config.get("alpha"))
    return overlap_loss(logits, target, name, config["experiment"], config.get("naive", False), config.get("weights"))


def loss_and_grad(name, config, logits, target, dtype, scale=1.0):
    x = logits.detach().to(dtype).requires_grad_()
    loss = loss_of(name, config, x, target)
    (loss * scale).backward()
    return loss.detach(), x.grad
