"""SemiSupervisedLoss -- losses/SemiSupervisedLoss.py:8-84 of the reference, quirks included: the first half of the batch is labelled, the
second half pseudo-labelled (with an odd batch the extra frame is pseudo), the same loss runs on both halves and only the weights differ.

No kernel of its own: a batch slice of the engine's NHWC logits is a contiguous view, so the inner losses' kernels (Lovasz, OHEM, the
two-scale pair) run on each half in place, one after the other on the current stream (an inner TwoScaleLoss keeps its side stream).
Nothing here synchronises with the host, so a step with this loss can be captured by graph.GraphedTrainStep.  The gradient of the full
logits tensor is assembled once: _SplitBatch hands out both halves and its backward writes each half's gradient into one buffer, where
torch's slice backward would zero-fill and add a full-size tensor per half."""
import torch
from torch import nn

from ..utils import IGNORE_LABEL
from .lovasz import LovaszSoftmax
from .ohem import OhemCrossEntropy
from .two_scale import TwoScaleLoss

# the names the reference's module resolves with globals() (:4-5, 16-17).  'CrossEntropy' resolves there too, but its constructor call
# hands a dict to nn.CrossEntropyLoss(weight=...) and dies with a TypeError (:33-36 takes the config branch, :28 compares dicts to strings)
_INNER = {"LovaszSoftmax": LovaszSoftmax, "OhemCrossEntropy": OhemCrossEntropy, "TwoScaleLoss": TwoScaleLoss, "CrossEntropy": None}
CROSS_ENTROPY_REFUSAL = ("SemiSupervisedLoss: 'CrossEntropy' is not supported as the inner loss: the reference's own constructor fails on it "
                         "(a config dict reaches nn.CrossEntropyLoss(weight=...): TypeError), so there is no behaviour to reproduce; "
                         "use LovaszSoftmax, OhemCrossEntropy or TwoScaleLoss")


class _SplitBatch(torch.autograd.Function):
    """batch -> (batch[:B // 2], batch[B // 2:]) as views; backward: both halves' gradients written into one buffer of the batch's layout"""

    @staticmethod
    def forward(ctx, batch):
        h = batch.shape[0] // 2
        ctx.channels_last = batch.dim() == 4 and not batch.is_contiguous() and batch.permute(0, 2, 3, 1).is_contiguous()
        ctx.meta = (tuple(batch.shape), batch.dtype, batch.device)
        return batch[:h], batch[h:]

    @staticmethod
    def backward(ctx, g_lab, g_ulab):
        shape, dtype, device = ctx.meta
        h = shape[0] // 2
        if ctx.channels_last:          # the engine's logits: NCHW views of NHWC storage, and so are the gradients the HIP losses return
            full = torch.empty((shape[0], shape[2], shape[3], shape[1]), dtype=dtype, device=device).permute(0, 3, 1, 2)
        else:
            full = torch.empty(shape, dtype=dtype, device=device)
        for part, g in ((full[:h], g_lab), (full[h:], g_ulab)):
            if g is None:
                part.zero_()
            else:
                part.copy_(g)
        return full


def split_batch(batch):
    """losses/SemiSupervisedLoss.py:76-84: (labelled, pseudo-labelled) halves of a (B, ...) tensor"""
    batch_size = batch.size()[0]
    assert batch_size >= 2, "batch_size must be great or equal of 2 instead got {}".format(batch_size)
    if batch.requires_grad:
        return _SplitBatch.apply(batch)
    return batch[0:batch_size // 2], batch[batch_size // 2:]


class SemiSupervisedLoss(nn.Module):
    def __init__(self, config):
        super().__init__()
        lab_loss_class = _INNER[config["labeled"]["name"]]          # (an unknown name: KeyError, as globals()[...] at :16)
        ulab_loss_class = _INNER[config["unlabeled"]["name"]]
        self.w_lab = config["labeled"]["weight"] if "weight" in config["labeled"] else 1.0
        self.w_ulab = config["unlabeled"]["weight"] if "weight" in config["unlabeled"] else 1.0
        self.ignore_label = -100
        if "experiment" in config:
            self.ignore_label = IGNORE_LABEL[config["experiment"]] if config["experiment"] in (2, 3) else -100
        # pass experiment id to constructors of the two losses (:25-26: KeyError without config['experiment'])
        config["labeled"].update({"experiment": config["experiment"]})
        config["unlabeled"].update({"experiment": config["experiment"]})
        if config["labeled"]["name"] != config["unlabeled"]["name"]:
            raise NotImplementedError("different losses for labeled {} and unlabeled {}".format(config["labeled"], config["unlabeled"]))
        if lab_loss_class is None:
            raise NotImplementedError(CROSS_ENTROPY_REFUSAL)
        self.loss_lab = lab_loss_class(config["labeled"])
        self.loss_ulab = ulab_loss_class(config["unlabeled"])

    def forward(self, logits, targets, run_on_labeled_validation=False):
        if isinstance(logits, list):
            if len(logits) != 2:
                raise NotImplementedError("currently only two scales are assumed")
            logits_interm, logits_final = logits
            if run_on_labeled_validation:
                return self.loss_lab(logits_interm, logits_final, targets)
            interm_lab, interm_ulab = split_batch(logits_interm)
            final_lab, final_ulab = split_batch(logits_final)
            targets_lab, targets_ulab = split_batch(targets)
            loss_lab = self.loss_lab(interm_lab, final_lab, targets_lab)
            loss_ulab = self.loss_ulab(interm_ulab, final_ulab, targets_ulab)
            return loss_lab * self.w_lab + loss_ulab * self.w_ulab
        if torch.is_tensor(logits):
            if run_on_labeled_validation:
                return self.loss_lab(logits, targets)
            logits_lab, logits_ulab = split_batch(logits)
            targets_lab, targets_ulab = split_batch(targets)
            loss_lab = self.loss_lab(logits_lab, targets_lab)
            loss_ulab = self.loss_lab(logits_ulab, targets_ulab)      # (:68: loss_lab on the pseudo half too -- only the weights differ)
            return loss_lab * self.w_lab + loss_ulab * self.w_ulab
        raise ValueError("logits has to be either torch.tensor or a list of torch tensors instead got {}".format(type(logits)))
