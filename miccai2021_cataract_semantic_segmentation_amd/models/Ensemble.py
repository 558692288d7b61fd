"""Bagging ensemble of trained segmentation nets at inference (reference: models/Ensemble.py:12-90): every member sees the same frame,
each output goes through nn.Softmax2d, the probabilities are merged over the members, and the manager takes the argmax of the merge.
Here the members are the HIP-engine networks of this package and softmax + merge (+ argmax) are ONE kernel launch
(ops.ensemble_merge); members named 'UPerNet' get the ImageNet-normalised frame, produced from the raw frame directly in the stem's
NHWC-4 layout (ops.nchw3_to_nhwc4_norm), the others the raw frame (models/Ensemble.py:63-65).

Config, as the reference's:  {"merge": "mean" | "max", "members": {"1": {"model": "OCRNet" | "DeepLabv3Plus" | "DeepLabv3" | "UPerNet" | ...,
"ckpt": <run id>, ...the member's own config...}, "2": ...}}.

merge = "max": the reference's line is torch.max(output, dim=0), which returns a (values, indices) pair that its own manager cannot
argmax; implemented here is the evident intent, the element-wise maximum of the members' probabilities."""
import torch
from torch import nn

from .. import ops
from ..engine import EngineNet, is_nhwc4
from ..utils.classes import CLASS_REMAP


def get_upernet(config, experiment):
    """models/Ensemble.py:12-18: a 'UPerNet' member is an EncDec built from the member's 'encoder' / 'decoder' entries, prediction only"""
    from .EncDec import EncDec
    model = EncDec(config, experiment)
    model.get_features = False
    return model


class Ensemble(nn.Module):
    def __init__(self, config, experiment):
        super().__init__()
        table = CLASS_REMAP[experiment]
        self.num_classes = len(table) - 1 if 255 in table else len(table)
        self.merge_op = config["merge"]
        if self.merge_op not in ops.MERGE_MODES:
            raise ValueError("Ensemble: merge '{}' is not one of {}".format(self.merge_op, sorted(ops.MERGE_MODES)))
        self.config = config
        self.experiment = experiment
        # a plain list, as in the reference: the members are NOT registered sub-modules (state_dict() of the ensemble is empty)
        self.members, self.members_names, self.ckpt_files = [], [], []
        if not config.get("members"):
            raise ValueError("Ensemble: config['members'] is empty")
        if len(config["members"]) > 8:
            raise ValueError("Ensemble: at most 8 members (got {})".format(len(config["members"])))
        from .. import models as registry
        for key, mc in config["members"].items():
            name = mc.get("model")
            if name == "UPerNet":
                model = get_upernet(mc, experiment)
            else:
                cls = getattr(registry, name, None) if isinstance(name, str) else None
                if not (isinstance(cls, type) and issubclass(cls, EngineNet)):
                    raise ValueError("Ensemble: member '{}' names model '{}', which is not a network of this package".format(key, name))
                model = cls(mc, experiment)
            if hasattr(model, "get_intermediate"):
                model.get_intermediate = False      # OCRNet: final prediction only
            if hasattr(model, "get_features"):
                model.get_features = False
            if getattr(model, "num_classes", None) != self.num_classes:
                raise ValueError("Ensemble: member '{}' ({}) predicts {} classes, experiment {} has {}".format(
                    key, name, getattr(model, "num_classes", None), experiment, self.num_classes))
            model.eval()
            self.members_names.append("UPerNet" if name == "UPerNet" else type(model).__name__)
            self.ckpt_files.append(mc.get("ckpt"))
            self.members.append(model)
        self.num_models = len(self.members)
        self._normed = [mc.get("model") == "UPerNet" for mc in config["members"].values()]

    # the members are outside nn.Module's registry: device moves and eval() have to be handed on
    def _apply(self, fn, *a, **k):
        super()._apply(fn, *a, **k)
        for m in self.members:
            m._apply(fn, *a, **k)
        return self

    def train(self, mode=True):
        """inference only: the members stay in eval mode whatever is asked of the ensemble"""
        super().train(mode)
        for m in self.members:
            m.eval()
        return self

    def _member_logits(self, x):
        """NHWC views of the members' logit buffers for one frame"""
        assert x.shape[0] == 1, "batch size must be one for inference with ensemble"
        if not x.is_cuda:
            raise RuntimeError("the HIP engine only runs on an MI355X device tensor (no CPU fallback)")
        x = x.contiguous().float()
        normed = None
        outs = []
        for model, norm in zip(self.members, self._normed):
            if model.training:
                model.eval()
            xin = x
            if norm:
                if normed is None:
                    # (a frame that arrives in the NHWC-4 layout -- the TTA wrapper's resized copies -- is brought back to NCHW first)
                    nchw = x[..., :3].permute(0, 3, 1, 2).contiguous() if is_nhwc4(x) else x
                    normed = ops.nchw3_to_nhwc4_norm(nchw, ops.IMAGENET_MEAN, ops.IMAGENET_STD)
                xin = normed
            out = model(xin)
            if not torch.is_tensor(out):
                raise RuntimeError("Ensemble: a member returned more than its final logits")
            outs.append(out.permute(0, 2, 3, 1))        # NHWC view of the engine's output buffer
        return outs

    @torch.no_grad()
    def forward(self, x):
        """x: the un-normalised float frame [1, 3, H, W] -> merged probabilities [1, K, H, W] (an NCHW view of an NHWC buffer)"""
        probs, _ = ops.ensemble_merge(self._member_logits(x), self.merge_op, want_probs=True, want_labels=False)
        return probs.permute(0, 3, 1, 2)

    @torch.no_grad()
    def predict(self, x):
        """the int64 label map [1, H, W] = forward(x).argmax(1), straight from the merge kernel (the probabilities are not written)"""
        _, labels = ops.ensemble_merge(self._member_logits(x), self.merge_op, want_probs=False, want_labels=True)
        return labels

    def load_pretrained(self, logging_dir_path, device):
        """models/Ensemble.py:76-90: logging_dir_path / ckpt / 'chkpts' / 'chkpt_best.pt' -> ['model_state_dict'] into each member,
        strict=False; a checkpoint key the member does not have may only belong to the contrastive projector"""
        map_location = device if isinstance(device, (str, torch.device)) else "cuda:{}".format(device)
        for model, ckpt_file in zip(self.members, self.ckpt_files):
            path = logging_dir_path / ckpt_file / "chkpts" / "chkpt_best.pt"
            state_dict = torch.load(str(path), map_location=map_location, weights_only=False)["model_state_dict"]
            have = model.state_dict().keys()
            for k in state_dict:
                if k not in have and "projector" not in k:
                    raise RuntimeError("only projector_model variables can be ignored from ckpt, instead tried to load {} ({})".format(k, path))
            model.load_state_dict(state_dict, strict=False)
