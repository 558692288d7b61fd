"""Per-model managers (names as main.py:46 resolves them: config['manager'] + 'Manager') and a synthetic
CaDIS-like dataset for smoke runs and benchmarks."""
import torch
from torch.utils.data import Dataset

from ..losses import LossWrapper, SemiSupervisedLoss
from .base import BaseManager


class OCRNetManager(BaseManager):
    """managers/OCRNet_Manager.py:12-245: the model returns (interm, final); TwoScaleLoss takes both."""

    def forward_loss(self, img, lbl):
        if self.model.projector_model is not None and isinstance(self.loss, LossWrapper):       # (:82-84 of the reference's manager)
            interm, out, proj = self.model(img.float())
            return self.loss(proj, out, lbl.long(), interm_prediction=interm), out
        interm, out = self.model(img.float())[:2]
        if isinstance(self.loss, LossWrapper):
            return self.loss(None, out, lbl.long(), interm_prediction=interm), out
        if isinstance(self.loss, SemiSupervisedLoss):
            return self.semi_loss([interm, out], lbl.long()), out
        return self.loss(interm, out, lbl.long()), out

    def final_output(self, out):
        return out[1] if isinstance(out, tuple) else out


class DeepLabv3PlusManager(BaseManager):
    """managers/DeepLabv3Plus_Manager.py:65-237: single output; LossWrapper-style or plain two-argument losses."""

    def forward_loss(self, img, lbl):
        out = self.model(img.float())
        if getattr(self.model, "projector_model", None) is not None:       # (out, proj): managers/DeepLabv3Plus_Manager.py:80-82
            out, proj = out
            if isinstance(self.loss, LossWrapper):
                return self.loss(proj, out, lbl.long()), out
        if isinstance(self.loss, LossWrapper):
            return self.loss(None, out, lbl.long()), out
        if isinstance(self.loss, SemiSupervisedLoss):
            return self.semi_loss(out, lbl.long()), out
        return self.loss(out, lbl.long()), out


    def final_output(self, out):
        return out[0] if isinstance(out, tuple) else out        # (with a projector the logits come first)


class DeepLabv3Manager(DeepLabv3PlusManager):
    """managers/DeepLabv3_Manager.py: a twin of the DeepLabv3Plus manager bar the class name (configs/DeepLabv3_rf_lvsz.json)."""


class HRNetv2Manager(DeepLabv3PlusManager):
    """(build-side name: the reference has no HRNetv2 manager; its HRNetv2 is a single-output net like DeepLabv3+)"""


class FCNManager(DeepLabv3PlusManager):
    """managers/FCN_Manager.py:10-17 of the reference: image in, logits out; Adam with a CONSTANT learning rate, or an exponential decay
    by config['train']['lr_decay_gamma'] per epoch (the other managers' polynomial schedule is not used)."""

    def load_optimiser(self):
        from ..optim import build_optimiser
        tc = self.config["train"]
        self.optimiser = build_optimiser(self.model, tc.get("optimiser"), tc["learning_rate"], self.grad_scale)
        self.scheduler = torch.optim.lr_scheduler.ExponentialLR(self.optimiser, tc["lr_decay_gamma"]) if "lr_decay_gamma" in tc else None


class EncDecManager(BaseManager):
    """managers/EncDec_Manager.py:14-274: the model is built from the TOP-LEVEL 'encoder' / 'decoder' config entries
    (:16-21, configs/UPN_rf_lvsz.json has no 'graph'), the loss is always a LossWrapper (:23-29), and the step is
    ``deep_features, prediction = model(img); loss = LossWrapper(deep_features, prediction, lbl, epoch=epoch)`` (:158-185)."""

    def __init__(self, configuration, *args, **kwargs):
        dec = configuration.get("decoder", {})
        if configuration.get("mode") == "training" and dec.get("model") == "PointRend" and not dec.get("pr_train_on_device", False):
            from ..models.EncDec import POINTREND_TRAINING_REFUSAL
            raise NotImplementedError(POINTREND_TRAINING_REFUSAL)        # (before anything is built: validate / infer / demo_infer run)
        self.loss_coarse = self.loss_points = None      # PointRend training: the two terms of the last step (device scalars), for logging
        super().__init__(configuration, *args, **kwargs)

    def load_model(self):
        from .. import dist as D
        from ..models import EncDec
        self.model = EncDec(self.config, self.experiment).to(self.device)
        if self.world > 1:
            D.broadcast_parameters(self.model)
            self.grad_scale = D.attach(self.model)
        else:
            self.grad_scale = 1.0

    def load_loss(self):
        from ..losses import CrossEntropyLoss
        from ..utils import ce_ignore_index
        if self.config["loss"].get("name") == "SemiSupervisedLoss":
            raise NotImplementedError("EncDecManager always builds a LossWrapper from config['loss'] (managers/EncDec_Manager.py:23-29) and "
                                      "calls it with deep features and an epoch: a SemiSupervisedLoss has no place in that call; train "
                                      "on pseudo labels with OCRNetManager or a single-output manager")
        self.config["loss"]["experiment"] = self.experiment
        self.config["loss"]["device"] = str(self.device)
        self.loss = LossWrapper(self.config["loss"])
        self.point_loss = CrossEntropyLoss(ignore_index=ce_ignore_index(self.experiment))      # (:165-169: the ignore class in experiments 2 / 3)

    def forward_loss(self, img, lbl):
        out = self.model(img.float())
        if len(out) == 5:
            # PointRend in train mode (:160-171 of the reference's manager): seg_logits IS pred, the interpolated coarse logits that already
            # hold the point predictions; the labels of the points are the nearest pixels' (a point outside the map: class 0)
            from .. import ops
            deep_features, point_coords, point_logits, seg_logits, prediction = out
            lbl = lbl.long()
            self.loss_coarse = self.loss(deep_features, seg_logits, lbl, epoch=self.epoch)
            point_labels = ops.pointrend_point_labels(point_coords, lbl)
            self.loss_points = self.point_loss(point_logits.unsqueeze(3), point_labels.unsqueeze(2))
            return self.loss_coarse + self.loss_points, prediction
        deep_features, prediction = out
        return self.loss(deep_features, prediction, lbl.long(), epoch=self.epoch), prediction

    def final_output(self, out):
        return out[1] if isinstance(out, tuple) else out      # (get_features = False at inference: prediction only)


class EnsembleManager(BaseManager):
    """managers/Ensemble_Manager.py:6-16: inference with models.Ensemble built from config['graph'] = {"model": "Ensemble", "merge": ...,
    "members": {...}}; every member loads log_path / <member's ckpt> / chkpts / chkpt_best.pt.  There is nothing to train and no
    checkpoint of the ensemble itself (BaseManager.py:649 skips load_checkpoint for it).  With WORLD_SIZE > 1 every rank loads the
    same checkpoints (no parameter broadcast) and the frames are sharded round-robin by _eval_pass."""

    def load_model(self):
        import pathlib
        if self.config["mode"] not in ("inference", "demo_video_inference"):
            raise ValueError("EnsembleManager runs mode: 'inference' / 'demo_video_inference' only (got '{}'): an ensemble is not trained"
                             .format(self.config["mode"]))
        cls = getattr(self.model_registry, self.config["graph"]["model"])
        self.model = cls(config=self.config["graph"], experiment=self.experiment).to(self.device)
        self.model.load_pretrained(pathlib.Path(self.config["log_path"]), self.device)
        self.model.to(self.device).eval()        # (reaches every member)
        self.grad_scale = 1.0

    def load_inference_weights(self):
        pass


class SyntheticCataractDataset(Dataset):
    """Seeded synthetic frames with blob-structured label maps (piecewise-constant patches, a few classes
    absent, optional ignore label) — the shape of data SURVEY.md 8d asks the measurements to use."""

    def __init__(self, n, height, width, num_classes, ignore=True, seed=0, patch=16):
        self.n, self.h, self.w, self.k, self.ignore, self.seed, self.patch = n, height, width, num_classes, ignore, seed, patch

    def __len__(self):
        return self.n

    def __getitem__(self, i):
        g = torch.Generator().manual_seed(self.seed * 100003 + i)
        p = self.patch
        lbl = torch.randint(0, self.k + (1 if self.ignore else 0), ((self.h + p - 1) // p, (self.w + p - 1) // p), generator=g)
        lbl[lbl == 3] = 0
        lbl = lbl.repeat_interleave(p, 0).repeat_interleave(p, 1)[: self.h, : self.w].contiguous()
        # image correlated with the labels so that a few optimisation steps can reduce the loss
        img = torch.rand(3, self.h, self.w, generator=g) * 0.5
        img[0] += (lbl.float() / (self.k + 1)) * 0.5
        img[1] += ((lbl * 7) % (self.k + 1)).float() / (self.k + 1) * 0.5
        return img, lbl, {"index": i}

    def raw_labels(self):
        """the frames' label maps as uint8, one after the other: what a scheduled class-aware loader takes its class table from
        (BaseManager.class_table: a census on the device).  The synthetic ids stand in for the raw CaDIS ids."""
        for i in range(self.n):
            yield self[i][1].to(torch.uint8).numpy()
