"""Training / validation / inference loop with the reference managers' contract
(managers/BaseManager.py:26-741, managers/OCRNet_Manager.py:12-245) on the HIP engine.

Kept: step order ``zero_grad -> model(img.float()) -> loss -> backward -> step`` (OCRNet_Manager.py:80-90),
Adam(lr) + LambdaLR(LRFcts) stepped once per epoch (BaseManager.py:439-464, OCRNet_Manager.py:132-134),
validation with batch size 1 in eval mode under no_grad (BaseManager.py:305), best-mIoU rule on the mIoU
rounded to 4 decimals (OCRNet_Manager.py:208-223), checkpoint file names and dictionary keys
(BaseManager.py:471-495), inference with ``get_intermediate = False`` from the 'best' checkpoint (:640-688),
``mode: demo_video_inference`` / ``demo_infer()`` (:148-189, 690-741) with the frames' decoding and encoding outside (video_set / frame_sink).

Changed on purpose (SURVEY.md "hard parts"): metrics stay on the device (one confusion-matrix kernel per
step, no one-hot matmul, no per-step ``.item()``); TensorBoard / matplotlib logging is out of scope; data
parallelism (absent in the reference) shards frames by rank and averages gradients over RCCL.
The dataset is any ``torch.utils.data.Dataset`` yielding ``(img float[3,H,W], lbl int[H,W], metadata)`` like
datasets/Dataset_from_df.py:69; the CaDIS cv2/PIL pipeline itself is outside the accelerated path.
"""
import contextlib
import copy
import datetime
import json
import os
import pathlib

import numpy as np
import torch
from torch.utils.data import DataLoader

from .. import dist as D
from .. import losses as _losses
from .. import models as _models
from ..optim import FusedOptimizer, WeightAverage, accumulate_config, average_config, build_average, build_optimiser
from ..utils import LRFcts
from ..utils.metrics import t_get_confusion_matrix, t_get_mean_iou, t_get_pixel_accuracy, t_normalise_confusion_matrix

DEFAULTS = {"mode": "training", "debugging": False, "log_every_n_epochs": 100, "max_valid_imgs": 10, "cuda": True,
            "gpu_device": 0, "seed": 0, "tta": False, "log_path": "logs"}
TRAIN_DEFAULTS = {"epochs": 50, "lr_fct": "exponential", "lr_batchwise": False, "lr_restarts": [], "lr_restart_vals": 1,
                  "lr_params": None, "learning_rate": 1e-4}
DATA_DEFAULTS = {"batch_size": 10, "num_workers": 0, "experiment": 1,
                 # the per-epoch loader schedule (utils/defaults.py:366-375 of the reference): [start, stop) epochs per loader type
                 "weighted_random": [0, 0], "weighted_random_mode": "v1", "oversampling": [0, 0], "oversampling_frac": 0.2,
                 "oversampling_preset": "default", "adaptive_batching": [0, 0], "adaptive_sel_size": 10, "adaptive_iou_update": 1,
                 "repeat_factor": [0, 0], "repeat_factor_freq_thresh": 0.2,
                 # build-side keys: the [frames, 36] class pixel table of the training set (None: train_set.label_table, or a census of
                 # train_set.raw_labels()), and how many steps the adaptive sampler's IoU may lag behind (utils.IoUTracker)
                 "label_table": None, "adaptive_iou_lag": 0}


def _item(v):
    """one entry of a batch-of-one the DataLoader collated (a tensor, a list or a plain value) as a Python value"""
    if isinstance(v, torch.Tensor):
        return v.reshape(-1)[0].item()
    return v[0] if isinstance(v, (list, tuple)) else v


def _is_frame_triple(v):
    return isinstance(v, (tuple, list)) and len(v) == 3 and isinstance(v[0], torch.Tensor) and isinstance(v[1], torch.Tensor)


def unpack_batch(batch):
    """(img, lbl) of what a loader yields: the (img, lbl, metadata) triple of every dataset here, or -- a utils.BalancedConcatDataset of
    (labelled, pseudo-labelled) members under torch's DataLoader -- one such triple per member, joined along the batch as
    [labelled frames | pseudo-labelled frames], the layout losses.SemiSupervisedLoss splits"""
    if _is_frame_triple(batch):
        return batch[0], batch[1]
    if isinstance(batch, (tuple, list)) and batch and all(_is_frame_triple(m) for m in batch):
        return torch.cat([m[0] for m in batch]), torch.cat([m[1] for m in batch])
    raise ValueError("a batch must be (img, lbl, metadata), or one such triple per member of a BalancedConcatDataset")


def merge_defaults(config):
    """utils/utils.py:533-542: flat defaults + nested defaults for 'data' / 'train' ('loss' must exist)"""
    cfg = dict(DEFAULTS)
    cfg.update(config)
    for key, dflt in (("train", TRAIN_DEFAULTS), ("data", DATA_DEFAULTS)):
        merged = copy.deepcopy(dflt)                   # (the schedule's lists are extended in place: never the defaults' own)
        merged.update(cfg.get(key, {}))
        cfg[key] = merged
    if "loss" not in cfg:
        raise KeyError("config needs a 'loss' entry")
    return cfg


class BaseManager:
    model_registry = _models
    loss_registry = _losses

    def __init__(self, configuration, train_set=None, valid_set=None, train_sampler=None, video_set=None, frame_sink=None):
        self.config = merge_defaults(configuration)
        # config['train']['accumulate'] (build-side key, optim.accumulate_config): micro-steps per optimiser step.  Checked in front of
        # the process group: a window over data-parallel ranks is refused.  Without the key (1) nothing below differs.
        self.accumulate = accumulate_config(self.config["train"].get("accumulate"), int(os.environ.get("WORLD_SIZE", "1")))
        self.start_epoch = self.epoch = 0
        self.best_loss = 1e10
        self.metrics = {"best_miou": 0, "best_miou_anatomies": 0, "best_miou_instruments": 0, "best_miou_rare": 0,
                        "best_miou_epoch_step": "n/a"}
        self.global_step = 0
        self.experiment = self.config["data"]["experiment"]
        self.rank, self.local_rank, self.world = D.init_from_env()
        if not torch.cuda.is_available():
            raise RuntimeError("the HIP engine needs an MI355X device (no CPU fallback)")
        self.device = torch.device("cuda", self.local_rank if self.world > 1 else self.config["gpu_device"])
        torch.cuda.set_device(self.device)
        self.run_id = self.config.get("load_checkpoint") if self.config["mode"] != "training" and "load_checkpoint" in self.config \
            else "{:%Y%m%d_%H%M%S}_e{}".format(datetime.datetime.now(), self.experiment) + \
                 ("__" + self.config["name"] if "name" in self.config else "")
        self.log_dir = pathlib.Path(self.config["log_path"]) / self.run_id
        if self.rank == 0:
            self.log_dir.mkdir(parents=True, exist_ok=True)
        # `manager_class(config)` as main.py:61 constructs it: the reference's load_data() (cv2 / pandas decoding, out of this path's scope)
        # is replaced by a callable the configuration names -- config['data']['dataset_factory'](config) -> (train_set, valid_set, sampler)
        factory = self.config["data"].get("dataset_factory")
        if train_set is None and valid_set is None and callable(factory):
            made = tuple(factory(self.config))
            train_set, valid_set, train_sampler = (made + (None, None, None))[:3]
        self.train_set, self.valid_set, self.train_sampler = train_set, valid_set, train_sampler
        # mode 'demo_video_inference' (BaseManager.py:148-189): cv2's VideoCapture / VideoWriter stay outside -- video_set is any dataset
        # yielding (frame float [3, H, W] in [0, 1], frame_idx, vid_id) as DatasetFromVideo does, frame_sink a callable
        # (vid_id, frame_idx, ndarray [H, n W, 3] uint8 BGR); or config['data']['video_factory'](config) -> (video_set, frame_sink)
        if self.config["mode"] == "demo_video_inference":
            self.config.setdefault("demo_frame_freq", 1)       # every n-th frame: for the factory to honour
            vfactory = self.config["data"].get("video_factory")
            if video_set is None and frame_sink is None and callable(vfactory):
                video_set, frame_sink = tuple(vfactory(self.config))[:2]
        self.video_set, self.frame_sink = video_set, frame_sink
        self.load_model()
        self.loss = self.optimiser = self.scheduler = None
        # config['train']['ema'] (build-side key, optim.average_config): a running average of the weights updated behind every optimiser
        # step, scored by validate(), saved beside the model and loaded by the inference modes.  Without the key nothing is attached.
        self.ema_cfg, self.average = average_config(self.config["train"].get("ema")), None
        self.labeled_validation = False      # inside _eval_pass(with_loss=True): a SemiSupervisedLoss scores the whole batch as labelled
        if self.config["mode"] == "training":
            self.load_loss()
            self.bind_contrast()
            torch.manual_seed(self.config["seed"])      # after model construction, as BaseManager.py:104-112
            self.load_optimiser()
            if self.accumulate > 1:
                if not isinstance(self.optimiser, FusedOptimizer):
                    raise ValueError("config['train']['accumulate'] needs a fused optimiser of optim.py (the window lives in it)")
                self.optimiser.set_accumulation(self.accumulate)
            self.average = build_average(self.model, self.optimiser, self.ema_cfg)
        elif self.config["mode"] not in ("inference", "demo_video_inference"):
            raise ValueError("mode: {} is not recognized".format(self.config["mode"]))
        self.history = []
        # the per-epoch loader schedule (build_schedule): None = every epoch iterates self.train_loader
        self.train_schedule, self.data_loaders = None, {}
        self.iou_tracker = self.adaptive_sampler = self._label_table = self._checkpoint_iou = None

    # ------------------------------------------------------------------ construction
    def load_model(self):
        cls = getattr(self.model_registry, self.config["graph"]["model"])
        self.model = cls(config=self.config["graph"], experiment=self.experiment).to(self.device)
        if self.world > 1:
            D.broadcast_parameters(self.model)
            self.grad_scale = D.attach(self.model)
        else:
            self.grad_scale = 1.0

    def load_loss(self):
        cls = getattr(self.loss_registry, self.config["loss"]["name"])
        self.config["loss"]["experiment"] = self.experiment
        self.config["loss"]["device"] = str(self.device)
        self.loss = cls(self.config["loss"])

    def load_optimiser(self):
        tc = self.config["train"]
        # config['train']['optimiser'] (build-side key, optim.build_optimiser); without it: Adam(lr), what the reference builds
        self.optimiser = build_optimiser(self.model, tc.get("optimiser"), tc["learning_rate"], self.grad_scale)
        self.scheduler = torch.optim.lr_scheduler.LambdaLR(self.optimiser, lr_lambda=LRFcts(tc, list(tc["lr_restarts"]), tc["epochs"]))

    def loaders(self):
        """train loader (batch bs, drop_last) + validation loader (batch 1, BaseManager.py:305).  With WORLD_SIZE > 1 the
        training frames are SHARDED by rank: one shared-seed index stream per epoch (a permutation, or the given sampler's
        stream -- the repeat-factor sampler draws from a private Generator(seed=1) and is identical on every rank), each
        rank taking every world-th index: global batch = world * bs, disjoint frames, equal step counts."""
        bs = self.config["data"]["batch_size"]
        self.shard_sampler = None
        if self.world > 1:
            src = self.train_sampler if self.train_sampler is not None else len(self.train_set)
            if self.train_sampler is not None:
                D.check_unsharded(self.train_sampler)
            self.shard_sampler = D.ShardedSampler(src, self.rank, self.world, bs, seed=self.config["seed"])
            tl = DataLoader(self.train_set, batch_size=bs, sampler=self.shard_sampler, drop_last=True,
                            num_workers=0 if self.train_sampler is not None else self.config["data"]["num_workers"])
        elif self.train_sampler is not None:
            tl = DataLoader(self.train_set, batch_size=bs, sampler=self.train_sampler, drop_last=True, num_workers=0)
        else:
            tl = DataLoader(self.train_set, batch_size=bs, shuffle=True, drop_last=True,
                            num_workers=self.config["data"]["num_workers"])
        vl = DataLoader(self.valid_set, batch_size=1, shuffle=False) if self.valid_set is not None else None
        return tl, vl

    def class_table(self):
        """int64 [frames, 36]: pixels per canonical class and training frame -- what the reference reads from data/data.csv.  From, in
        order: config['data']['label_table'], train_set.label_table, a census of train_set.raw_labels() (utils.label_census: the uint8
        label maps, counted on the device)."""
        if self._label_table is None:
            table = self.config["data"].get("label_table")
            if table is None:
                table = getattr(self.train_set, "label_table", None)
            if table is None and hasattr(self.train_set, "raw_labels"):
                from ..utils import label_census
                table = label_census(self.train_set.raw_labels(), 36, device=self.device)
            if table is None:
                raise ValueError("a scheduled class-aware train loader needs the [frames, 36] class pixel table of the training set: "
                                 "config['data']['label_table'], train_set.label_table, or train_set.raw_labels() (the raw uint8 label "
                                 "maps, for a census on the device)")
            table = np.asarray(table)
            if table.ndim != 2 or table.shape != (len(self.train_set), 36):
                raise ValueError("the class pixel table must be [{}, 36] (one row per training frame), got {}".format(
                    len(self.train_set), table.shape))
            self._label_table = table.astype(np.int64)
        return self._label_table

    def build_schedule(self):
        """BaseManager.py:198-213 of the reference: self.train_schedule (epoch -> loader name, utils.train_schedule) from the four
        config['data'] keys adaptive_batching / oversampling / weighted_random / repeat_factor, and one loader per scheduled name in
        self.data_loaders.  With every key at its default [0, 0] every epoch iterates self.train_loader and nothing else is built."""
        from ..utils import train_schedule
        self.train_schedule = train_schedule(self.config["data"], self.config["train"]["epochs"])
        self.data_loaders = {"train_loader": self.train_loader, "valid_loader": self.valid_loader}
        for name in sorted(set(self.train_schedule.values()) - {"train_loader"}):
            self.data_loaders[name] = self.scheduled_loader(name)

    def scheduled_loader(self, name):
        """BaseManager.py:310-403: the loader `name` of the schedule over self.train_set.  Like loaders(), every loader drops the ragged
        last batch.  Data parallel: oversampling and repeat-factor streams are the same on every rank and are sharded
        (dist.ShardedSampler); adaptive batching and weighted random are refused."""
        from ..utils import (CLASS_REMAP, OVERSAMPLING_PRESETS, AdaptiveBatchSampler, IoUTracker, RepeatFactorSampler, ShuffledIndexList,
                             class_info, oversampled_indices, presence_of, weighted_random_weights)
        dc = self.config["data"]
        bs, workers = dc["batch_size"], dc["num_workers"]
        if self.world > 1 and name == "train_adaptive_batching_loader":
            raise ValueError("adaptive batching is refused with WORLD_SIZE > 1: every rank averages the IoU of its own batches and draws "
                             "from its own numpy generator, so the ranks' batches would neither be disjoint nor follow one IoU")
        if self.world > 1 and name == "train_weighted_random_loader":
            raise ValueError("the weighted-random loader is refused with WORLD_SIZE > 1: torch's WeightedRandomSampler draws from each "
                             "rank's own generator, so the ranks' streams differ and cannot be sharded")
        table = self.class_table()
        table_k = class_info(table, self.experiment)

        def shard(sampler):
            if self.world == 1:
                return sampler
            return D.ShardedSampler(sampler, self.rank, self.world, bs, seed=self.config["seed"])

        if name == "train_adaptive_batching_loader":
            # the tracker follows the network's confusion matrix (UNet and FCN predict the ignore class too: one row and column more);
            # the sampler takes the experiment's real classes, the leading entries (t_get_mean_iou's `indices`)
            real = table_k.shape[1]
            self.iou_tracker = IoUTracker(self.model.num_classes, dc["adaptive_iou_update"], self.device, lag=dc["adaptive_iou_lag"])
            if self._checkpoint_iou is not None:
                self.iou_tracker.load_values(self._checkpoint_iou)
            # (with num_workers > 0 torch draws batches `prefetch_factor * num_workers` ahead of the step, as it does in the reference)
            self.adaptive_sampler = AdaptiveBatchSampler(table_k, np.array(self.iou_tracker.host()[:real], dtype=np.float32), "1-**2", bs,
                                                         dc["adaptive_sel_size"], refresh=lambda: self.iou_tracker.host()[:real])
            return DataLoader(self.train_set, batch_sampler=self.adaptive_sampler, num_workers=workers)
        if name == "train_oversampling_loader":
            class_list = OVERSAMPLING_PRESETS[dc["oversampling_preset"]][self.experiment - 1]
            indices = oversampled_indices(table_k, class_list, dc["oversampling_frac"])
            return DataLoader(self.train_set, batch_size=bs, sampler=shard(ShuffledIndexList(indices, seed=self.config["seed"])),
                              drop_last=True, num_workers=workers)
        if name == "train_weighted_random_loader":
            weights = weighted_random_weights(table_k, dc["weighted_random_mode"])
            return DataLoader(self.train_set, batch_size=bs, sampler=torch.utils.data.WeightedRandomSampler(weights, len(self.train_set)),
                              drop_last=True, num_workers=workers)
        if name == "train_repeat_factor_loader":
            remap = CLASS_REMAP[self.experiment]
            cmap = np.array([next(k for k, raw in remap.items() if j in raw) for j in range(36)], dtype=np.int64)
            sampler = RepeatFactorSampler(presence_of(table), cmap, sorted(remap), dc["repeat_factor_freq_thresh"])
            return DataLoader(self.train_set, batch_size=bs, sampler=shard(sampler), drop_last=True, num_workers=0)
        raise ValueError("Dataloader special type '{}' not recognised".format(name))

    def contrast_loss(self):
        """the DenseContrastiveLoss of a LossWrapper, or None"""
        if isinstance(self.loss, _losses.LossWrapper):
            return self.loss.loss_classes.get("DenseContrastiveLoss")
        return None

    def bind_contrast(self):
        """the anchors of a DenseContrastiveLoss are drawn from the projector's device state (engine.AnchorSampler): a buffer of the model,
        which graph.GraphedTrainStep seeds before its capture and restores around its warm-up, and which dist.attach gives the rank"""
        dc = self.contrast_loss()
        if dc is None:
            return
        proj = getattr(self.model, "projector_model", None)
        if proj is None:
            raise ValueError("the loss 'DenseContrastiveLoss' contrasts the output of a projector: the model's configuration has no "
                             "'projector' key")
        if dc.K != self.model.num_classes:
            raise ValueError("DenseContrastiveLoss was built for %d classes, the model predicts %d" % (dc.K, self.model.num_classes))
        dc.sampler = proj.sampler

    def update_contrast(self, running_cm):
        """the end of a training epoch, managers/OCRNet_Manager.py:124-131 of the reference (without the TensorBoard figure): the epoch's
        column-normalised confusion matrix goes to the contrastive loss"""
        dc = self.contrast_loss()
        if dc is not None:
            dc.update_confusion_matrix(t_normalise_confusion_matrix(running_cm, mode="col"))

    # ------------------------------------------------------------------ hooks for the subclasses
    def forward_loss(self, img, lbl):
        """returns (loss, final logits)"""
        out = self.model(img.float())
        if isinstance(self.loss, _losses.SemiSupervisedLoss):
            return self.semi_loss(out, lbl.long()), out
        return self.loss(out, lbl.long()), out

    def semi_loss(self, logits, lbl):
        """a SemiSupervisedLoss on a tensor (single-output nets) or on [interm, final] (OCRNet).  Build-side wiring: the reference's managers
        never call this loss (OCRNet_Manager.py:87 hands it three arguments, which SemiSupervisedLoss.forward cannot take).  In training the
        batch is [labelled | pseudo-labelled]; validation batches are labelled throughout (run_on_labeled_validation)"""
        return self.loss(logits, lbl, run_on_labeled_validation=self.labeled_validation)

    def final_output(self, out):
        return out

    # ------------------------------------------------------------------ loops
    def train(self):
        self.train_loader, self.valid_loader = self.loaders()
        self.build_schedule()
        for self.epoch in range(self.config["train"]["epochs"]):
            self.train_one_epoch()
            if self.valid_loader is not None:
                self.validate()
        return self.metrics

    def train_one_epoch(self):
        self.model.train()
        K = self.model.num_classes
        running_cm = torch.zeros((K, K), dtype=torch.int32, device=self.device)
        loss_sum = torch.zeros((), device=self.device)
        n = 0
        if getattr(self, "shard_sampler", None) is not None:
            self.shard_sampler.set_epoch(self.epoch + self.start_epoch)
        # the epoch's loader (OCRNet_Manager.py:72): self.train_loader unless build_schedule() put another one on this epoch
        loader = self.train_loader
        if self.train_schedule is not None and self.train_schedule.get(self.epoch, "train_loader") != "train_loader":
            loader = self.data_loaders[self.train_schedule[self.epoch]]
        # adaptive batching anywhere in the schedule: every step of every epoch ends with the per-batch IoU average on the device
        # (OCRNet_Manager.py:114-117; utils.IoUTracker), published to the host behind the step
        tracker = self.iou_tracker
        if tracker is not None:
            tracker.reset()                      # (running_cm starts at zero: so does the matrix the batch differences are taken from)
        # config['train']['hip_graph'] (build-side key, default off): the step -- zero_grad, forward, loss, backward, Adam, confusion matrix --
        # is recorded once per epoch into a hipGraph and replayed (graph.GraphedTrainStep: bit-identical to this loop, one host call per
        # step instead of ~3000 launches); batches of another shape (a ragged last batch) run the loop below
        # config['train']['accumulate'] = n > 1: every batch is a micro-step (zero_grad, forward, loss, backward, fold); the optimiser steps
        # when its window is full and, on a partial window, at the end of the epoch in front of the scheduler: no window spans an epoch, no
        # batch's gradient is dropped.  The graph and the loop below share the optimiser's window, so a ragged batch continues it eagerly.
        graphed = None
        accumulate = self.accumulate
        steps0 = self.optimiser._steps if accumulate > 1 else 0
        use_graph = bool(self.config.get("train", {}).get("hip_graph", False)) and isinstance(self.optimiser, FusedOptimizer)
        for batch in loader:
            img, lbl = unpack_batch(batch)
            img, lbl = img.to(self.device, non_blocking=True), lbl.to(self.device, non_blocking=True)
            if use_graph and graphed is None:
                from ..graph import GraphedTrainStep
                img, lbl = img.float().contiguous(), lbl.long().contiguous()
                graphed = GraphedTrainStep(self.model, None, self.optimiser, img, lbl, confusion=running_cm, forward_loss=self.forward_loss,
                                           tracker=tracker, accumulate=accumulate)
            if graphed is not None and img.shape == graphed.img.shape and lbl.shape == graphed.lbl.shape:
                loss_sum += graphed(img, lbl)
            else:
                if graphed is not None:
                    graphed.release()
                    graphed, use_graph = None, False
                self.optimiser.zero_grad()
                loss, out = self.forward_loss(img, lbl)
                loss.backward()
                if accumulate > 1:
                    self.optimiser.fold()
                    if self.optimiser.window_full():
                        self.optimiser.step()
                else:
                    self.optimiser.step()
                t_get_confusion_matrix(out.detach(), lbl, running_cm)      # accumulates on the device
                if tracker is not None:
                    tracker.step(running_cm)
                loss_sum += loss.detach()
            if tracker is not None:
                tracker.publish()                # K floats on their way to the pinned buffer the next batch's draw reads
            n += 1
            self.global_step += 1
        if accumulate > 1 and self.optimiser._folded > 0:      # the epoch's last, partial window
            if graphed is not None:
                graphed.flush()
            else:
                self.optimiser.step()
        if graphed is not None:
            graphed.release()
        self.update_contrast(running_cm)         # (this rank's matrix: each rank contrasts its own anchors with its own table)
        if self.scheduler is not None:
            self.scheduler.step()
        if self.world > 1:                       # logged training metrics are GLOBAL: one exchange per epoch
            import torch.distributed as dist
            cm64 = running_cm.to(torch.int64)
            dist.all_reduce(cm64)
            running_cm = cm64.to(torch.int32)
            cnt = torch.tensor([float(n)], device=self.device)
            dist.all_reduce(cnt)
            dist.all_reduce(loss_sum)
            n = int(cnt)
        pa, pac = t_get_pixel_accuracy(running_cm)
        miou = t_get_mean_iou(running_cm, self.experiment)
        rec = {"epoch": self.epoch + self.start_epoch, "train_loss": float(loss_sum / max(n, 1)), "train_miou": float(miou),
               "train_pixel_accuracy": float(pa), "lr": self.optimiser.param_groups[0]["lr"]}
        if accumulate > 1:
            rec["optimiser_steps"] = self.optimiser._steps - steps0
        self.history.append(rec)
        if self.rank == 0:
            print("Epoch {epoch:03d} - loss {train_loss:.5f} - miou {train_miou:.4f} - pa {train_pixel_accuracy:.4f}".format(**rec))

    def _eval_pass(self, loader, with_loss):
        K = self.model.num_classes
        cm = torch.zeros((K, K), dtype=torch.int32, device=self.device)
        loss_sum = torch.zeros((), device=self.device)
        n = 0
        self.labeled_validation = bool(with_loss)
        try:
            with torch.no_grad():
                for i, (img, lbl, _) in enumerate(loader):
                    if self.world > 1 and i % self.world != self.rank:   # frames sharded round-robin over ranks
                        continue
                    img, lbl = img.to(self.device), lbl.to(self.device)
                    if with_loss:
                        loss, out = self.forward_loss(img, lbl)
                        loss_sum += loss
                    else:
                        out = self.final_output(self.model(img.float()))
                    t_get_confusion_matrix(out, lbl, cm)
                    n += 1
        finally:
            self.labeled_validation = False
        if self.world > 1:                                            # one exchange at the end
            import torch.distributed as dist
            cm64 = cm.to(torch.int64)
            dist.all_reduce(cm64)
            cm = cm64.to(torch.int32)
            cnt = torch.tensor([float(n)], device=self.device)
            dist.all_reduce(cnt)
            dist.all_reduce(loss_sum)
            n = int(cnt)
        return cm, float(loss_sum) / max(n, 1)

    def validate(self):
        self.model.eval()
        D.sync_bn_stats(self.model)      # every rank scores (and rank 0 saves) the same running statistics
        # config['train']['ema']: the averaged weights are scored ("ema"; "both": the live ones as well, for the history) -- swapped into
        # the live model in place.  Data parallel: the averaged running statistics are pooled over ranks like the live ones above (the
        # parameter shadows are bit-identical across ranks as the parameters are), so that every rank scores what rank 0 saves.
        which = self.ema_cfg["validate"] if self.average is not None and self.average.ready else "live"
        live = None
        if which == "live":
            cm, valid_loss = self._eval_pass(self.valid_loader, with_loss=True)
        else:
            if which == "both":
                live = self._eval_pass(self.valid_loader, with_loss=True)
            with self.average.applied():
                D.sync_bn_stats(self.model)
                cm, valid_loss = self._eval_pass(self.valid_loader, with_loss=True)
        pa, pac = t_get_pixel_accuracy(cm)
        m_iou, m_ins, m_anat, m_rare = t_get_mean_iou(cm, self.experiment, True, rare=True)
        m_iou, m_ins, m_anat = round(float(m_iou), 4), round(float(m_ins), 4), round(float(m_anat), 4)
        step = [self.epoch + self.start_epoch, self.global_step - 1]
        if self.history:
            self.history[-1].update({"valid_loss": valid_loss, "valid_miou": m_iou})
            if live is not None:
                self.history[-1].update({"valid_loss_live": live[1], "valid_miou_live": round(float(t_get_mean_iou(live[0], self.experiment)), 4)})
        if m_iou > self.metrics["best_miou"]:
            self.metrics.update({"best_miou": m_iou, "best_miou_anatomies": m_anat, "best_miou_instruments": m_ins,
                                 "best_miou_rare": float(m_rare), "best_miou_epoch_step": step})
            self.save_checkpoint(is_best=True)
        if valid_loss < self.best_loss:
            self.best_loss = valid_loss
            self.metrics.update({"best_loss_miou": m_iou, "best_loss_miou_anatomies": m_anat,
                                 "best_loss_miou_instruments": m_ins, "best_loss_miou_rare": float(m_rare),
                                 "best_loss_epoch_step": step})
        if (self.epoch % self.config["log_every_n_epochs"] == 0 and self.epoch > 0) or self.epoch == self.config["train"]["epochs"] - 1:
            self.save_checkpoint(is_best=False)
        self.write_info_json()
        if self.rank == 0:
            print("Epoch {:03d} - Validation loss: {:.5f} - miou:{:.3f} - ins:{:.3f} - anat:{:.3f} - rare:{:.4f}".format(
                self.epoch + self.start_epoch, valid_loss, m_iou, m_ins, m_anat, float(m_rare)))
        return m_iou

    def infer(self):
        self.model.eval()
        if hasattr(self.model, "get_intermediate"):
            self.model.get_intermediate = False
        if hasattr(self.model, "get_features"):
            self.model.get_features = False
        self.load_inference_weights()
        loader = DataLoader(self.valid_set, batch_size=1, shuffle=False)
        net = self.model
        if self.config["tta"]:                       # BaseManager.py:652-660: hflip x 5 scales, mean-merged
            from ..utils.tta import SegmentationTTA
            self.model = SegmentationTTA(net)
            self.model.num_classes = net.num_classes
        try:
            cm, _ = self._eval_pass(loader, with_loss=False)
        finally:
            self.model = net
        m = t_get_mean_iou(cm, self.experiment, True, rare=True)
        return tuple(float(v) for v in m)

    def demo_infer(self):
        """BaseManager.py:690-741: the model over every frame of video_set, the frame_sink called once per frame, in order, with the uint8
        BGR picture frame | coloured prediction ([H, 2 W, 3]; the prediction alone, [H, W, 3], with 'miccai_demo' in the configuration).
        argmax, colouring, the frame's bytes and the concatenation are one kernel (utils.GpuEgress); the picture of frame i travels to
        the host on a second stream, through a two-slot pinned ring with one event per slot, while frame i + 1 is in the network.
        config['demo_crop'] = (top, bottom) drops the rows a padding ingest added (default (0, 0): the reference feeds 540-row frames
        unpadded).  Returns the number of frames."""
        from ..utils.egress import GpuEgress
        if self.video_set is None or not callable(self.frame_sink):
            raise ValueError("mode: demo_video_inference needs video_set= and frame_sink= (or config['data']['video_factory'])")
        self.model.eval()
        if hasattr(self.model, "get_intermediate"):
            self.model.get_intermediate = False
        if hasattr(self.model, "get_features"):
            self.model.get_features = False
        self.load_inference_weights()
        probs = isinstance(self.model, _models.Ensemble)      # already softmaxed and merged (BaseManager.py:724)
        only_pred = "miccai_demo" in self.config
        egress = GpuEgress(self.experiment, crop=tuple(self.config.get("demo_crop", (0, 0))), bgr=True, device=self.device)
        main, side = torch.cuda.current_stream(self.device), torch.cuda.Stream(self.device)
        ring = [{"host": None, "event": torch.cuda.Event(), "dev": None, "tag": None} for _ in range(2)]

        def flush(slot):
            if slot["tag"] is not None:
                slot["event"].synchronize()
                self.frame_sink(slot["tag"][0], slot["tag"][1], slot["host"].numpy().copy())      # the array is the sink's to keep
                slot["tag"] = slot["dev"] = None

        n = 0
        with torch.no_grad():
            for frame, frame_idx, vid_id in DataLoader(self.video_set, batch_size=1, shuffle=False):
                frame = frame.to(self.device, non_blocking=True).float()
                out = self.final_output(self.model(frame))
                if isinstance(out, (tuple, list)):              # (UPerNet: the last output, BaseManager.py:718-719)
                    out = out[-1]
                canvas = egress(out, frame=None if only_pred else frame, probs=probs)[0]
                slot = ring[n % 2]                               # (emptied when frame n - 1 was enqueued)
                if slot["host"] is None or slot["host"].shape != canvas.shape:
                    slot["host"] = torch.empty(canvas.shape, dtype=torch.uint8, pin_memory=True)
                side.wait_stream(main)
                with torch.cuda.stream(side):
                    slot["host"].copy_(canvas, non_blocking=True)
                    slot["event"].record(side)
                slot["dev"], slot["tag"] = canvas, (_item(vid_id), _item(frame_idx))      # the device picture lives until its copy has ended
                flush(ring[(n + 1) % 2])                         # frame n - 1: its copy ran beside this frame's forward pass
                n += 1
        flush(ring[n % 2])
        flush(ring[(n + 1) % 2])
        return n

    def pseudo_label(self, frame_set=None, label_sink=None, threshold=None, weights="live"):
        """Pseudo labels for unlabelled frames, in the form DatasetFromDF(labels_remaped=True) reads (datasets/Dataset_from_df.py:49-53):
        the eval-mode forward as infer() runs it (the model, an Ensemble, or TTA per config['tta']) over every frame of frame_set (items
        (frame float [3, H, W], ...); default: video_set), then utils.GpuEgress with `threshold` and the pad rows of config['demo_crop']
        cropped.  label_sink(index, labels) receives, in order, a uint8 [H, W] map of the experiment's NETWORK ids in which the
        experiment's ignore id marks the pixels whose largest softmax score is below the threshold (utils.clipped_argmax).  The maps
        travel to the host through demo_infer's two-slot pinned ring, beside the next frame's forward pass.  Experiment 1 has no ignore
        id: a threshold is refused there.  weights="ema" (a training manager with config['train']['ema']): the frames are labelled with
        the averaged weights, swapped in for the duration of the call -- the teacher of a mean-teacher loop.  Returns the number of frames."""
        if weights not in ("live", "ema"):
            raise ValueError("pseudo_label: weights is 'live' or 'ema', got {!r}".format(weights))
        if weights == "ema" and self.average is None:
            raise ValueError("pseudo_label(weights='ema') needs a training manager with config['train']['ema'] (an inference manager loads "
                             "the averaged weights of its checkpoint by that key's 'infer')")
        frame_set = self.video_set if frame_set is None else frame_set
        if frame_set is None or not callable(label_sink):
            raise ValueError("pseudo_label needs frame_set= (or video_set) and a callable label_sink(index, labels)")
        if threshold and self.experiment not in (2, 3):
            raise ValueError("pseudo_label: experiment {} has no ignore id to mark pixels below the threshold with (clipped_argmax asserts a "
                             "truthy ignore_value); use threshold=None".format(self.experiment))
        flags = {f: getattr(self.model, f) for f in ("get_intermediate", "get_features") if hasattr(self.model, f)}
        was_training = self.model.training
        try:
            with self.average.applied() if weights == "ema" else contextlib.nullcontext():
                return self._pseudo_label(frame_set, label_sink, threshold)
        finally:                                     # a training manager goes on training: (interm, final) outputs, train mode
            for f, v in flags.items():
                setattr(self.model, f, v)
            self.model.train(was_training)

    def _pseudo_label(self, frame_set, label_sink, threshold):
        from ..utils import IGNORE_LABEL
        from ..utils.egress import GpuEgress
        self.model.eval()
        if hasattr(self.model, "get_intermediate"):
            self.model.get_intermediate = False
        if hasattr(self.model, "get_features"):
            self.model.get_features = False
        if self.config["mode"] != "training":        # as infer(): the run's 'best' checkpoint; a training manager labels with the weights it holds
            self.load_inference_weights()
        probs = isinstance(self.model, _models.Ensemble)
        net = self.model
        if self.config["tta"]:
            from ..utils.tta import SegmentationTTA
            net = SegmentationTTA(self.model)
        egress = GpuEgress(self.experiment, crop=tuple(self.config.get("demo_crop", (0, 0))), threshold=threshold,
                           ignore_value=IGNORE_LABEL[self.experiment] if self.experiment in (2, 3) else 0, device=self.device)
        egress.lut = torch.arange(256, dtype=torch.uint8, device=self.device)      # the uint8 maps keep the network ids
        main, side = torch.cuda.current_stream(self.device), torch.cuda.Stream(self.device)
        ring = [{"host": None, "event": torch.cuda.Event(), "dev": None, "tag": None} for _ in range(2)]

        def flush(slot):
            if slot["tag"] is not None:
                slot["event"].synchronize()
                label_sink(slot["tag"], slot["host"].numpy().copy())
                slot["tag"] = slot["dev"] = None

        n = 0
        with torch.no_grad():
            for item in DataLoader(frame_set, batch_size=1, shuffle=False):
                frame = (item[0] if isinstance(item, (tuple, list)) else item).to(self.device, non_blocking=True).float()
                out = self.final_output(net(frame))
                if isinstance(out, (tuple, list)):
                    out = out[-1]
                labels = egress(out, want="labels_u8", probs=probs)[0]
                slot = ring[n % 2]
                if slot["host"] is None or slot["host"].shape != labels.shape:
                    slot["host"] = torch.empty(labels.shape, dtype=torch.uint8, pin_memory=True)
                side.wait_stream(main)
                with torch.cuda.stream(side):
                    slot["host"].copy_(labels, non_blocking=True)
                    slot["event"].record(side)
                slot["dev"], slot["tag"] = labels, n
                flush(ring[(n + 1) % 2])
                n += 1
        flush(ring[n % 2])
        flush(ring[(n + 1) % 2])
        return n

    def load_inference_weights(self):
        """BaseManager.py:649: inference scores this run's 'best' checkpoint (EnsembleManager: its members' own, loaded at construction)"""
        self.load_checkpoint("best", averaged=bool(self.ema_cfg and self.ema_cfg["infer"]))

    # ------------------------------------------------------------------ checkpoints (BaseManager.py:471-529)
    def save_checkpoint(self, is_best):
        """BaseManager.py:471-495.  Called by every rank (validate() synchronised the BatchNorm running statistics just
        before); only rank 0 writes."""
        if self.rank != 0:
            return
        base = self.log_dir / "chkpts"
        base.mkdir(exist_ok=True)
        state = {"global_step": self.global_step, "epoch": self.start_epoch + self.epoch,
                 "model_state_dict": {k: v.detach().cpu().contiguous() for k, v in self.model.state_dict().items()},
                 "optimiser_state_dict": self.optimiser.state_dict(), "best_loss": self.best_loss,
                 "best_miou": self.metrics["best_miou"], "is_best": is_best}
        if self.scheduler is not None:
            state["scheduler_state_dict"] = self.scheduler.state_dict()
        if self.iou_tracker is not None:             # the adaptive sampler's per-class IoU averages (metrics['iou_values'] of the reference)
            state["iou_values"] = self.iou_tracker.iou_values.detach().cpu().numpy()
        if self.average is not None and self.average.ready:      # the averaged network under the model's own keys, and the averaging record
            avg = self.average.state_dict()
            state["ema"] = avg.pop(WeightAverage.META)
            state["ema_state_dict"] = {k: v.detach().cpu().contiguous() for k, v in avg.items()}
        name = "chkpt_best.pt" if is_best else "chkpt_epoch_{:03d}.pt".format(state["epoch"])
        torch.save(state, base / name)

    def load_checkpoint(self, chkpt_type, averaged=False):
        """averaged (the inference modes): the model takes the checkpoint's 'ema_state_dict' where it has one"""
        names = sorted(f.name for f in (self.log_dir / "chkpts").iterdir())
        name = "chkpt_best.pt"
        if chkpt_type == "best":
            if name not in names:
                raise ValueError("No checkpoint of type 'best' found.")
        elif chkpt_type == "last":
            if "chkpt_epoch_" not in names[-1]:
                raise ValueError("No checkpoint of type 'last' found.")
            name = names[-1]
        ck = torch.load(str(self.log_dir / "chkpts" / name), map_location=self.device, weights_only=False)
        self.model.load_state_dict(ck["ema_state_dict"] if averaged and "ema_state_dict" in ck else ck["model_state_dict"], strict=False)
        if self.config["mode"] == "training":
            self.optimiser.load_state_dict(ck["optimiser_state_dict"])
            if "scheduler_state_dict" in ck:
                self.scheduler.load_state_dict(ck["scheduler_state_dict"])   # (the reference loads the optimiser dict here: a bug)
            self.start_epoch, self.global_step = ck["epoch"], ck["global_step"]
            if "iou_values" in ck:                   # (the tracker is built with the schedule: kept for build_schedule if it comes later)
                self._checkpoint_iou = ck["iou_values"]
                if self.iou_tracker is not None:
                    self.iou_tracker.load_values(ck["iou_values"])
            if self.average is not None:             # (behind the optimiser's state: the count continues from the step count it restored)
                if "ema_state_dict" in ck:
                    self.average.load_state_dict(dict(ck["ema_state_dict"], **{WeightAverage.META: ck["ema"]}))
                else:
                    self.average.reset()
        self.best_loss = ck["best_loss"]
        self.metrics["best_miou"] = ck["best_miou"]

    def write_info_json(self):
        if self.rank != 0:
            return
        cfg = json.loads(json.dumps(self.config, default=str))
        with open(self.log_dir / "info.json", "w") as f:
            json.dump({"config": cfg, "metrics": self.metrics, "history": self.history,
                       "frozen_bn_modules": len(getattr(self.model, "frozen_bn", ()))}, f, indent=1, default=str)
