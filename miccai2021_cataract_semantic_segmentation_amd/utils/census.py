"""The class table of the class-aware train loaders, taken from the label maps themselves, and the device-side IoU average that adaptive
batching feeds on.

The reference reads per-frame class pixel counts from the 36 canonical-class columns of data/data.csv, which
utils/data_class_analysis.py:get_class_numbers wrote offline (36 ``np.sum(label == i)`` passes per frame).  Here the raw uint8 label maps
go through the census kernel (csrc/census.hip) on their way to the device: ``label_census`` returns the same [frames, 36] table, and
``class_info`` / ``presence_of`` / ``class_sums_of`` make of it what the samplers and crop_mode 'freq' take.

``IoUTracker`` holds what OCRNet_Manager.py:108-117 keeps on the host -- the per-class IoU of every training batch, averaged
exponentially -- as device state behind one capturable launch, and hands the host K floats per step."""
import numpy as np
import torch

from .classes import CLASS_REMAP


def _frames_of(labels):
    """the label maps of `labels` one after the other: a dataset (dataset[i][1] is the map) or an iterable of [H, W] / [b, H, W] maps"""
    plain = isinstance(labels, (list, tuple, np.ndarray, torch.Tensor))
    if not plain and hasattr(labels, "__getitem__") and hasattr(labels, "__len__"):
        source = (labels[i][1] for i in range(len(labels)))
    else:
        source = iter(labels)
    for m in source:
        m = m.detach().cpu().numpy() if isinstance(m, torch.Tensor) else np.asarray(m)
        if m.dtype != np.uint8 or m.ndim not in (2, 3):
            raise ValueError("label_census: label maps must be uint8 [H, W] or [b, H, W] (got {} {})".format(m.dtype, m.shape))
        for f in (m if m.ndim == 3 else m[None]):
            yield f


def label_census(labels, nbins=36, lut=None, device=None, chunk=64, allow_other=False):
    """per-frame class pixel counts: numpy int64 [N, nbins].  labels: an iterable of uint8 arrays / tensors [H, W] or [b, H, W], or a
    dataset whose dataset[i][1] is the uint8 label map; lut: 256 uint8 entries applied before counting, or None.  Frames are uploaded
    ``chunk`` at a time (frames of one chunk share a shape), counted by ops.label_census, and the whole table comes back in ONE readback.
    A pixel whose value is >= nbins is the reference's "Unknown class found": it raises unless allow_other=True."""
    from .. import ops
    device = torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)
    lut_d = None
    if lut is not None:
        lut_d = torch.as_tensor(np.asarray(lut, dtype=np.uint8).reshape(256)).to(device)
    parts, pending = [], []

    def flush():
        if pending:
            batch = torch.from_numpy(np.ascontiguousarray(np.stack(pending))).to(device, non_blocking=True)
            parts.append(ops.label_census(batch, nbins, lut_d))
            del pending[:]

    for f in _frames_of(labels):
        if pending and (len(pending) >= int(chunk) or pending[0].shape != f.shape):
            flush()
        pending.append(f)
    flush()
    if not parts:
        return np.zeros((0, nbins), dtype=np.int64)
    table = torch.cat(parts).cpu().numpy()
    if not allow_other and table[:, nbins].any():
        bad = np.nonzero(table[:, nbins])[0]
        raise ValueError("label_census: Unknown class found: {} frame(s) hold values >= {} (first: frame {}, {} pixels)".format(
            len(bad), nbins, int(bad[0]), int(table[bad[0], nbins])))
    return np.ascontiguousarray(table[:, :nbins])


def class_info(table36, experiment):
    """utils/utils.py:577-588 (get_class_info) on the table: int64 [N, K], column c = the sum of the canonical columns the experiment maps
    to network class c; the ignore class (key 255) is left out"""
    t = np.asarray(table36, dtype=np.int64)
    remap = CLASS_REMAP[experiment]
    return np.stack([t[:, remap[c]].sum(1) for c in sorted(k for k in remap if k != 255)], 1)


def presence_of(table36):
    """bool [N, 36]: canonical class present in the frame -- utils.RepeatFactorSampler's ``presence``"""
    return np.asarray(table36) > 0


def class_sums_of(table36):
    """int64 [36]: pixels per canonical class over all frames -- crop['class_sums'] of crop_mode 'freq' (utils.class_frequencies)"""
    return np.asarray(table36, dtype=np.int64).sum(0)


class _DeviceBackend:
    """what IoUTracker needs of the device (tests replace it to check the lag logic without one)"""

    def __init__(self, device):
        self.device = torch.device(device)

    def state(self, K):
        return (torch.zeros((K, K), dtype=torch.int32, device=self.device), torch.full((K,), 0.5, dtype=torch.float32, device=self.device))

    def launch(self, running_cm, cm_prev, iou_values, update):
        from .. import ops
        ops.iou_ema(running_cm, cm_prev, iou_values, update)

    def slot(self, K):
        return torch.full((K,), 0.5, dtype=torch.float32).pin_memory()

    def copy(self, iou_values, slot):
        slot.copy_(iou_values, non_blocking=True)

    def view(self, slot):
        return slot.numpy()

    def event(self):
        return torch.cuda.Event()

    def record(self, event):
        event.record(torch.cuda.current_stream(self.device))


class IoUTracker:
    """per-class IoU of every training batch, exponentially averaged, on the device (OCRNet_Manager.py:108-117; iou_values start at 0.5,
    BaseManager.py:313).  The manager keeps ONE running confusion matrix per epoch; the batch's own matrix is its difference to ``cm_prev``.

    step(running_cm)  one launch (ops.iou_ema) on the current stream: no host decision, it can sit inside a captured training step;
    publish()         OUTSIDE any capture, on the step's stream: an asynchronous copy of the K floats into a pinned buffer, and an event;
    host()            float32 [K] view of the averages after step n - lag, n the number of published steps: lag 0 waits for the last step
                      (the reference's semantics: batch n + 1 is drawn from the IoU of batch n), lag 1 for the step before it -- the
                      host then never waits on the step that is running.  Before enough steps were published: the starting values;
    reset()           at epoch start, when the manager makes a fresh running matrix: cm_prev = 0.  The averages carry over."""

    def __init__(self, K, update, device=None, lag=0, backend=None):
        if int(lag) not in (0, 1):
            raise ValueError("IoUTracker: lag must be 0 or 1")
        self.K, self.update, self.lag = int(K), update, int(lag)
        self.backend = backend if backend is not None else _DeviceBackend(device)
        self.cm_prev, self.iou_values = self.backend.state(self.K)
        self.slots = [self.backend.slot(self.K) for _ in range(self.lag + 2)]      # the slot host() reads is never the next copy's target
        self.events = [self.backend.event() for _ in self.slots]
        self.initial = np.full(self.K, 0.5, dtype=np.float32)
        self.published = 0

    def step(self, running_cm):
        self.backend.launch(running_cm, self.cm_prev, self.iou_values, self.update)

    def publish(self):
        i = self.published % len(self.slots)
        self.backend.copy(self.iou_values, self.slots[i])
        self.backend.record(self.events[i])
        self.published += 1

    def host(self):
        n = self.published - self.lag
        if n <= 0:
            return self.initial
        i = (n - 1) % len(self.slots)
        self.events[i].synchronize()
        return self.backend.view(self.slots[i])

    def reset(self):
        self.cm_prev.zero_()

    # the device state a warm-up must put back (graph.GraphedTrainStep) and a checkpoint carries
    def save(self):
        return self.cm_prev.clone(), self.iou_values.clone()

    def restore(self, saved):
        self.cm_prev.copy_(saved[0])
        self.iou_values.copy_(saved[1])

    def load_values(self, values):
        """(a checkpoint's averages) -> the device state and the value host() starts from"""
        v = np.asarray(values, dtype=np.float32).reshape(self.K)
        self.iou_values.copy_(torch.from_numpy(v.copy()))
        self.initial = v.copy()
        self.published = 0
