"""The class-aware train loaders of the reference (managers/BaseManager.py:198-229, 286-405; utils/adaptive_sampling.py) -- CPU-side, no
kernel: they only decide which frames an epoch visits.  Inputs are explicit instead of a pandas frame: ``class_table`` is the int64
[frames, K] table utils.class_info makes of the per-frame class pixel counts (utils.label_census: the census kernel), one column per
network class, the ignore class left out.

Pinned to the reference by tests/golden/class_loaders.npz: get_prob, get_dist, the v1 / v2 weights (bit for bit: the same float32 numpy
expressions), the adaptive batches and the oversampling lists on tables WITHOUT ties.  Not pinned: the order among frames with EQUAL counts
in a column (see AdaptiveBatchSampler), and train_schedule, whose loop lives inside the reference's load_data (hand-written known answers).
"""
import numpy as np
import torch
from torch.utils.data import Sampler

LOADER_TYPES = ("adaptive_batching", "oversampling", "weighted_random", "repeat_factor")

# utils/defaults.py:244-255 of the reference (data restated): preset -> the classes to oversample, per experiment 1..3
OVERSAMPLING_PRESETS = {
    "default": [[3, 5, 7], [7, 8, 15, 16], [19, 20, 22, 24]],
    "rare": [[2], [16, 10, 9, 12, 14], [24, 20, 21, 22, 18, 23, 19, 16, 12, 11, 14]],
}


def softmax(x, theta=1.0, axis=None):
    """utils/utils.py:471-506 of the reference, operation for operation (the probabilities are compared bit for bit)"""
    y = np.atleast_2d(x)
    if axis is None:
        axis = next(j[0] for j in enumerate(y.shape) if j[1] > 1)
    y = y * float(theta)
    y = y - np.expand_dims(np.max(y, axis=axis), axis)
    y = np.exp(y)
    ax_sum = np.expand_dims(np.sum(y, axis=axis), axis)
    p = y / ax_sum
    if len(x.shape) == 1:
        p = p.flatten()
    return p


def ranked_frames(class_table):
    """[K, frames]: per class the frame indices by DESCENDING count (df.sort_values(by=c, ascending=False)); equal counts: the lower frame
    index first -- a build-side rule, see AdaptiveBatchSampler"""
    t = np.asarray(class_table)
    if t.ndim != 2:
        raise ValueError("class_table must be [frames, classes]")
    return np.stack([np.argsort(-t[:, c].astype(np.int64), kind="stable") for c in range(t.shape[1])])


class AdaptiveBatchSampler(Sampler):
    """utils/adaptive_sampling.py:8-64 as a batch sampler over frame indices.  Before every batch the per-class IoU vector ``iou_values``
    (float32 [K], shared with whoever updates it; ``refresh()``, when given, is called first and its result written into it) becomes a
    distribution over classes (get_prob), the distribution a number of frames per class (get_dist), and each of a class's d frames is the
    best-ranked of ``sel_size`` frames drawn from ONE global ``np.random.choice(range(N), d * sel_size, replace=False)`` -- the global
    numpy generator, as in the reference: seed it with np.random.seed.

    Frames are ranked per class by descending pixel count.  TIE ORDER IS A BUILD-SIDE RULE: among frames with equal counts the lower frame
    index ranks first.  The reference's order there is unpinned -- pandas' sort_values uses an unstable sort (quicksort) whose order among
    equal keys depends on the numpy build -- so batches agree with the reference exactly only on columns without ties
    (tests/golden/class_loaders.npz records such tables).  An unknown ``dist_type`` raises; the reference builds a KeyError without raising
    it and fails later on ``None``."""

    DIST_TYPES = ("1/", "1-", "1-**2")

    def __init__(self, class_table, iou_values, dist_type=None, batch_size=None, sel_size=None, refresh=None):
        self.class_table = np.asarray(class_table)
        self.order = ranked_frames(self.class_table)
        self.iou_values = iou_values
        self.dist_type = "1/" if dist_type is None else dist_type
        if self.dist_type not in self.DIST_TYPES:
            raise KeyError("AdaptiveBatchSampler: dist_type '{}' not recognised (one of {})".format(self.dist_type, self.DIST_TYPES))
        self.batch_size = 1 if batch_size is None else batch_size
        self.sel_size = 10 if sel_size is None else sel_size
        self.refresh = refresh
        self.trace = None              # a list here records (IoU vector used, batch) per batch

    def get_prob(self):
        if self.dist_type == "1/":
            iou = np.copy(self.iou_values)
            iou[iou > 0] = iou[iou > 0] ** -1
            return softmax(iou)
        if self.dist_type == "1-":
            return softmax(1 - np.copy(self.iou_values))
        return softmax((1 - np.copy(self.iou_values)) ** 2)

    def get_dist(self, prob):
        ind = np.argsort(prob)[::-1]
        nums = self.batch_size * prob
        sel_nums = np.zeros_like(prob, 'i')
        cum_sum = 0
        for i in ind:
            to_allocate = self.batch_size - cum_sum
            n = int(np.minimum(to_allocate, np.ceil(nums[i])))
            sel_nums[i] = n
            cum_sum += n
            if cum_sum == self.batch_size:
                break
        return sel_nums

    def __iter__(self):
        n_frames = self.class_table.shape[0]
        num_batches = n_frames // self.batch_size
        while num_batches > 0:
            if self.refresh is not None:
                self.iou_values[:] = self.refresh()
            dist = self.get_dist(self.get_prob())
            idx = []
            for i, d in enumerate(dist):
                if d > 0:
                    ind = np.random.choice(range(n_frames), size=d * self.sel_size, replace=False)   # (raises as numpy does when d * sel_size > N)
                    ind = np.min(ind.reshape(d, -1), axis=1)
                    idx.extend(int(v) for v in self.order[i][ind])
            if self.trace is not None:
                self.trace.append((np.array(self.iou_values, dtype=np.float32), list(idx)))
            yield idx
            num_batches -= 1

    def __len__(self):
        return self.class_table.shape[0] // self.batch_size


def oversampled_indices(class_table, class_list, frac):
    """BaseManager.py:330-339: range(N) followed by the frames to repeat -- per class of ``class_list`` the ``sel_per_class_estimate``
    frames with the most pixels of it, concatenated in class order, first occurrence kept (drop_duplicates), the estimate grown until
    int(N * frac) frames are found.  Ties as in AdaptiveBatchSampler (build-side rule)."""
    order = ranked_frames(class_table)
    n = order.shape[1]
    class_list = [int(c) for c in class_list]
    required = int(n * frac)
    if required > n:
        raise ValueError("oversampled_indices: frac {} asks for {} of {} frames (the reference's loop would not end)".format(frac, required, n))
    extend = []
    est = required // len(class_list)
    while len(extend) < required:
        seen, extend = set(), []
        for c in class_list:
            for f in order[c][:est]:
                if int(f) not in seen:
                    seen.add(int(f))
                    extend.append(int(f))
        est += int(np.maximum(1, (required - len(extend)) // len(class_list)))
    return list(range(n)) + extend


def weighted_random_weights(class_table, mode):
    """BaseManager.py:354-372: the per-frame weights of torch's WeightedRandomSampler(weights, N), the reference's float32 expressions"""
    class_abs = np.asarray(class_table).astype('f')
    class_rel_to_class_sum = class_abs / np.sum(class_abs, axis=0)
    class_freq = np.sum(class_abs, axis=0) / np.sum(class_abs)
    if mode == "v1":
        class_weighting = 1 / class_freq
        class_weighting /= np.sum(class_weighting)
        return np.sum(class_abs * class_weighting[np.newaxis, :], axis=1)
    if mode == "v2":
        class_weighting = 1 - class_freq
        return np.sum(class_rel_to_class_sum * class_weighting, axis=1)
    raise ValueError("Mode '{}' not recognised.".format(mode))      # (the reference builds this error without raising it)


def train_schedule(data_config, epochs):
    """BaseManager.py:67-70, 203-211: epoch -> loader name.  Every epoch starts as 'train_loader'; the four loader types are applied in
    argsort order of their start epochs, each over range(*config[type]) -- a one-element [start] is extended to [start, epochs] IN the
    configuration, as the reference does -- so that of two overlapping ranges the one that starts later wins."""
    schedule = {i: "train_loader" for i in range(epochs)}
    starts = [data_config[t][0] for t in LOADER_TYPES]
    for t in np.array(LOADER_TYPES)[np.argsort(starts)]:
        t = str(t)
        if len(data_config[t]) == 1:
            data_config[t].extend([epochs])
        for i in range(*data_config[t]):
            schedule[i] = "train_" + t + "_loader"
    return schedule


class ShuffledIndexList(Sampler):
    """a fresh permutation of a fixed index list per epoch, from a private generator: the oversampling loader's DataLoader(shuffle=True)
    over the extended frame list.  The stream is the same on every rank, so dist.ShardedSampler can shard it."""

    def __init__(self, indices, seed=0):
        self.indices = torch.as_tensor(list(indices), dtype=torch.int64)
        self.g = torch.Generator()
        self.g.manual_seed(int(seed))

    def __iter__(self):
        return iter(self.indices[torch.randperm(len(self.indices), generator=self.g)].tolist())

    def __len__(self):
        return len(self.indices)
