"""The per-epoch loader schedule in a manager run: a tiny UNet under the FCN manager, 12 frames of 40 x 56, batch 2, three epochs scheduled
default -> adaptive batching -> oversampling.  Every batch's frame indices equal a host replay of the samplers fed with the IoU vectors the
tracker published; the published vectors and the final averages equal a numpy replay from the per-batch confusion matrices (bit for bit);
hip_graph on and off give the same batches and the same parameter bits; a checkpoint carries the averages; the refusals name their reason."""

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

N, H, W, BATCH, SEL, UPDATE = 12, 40, 56, 2, 3, 0.3
KNET, KREAL = 18, 17          # UNet predicts the ignore class too: an 18 x 18 confusion matrix; the sampler takes experiment 2's 17 classes


def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")


class _Logged(torch.utils.data.Dataset):
    """the synthetic frames, with a record of the indices asked for"""

    def __init__(self, inner):
        self.inner, self.log = inner, []

    def __len__(self):
        return len(self.inner)

    def __getitem__(self, i):
        self.log.append(int(i))
        return self.inner[i]

    def raw_labels(self):
        return self.inner.raw_labels()


def _cfg(log_path, hip_graph, lag):
    return {"name": "sched", "mode": "training", "manager": "FCN", "log_path": str(log_path), "graph": {"model": "UNet"},
            "data": {"experiment": 2, "batch_size": BATCH, "adaptive_batching": [1, 2], "oversampling": [2], "adaptive_sel_size": SEL,
                     "adaptive_iou_update": UPDATE, "adaptive_iou_lag": lag},
            "loss": {"name": "LovaszSoftmax"}, "train": {"learning_rate": 1e-3, "epochs": 3, "hip_graph": hip_graph},
            "log_every_n_epochs": 1, "seed": 0}


_RUNS = {}


def _run(tmp_path_factory, hip_graph, lag):
    """one three-epoch run; shared by the tests below"""
    key = (hip_graph, lag)
    if key in _RUNS:
        return _RUNS[key]
    from miccai2021_cataract_semantic_segmentation_amd import managers
    tr = _Logged(managers.SyntheticCataractDataset(N, H, W, 17, seed=3, patch=8))
    va = managers.SyntheticCataractDataset(2, H, W, 17, seed=4, patch=8)
    torch.manual_seed(0)
    m = managers.FCNManager(_cfg(tmp_path_factory.mktemp("sched"), hip_graph, lag), tr, va)
    m.train_loader, m.valid_loader = m.loaders()
    m.build_schedule()
    assert m.train_schedule == {0: "train_loader", 1: "train_adaptive_batching_loader", 2: "train_oversampling_loader"}
    assert m.config["data"]["oversampling"] == [2, 3]
    m.adaptive_sampler.trace = []
    tracker = m.iou_tracker
    running, publish = [], tracker.publish

    def recording_publish():                       # (outside any capture, behind the step: cm_prev is the running matrix now)
        publish()
        running.append(tracker.cm_prev.cpu().numpy().copy())

    tracker.publish = recording_publish
    epochs = []
    for m.epoch in range(3):
        torch.manual_seed(100 + m.epoch)           # the default loader's shuffle
        np.random.seed(11 + m.epoch)               # the adaptive sampler's draws
        first, steps = len(tr.log), len(running)
        m.train_one_epoch()
        epochs.append({"indices": tr.log[first:], "running": running[steps:]})
        m.validate()
    out = {"manager": m, "train_set": tr, "epochs": epochs, "params": m.model.flat().flat.detach().cpu().clone(),
           "iou_values": tracker.iou_values.cpu().numpy().copy(), "trace": list(m.adaptive_sampler.trace)}
    _RUNS[key] = out
    return out


def _iou_of(cm):
    """t_get_mean_iou(cm, experiment, calculate_mean=False) in numpy float32 (exact integers below 2^24)"""
    d, r, s = np.diag(cm).astype(np.float32), cm.sum(0).astype(np.float32), cm.sum(1).astype(np.float32)
    with np.errstate(invalid="ignore", divide="ignore"):
        iou = d / ((r + s) - d)
    iou[iou != iou] = 0
    return iou


def _replayed_values(run):
    """the averages after every step of the run, from the per-batch confusion matrices"""
    vals, seq = np.ones(KNET, 'f') * .5, []
    for ep in run["epochs"]:
        prev = np.zeros((KNET, KNET), dtype=np.int64)
        for cm in ep["running"]:
            batch = cm.astype(np.int64) - prev
            assert 0 < batch.sum() <= BATCH * H * W and batch.min() >= 0      # (pixels that carry the ignore id are not counted)
            prev = cm.astype(np.int64)
            vals = np.float32(1 - UPDATE) * vals + np.float32(UPDATE) * _iou_of(batch)
            seq.append(vals.copy())
    return seq


@pytest.mark.parametrize("hip_graph,lag", [(False, 0), (True, 0), (False, 1)], ids=["eager", "hip_graph", "eager, lag 1"])
def test_scheduled_run_equals_the_host_replay(tmp_path_factory, hip_graph, lag):
    _need_gpu()
    from miccai2021_cataract_semantic_segmentation_amd.utils import (OVERSAMPLING_PRESETS, AdaptiveBatchSampler, class_info,
                                                                     oversampled_indices)
    run = _run(tmp_path_factory, hip_graph, lag)
    m, e = run["manager"], run["epochs"]
    table = m.class_table()
    maps = np.stack(list(m.train_set.raw_labels()))
    assert np.array_equal(table[:, :18], np.stack([np.bincount(f.reshape(-1), minlength=18) for f in maps]))      # the census of the frames
    assert table[:, 18:].sum() == 0
    # epoch 0: the default loader -- every frame once
    assert sorted(e[0]["indices"]) == list(range(N)) and len(e[0]["running"]) == N // BATCH
    # the averages, step by step, from the per-batch confusion matrices
    seq = _replayed_values(run)
    assert len(seq) == sum(len(ep["running"]) for ep in e)
    assert np.array_equal(run["iou_values"].view(np.uint32), seq[-1].view(np.uint32))
    # epoch 1: adaptive batches = a host replay of the sampler fed with the vectors the tracker published
    trace = run["trace"]
    assert len(trace) == N // BATCH and [i for _, b in trace for i in b] == e[1]["indices"]
    steps0 = len(e[0]["running"])
    for b, (vec, _) in enumerate(trace):           # batch b is drawn after steps0 + b steps; the host sees the step `lag` before that
        n = steps0 + b - lag
        want = seq[n - 1][:KREAL].copy() if n > 0 else np.ones(KREAL, 'f') * .5
        assert vec.shape == (KREAL,) and np.array_equal(vec.view(np.uint32), want.view(np.uint32)), (b, lag)
    vals = np.ones(KREAL, 'f') * .5
    replay = AdaptiveBatchSampler(class_info(table, 2), vals, "1-**2", BATCH, SEL)
    np.random.seed(12)
    it = iter(replay)
    for vec, batch in trace:
        vals[:] = vec
        assert next(it) == batch
    assert len(set(map(tuple, (b for _, b in trace)))) > 1
    # epoch 2: every frame once and the oversampled frames, shuffled; whole batches only
    want = oversampled_indices(class_info(table, 2), OVERSAMPLING_PRESETS["default"][1], 0.2)
    assert len(want) >= N + int(N * 0.2)
    got = e[2]["indices"]
    assert len(got) == len(want) // BATCH * BATCH
    extra = sorted(want)
    for i in got:
        extra.remove(i)                            # a sub-multiset of the extended list
    assert len(extra) == len(want) - len(got)


def test_hip_graph_and_eager_agree_bit_for_bit(tmp_path_factory):
    _need_gpu()
    eager, graph = _run(tmp_path_factory, False, 0), _run(tmp_path_factory, True, 0)
    assert [ep["indices"] for ep in eager["epochs"]] == [ep["indices"] for ep in graph["epochs"]]
    assert torch.equal(eager["params"], graph["params"])
    assert np.array_equal(eager["iou_values"].view(np.uint32), graph["iou_values"].view(np.uint32))
    for a, b in zip(eager["epochs"], graph["epochs"]):
        assert all(np.array_equal(x, y) for x, y in zip(a["running"], b["running"]))


def test_checkpoint_carries_the_averages(tmp_path_factory):
    _need_gpu()
    from miccai2021_cataract_semantic_segmentation_amd import managers
    run = _run(tmp_path_factory, False, 0)
    m = run["manager"]
    ck = torch.load(str(m.log_dir / "chkpts" / "chkpt_epoch_002.pt"), weights_only=False)
    assert np.array_equal(ck["iou_values"].view(np.uint32), run["iou_values"].view(np.uint32))
    m2 = managers.FCNManager(_cfg(m.log_dir.parent, False, 0), run["train_set"].inner, None)
    m2.log_dir = m.log_dir
    m2.load_checkpoint("last")
    m2.train_loader, m2.valid_loader = m2.loaders()
    m2.build_schedule()
    assert torch.equal(m2.iou_tracker.iou_values.cpu(), torch.from_numpy(run["iou_values"]))
    assert np.array_equal(m2.iou_tracker.host(), run["iou_values"]) and np.array_equal(m2.adaptive_sampler.iou_values, run["iou_values"][:KREAL])
    assert torch.equal(m2.model.flat().flat.cpu(), run["params"]) and m2.start_epoch == 2


def test_weighted_random_and_repeat_factor_loaders_are_built(tmp_path):
    _need_gpu()
    from miccai2021_cataract_semantic_segmentation_amd import managers
    from miccai2021_cataract_semantic_segmentation_amd.utils import RepeatFactorSampler
    cfg = _cfg(tmp_path, False, 0)
    cfg["data"].update({"adaptive_batching": [0, 0], "oversampling": [0, 0], "weighted_random": [0, 1], "weighted_random_mode": "v2",
                        "repeat_factor": [1],
                        # the table from the configuration; every class present (an absent class makes the reference's weights 0 / 0)
                        "label_table": np.random.RandomState(2).randint(1, 500, (N, 36))})
    m = managers.FCNManager(cfg, managers.SyntheticCataractDataset(N, H, W, 17, seed=3, patch=8), None)
    m.train_loader, m.valid_loader = m.loaders()
    m.build_schedule()
    assert m.train_schedule == {0: "train_weighted_random_loader", 1: "train_repeat_factor_loader", 2: "train_repeat_factor_loader"}
    assert m.iou_tracker is None and np.array_equal(m.class_table(), cfg["data"]["label_table"])
    wl, rl = m.data_loaders["train_weighted_random_loader"], m.data_loaders["train_repeat_factor_loader"]
    assert isinstance(wl.sampler, torch.utils.data.WeightedRandomSampler) and len(wl.sampler.weights) == N
    assert isinstance(rl.sampler, RepeatFactorSampler)
    img, lbl, _ = next(iter(wl))
    assert tuple(img.shape) == (BATCH, 3, H, W) and tuple(lbl.shape) == (BATCH, H, W)
    assert len(list(rl)) >= N // BATCH


def test_refusals_carry_their_reasons(tmp_path):
    _need_gpu()
    from miccai2021_cataract_semantic_segmentation_amd import dist, managers
    from miccai2021_cataract_semantic_segmentation_amd.utils import (OVERSAMPLING_PRESETS, AdaptiveBatchSampler, PinnedFrameLoader, class_info,
                                                                     oversampled_indices)
    tr = managers.SyntheticCataractDataset(N, H, W, 17, seed=3, patch=8)
    m = managers.FCNManager(_cfg(tmp_path, False, 0), tr, None)
    m.train_loader, m.valid_loader = m.loaders()
    m.world = 2                                    # (what a second rank would see)
    with pytest.raises(ValueError, match="adaptive batching is refused with WORLD_SIZE > 1.*own numpy generator"):
        m.scheduled_loader("train_adaptive_batching_loader")
    with pytest.raises(ValueError, match="weighted-random loader is refused with WORLD_SIZE > 1.*cannot be sharded"):
        m.scheduled_loader("train_weighted_random_loader")
    shards = []
    for m.rank in (0, 1):                          # oversampling works: the same shuffled list on every rank, sharded
        loader = m.scheduled_loader("train_oversampling_loader")
        assert isinstance(loader.sampler, dist.ShardedSampler)
        shards.append(list(loader.sampler))
    want = oversampled_indices(class_info(m.class_table(), 2), OVERSAMPLING_PRESETS["default"][1], 0.2)
    assert len(shards[0]) == len(shards[1]) == len(want) // (2 * BATCH) * BATCH
    rest = sorted(want)
    for i in shards[0] + shards[1]:
        rest.remove(i)                             # the two shards are disjoint pieces of ONE shuffled copy of the extended list
    m.world, m.rank = 1, 0
    sampler = AdaptiveBatchSampler(np.ones((N, 17), dtype=np.int64), np.ones(17, 'f') * .5, "1-**2", BATCH, SEL)
    with pytest.raises(ValueError, match="adaptive batches are refused.*ahead"):
        PinnedFrameLoader(tr, BATCH, 2, sampler=sampler)

    class _Bare(torch.utils.data.Dataset):         # no table, no raw labels
        def __len__(self):
            return N

        def __getitem__(self, i):
            return tr[i]

    m3 = managers.FCNManager(_cfg(tmp_path, False, 0), _Bare(), None)
    m3.train_loader, m3.valid_loader = m3.loaders()
    with pytest.raises(ValueError, match=r"label_table.*train_set\.label_table.*raw_labels"):
        m3.build_schedule()
    with pytest.raises(ValueError, match=r"must be \[12, 36\]"):
        m4 = managers.FCNManager(dict(_cfg(tmp_path, False, 0), data=dict(_cfg(tmp_path, False, 0)["data"], label_table=np.zeros((5, 36)))),
                                 tr, None)
        m4.train_loader, m4.valid_loader = m4.loaders()
        m4.build_schedule()
