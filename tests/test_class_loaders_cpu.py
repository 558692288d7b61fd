"""Host side of the class-aware train loaders (utils/class_sampling.py, utils/census.py) against what the REAL reference computed
(tests/golden/class_loaders.npz, written by tests/golden/make_golden_class_loaders.py): get_class_info, get_prob / get_dist, the v1 / v2
weights, adaptive batch sequences and oversampling lists on tie-free tables, every item EXACTLY (probabilities and weights bit for bit).
The schedule loop cannot be called in the reference (it sits inside load_data): it is pinned to hand-written known answers.  Also: the
IoUTracker's lag logic with a fake event source, and the C ABI of include/catseg_census.h."""
import functools
import os

import numpy as np
import pytest

import _abi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DIST_NAMES = (("1/", "inv"), ("1-", "one_minus"), ("1-**2", "one_minus_sq"))
K_EXP = ((8, 1), (17, 2), (25, 3))


@functools.lru_cache(maxsize=None)
def _fixture():
    return np.load(os.path.join(ROOT, "tests", "golden", "class_loaders.npz"))


def _bits(a):
    a = np.ascontiguousarray(a)
    assert a.dtype == np.float32
    return a.view(np.uint32)


# ---- (a) data.csv
@pytest.mark.parametrize("experiment", [1, 2, 3])
def test_class_info_equals_get_class_info(experiment):
    from miccai2021_cataract_semantic_segmentation_amd.utils import NUM_CLASSES, class_info
    g = _fixture()
    got = class_info(g["table36"], experiment)
    real = NUM_CLASSES[experiment]
    assert got.dtype == np.int64 and got.shape == (len(g["table36"]), real)
    assert np.array_equal(got, g["e%d_class_info" % experiment])


def test_presence_and_class_sums_of_the_table():
    from miccai2021_cataract_semantic_segmentation_amd.utils import class_sums_of, presence_of
    t = _fixture()["table36"]
    assert presence_of(t).dtype == np.bool_ and np.array_equal(presence_of(t), t > 0)
    assert class_sums_of(t).dtype == np.int64 and np.array_equal(class_sums_of(t), t.sum(0))


@pytest.mark.parametrize("K", [8, 17, 25])
def test_get_prob_and_get_dist_bit_for_bit(K):
    from miccai2021_cataract_semantic_segmentation_amd.utils import AdaptiveBatchSampler
    g = _fixture()
    table = np.zeros((40, K), dtype=np.int64)
    for dist_type, name in DIST_NAMES:
        for vi, v in enumerate(g["k%d_iou_vectors" % K]):
            s = AdaptiveBatchSampler(table, v.copy(), dist_type, 1, 1)
            p = s.get_prob()
            assert np.array_equal(_bits(p), _bits(g["k%d_prob_%s" % (K, name)][vi])), (dist_type, vi)
            for bi, bs in enumerate((1, 4, 8, 10)):
                s.batch_size = bs
                d = s.get_dist(p)
                assert d.dtype == np.int32 and int(d.sum()) == bs
                assert np.array_equal(d, g["k%d_dist_%s" % (K, name)][vi, bi]), (dist_type, vi, bs)


@pytest.mark.parametrize("experiment", [1, 2, 3])
@pytest.mark.parametrize("mode", ["v1", "v2"])
def test_weighted_random_weights_bit_for_bit(experiment, mode):
    from miccai2021_cataract_semantic_segmentation_amd.utils import weighted_random_weights
    g = _fixture()
    w = weighted_random_weights(g["e%d_class_info" % experiment], mode)
    assert np.array_equal(_bits(w), _bits(g["e%d_weights_%s" % (experiment, mode)]))


def test_unknown_modes_raise():
    from miccai2021_cataract_semantic_segmentation_amd.utils import AdaptiveBatchSampler, weighted_random_weights
    with pytest.raises(ValueError, match="not recognised"):
        weighted_random_weights(np.ones((4, 3), dtype=np.int64), "v3")
    with pytest.raises(KeyError, match="not recognised"):
        AdaptiveBatchSampler(np.ones((4, 3), dtype=np.int64), np.full(3, 0.5, 'f'), "1+", 2, 1)


# ---- (b) tie-free tables
@pytest.mark.parametrize("K", [8, 17, 25])
def test_adaptive_batches_equal_the_reference(K):
    from miccai2021_cataract_semantic_segmentation_amd.utils import AdaptiveBatchSampler
    g = _fixture()
    table = g["k%d_table" % K]
    for c in range(K):
        assert len(np.unique(table[:, c])) == len(table)          # the comparison is exact only without ties
    batch, sel = (int(v) for v in g["k%d_adaptive_params" % K])
    for si, seed in enumerate(g["k%d_adaptive_seeds" % K]):
        vals = np.ones(K, 'f') * .5
        s = AdaptiveBatchSampler(table, vals, "1-**2", batch, sel)
        assert len(s) == len(table) // batch
        np.random.seed(int(seed))
        it = iter(s)
        for b, want in enumerate(g["k%d_adaptive_batches" % K][si]):
            vals[:] = g["k%d_adaptive_ious" % K][si, b]
            assert next(it) == [int(v) for v in want], (K, seed, b)


def test_adaptive_refresh_is_called_before_every_batch_and_traced():
    from miccai2021_cataract_semantic_segmentation_amd.utils import AdaptiveBatchSampler
    g = _fixture()
    table, ious = g["k8_table"], g["k8_adaptive_ious"][1]
    calls = []

    def refresh():
        calls.append(len(calls))
        return ious[len(calls) - 1]

    s = AdaptiveBatchSampler(table, np.ones(8, 'f') * .5, "1-**2", 4, 5, refresh=refresh)
    s.trace = []
    np.random.seed(1)
    it = iter(s)
    got = [next(it) for _ in range(len(ious))]
    assert calls == list(range(len(ious)))
    assert got == [[int(v) for v in b] for b in g["k8_adaptive_batches"][1]]
    assert [t[1] for t in s.trace] == got and all(np.array_equal(t[0], ious[i]) for i, t in enumerate(s.trace))


def test_more_draws_than_frames_raise_as_numpy_does():
    from miccai2021_cataract_semantic_segmentation_amd.utils import AdaptiveBatchSampler
    table = np.stack([np.random.RandomState(0).permutation(12) for _ in range(3)], 1)
    s = AdaptiveBatchSampler(table, np.array([0.0, 1.0, 1.0], 'f'), "1-", 8, 3)      # class 0 takes ceil(8 p) frames: 3 d > 12
    with pytest.raises(ValueError, match="larger sample than population"):
        next(iter(s))


@pytest.mark.parametrize("K,experiment", K_EXP)
def test_oversampled_indices_equal_the_reference(K, experiment):
    from miccai2021_cataract_semantic_segmentation_amd.utils import OVERSAMPLING_PRESETS, oversampled_indices
    g = _fixture()
    table = g["k%d_table" % K]
    for preset in ("default", "rare"):
        class_list = OVERSAMPLING_PRESETS[preset][experiment - 1]
        assert list(g["e%d_preset_%s" % (experiment, preset)]) == class_list
        for frac in (0.2, 0.5):
            want = g["k%d_oversampled_%s_%d" % (K, preset, int(frac * 100))]
            got = oversampled_indices(table, class_list, frac)
            assert got == [int(v) for v in want], (K, preset, frac)
            assert got[:len(table)] == list(range(len(table))) and len(got) >= len(table) + int(len(table) * frac)


def test_ties_rank_the_lower_frame_first():
    """the build-side rule (the reference's order among equal counts is unpinned: pandas' sort_values is not stable)"""
    from miccai2021_cataract_semantic_segmentation_amd.utils.class_sampling import ranked_frames
    table = np.array([[5, 0], [9, 0], [5, 1], [9, 0], [1, 0]])
    assert ranked_frames(table).tolist() == [[1, 3, 0, 2, 4], [2, 0, 1, 3, 4]]


def test_oversampling_growth_loop_by_hand():
    """required = int(5 * 0.6) = 3, two classes: estimate 1 gives frames [1] + [2] = 2 < 3; the estimate grows by max(1, (3 - 2) // 2) = 1;
    estimate 2 gives [1, 3] + [2, 0] = 4 >= 3: ALL four are appended (the reference does not cut the list back to `required`)"""
    from miccai2021_cataract_semantic_segmentation_amd.utils.class_sampling import oversampled_indices
    table = np.array([[5, 0], [9, 0], [5, 1], [9, 0], [1, 0]])
    assert oversampled_indices(table, [0, 1], 0.6) == [0, 1, 2, 3, 4, 1, 3, 2, 0]
    with pytest.raises(ValueError, match="would not end"):
        oversampled_indices(table, [0, 1], 1.5)


# ---- the schedule: hand-written known answers (BaseManager.py:67-70, 203-211 read by eye)
def _data(**kw):
    d = {"adaptive_batching": [0, 0], "oversampling": [0, 0], "weighted_random": [0, 0], "repeat_factor": [0, 0]}
    d.update(kw)
    return d


def test_schedule_known_answers():
    from miccai2021_cataract_semantic_segmentation_amd.utils import train_schedule
    assert train_schedule(_data(), 4) == {i: "train_loader" for i in range(4)}
    # a one-element [start] extends to `epochs`, in the configuration too
    cfg = _data(oversampling=[2])
    assert train_schedule(cfg, 5) == {0: "train_loader", 1: "train_loader", 2: "train_oversampling_loader", 3: "train_oversampling_loader",
                                      4: "train_oversampling_loader"}
    assert cfg["oversampling"] == [2, 5]
    # default -> adaptive -> oversampling
    assert train_schedule(_data(adaptive_batching=[1, 2], oversampling=[2, 3]), 3) == {
        0: "train_loader", 1: "train_adaptive_batching_loader", 2: "train_oversampling_loader"}
    # overlapping ranges resolve in argsort order of the starts: the range that starts later is written later and wins
    s = train_schedule(_data(repeat_factor=[0, 4], weighted_random=[2, 6], adaptive_batching=[3, 4]), 6)
    assert s == {0: "train_repeat_factor_loader", 1: "train_repeat_factor_loader", 2: "train_weighted_random_loader",
                 3: "train_adaptive_batching_loader", 4: "train_weighted_random_loader", 5: "train_weighted_random_loader"}
    # a range past the last epoch leaves its entries in the dictionary, as the reference does
    assert train_schedule(_data(oversampling=[1, 4]), 2)[3] == "train_oversampling_loader"


# ---- (c) the update in numpy: the restatement the GPU test's kernel is compared with is itself the fixture's
@pytest.mark.parametrize("K", [8, 17, 25])
def test_fixture_update_sequences_are_the_float32_expression(K):
    g = _fixture()
    cms, ious = g["k%d_cms" % K], g["k%d_cm_iou" % K]
    assert cms.dtype == np.int32 and all(0 < int(m.sum()) < 2 ** 24 for m in cms)
    assert ((cms.sum(1) + cms.sum(2)) == 0).any(), "no absent class in the fixture"
    for a, name in ((1, "1"), (0.3, "03"), (0, "0")):
        vals = np.ones(K, 'f') * .5
        for t in range(len(cms)):
            vals = np.float32(1 - a) * vals + np.float32(a) * ious[t]
            assert np.array_equal(_bits(vals), _bits(g["k%d_ema_a%s" % (K, name)][t]))


# ---- the tracker's lag logic, without a device
class _FakeEvent:
    def __init__(self, log):
        self.log, self.recorded = log, None

    def synchronize(self):
        self.log.append(("wait", self.recorded))


class _FakeBackend:
    """device state as numpy arrays; a 'launch' adds 1 to every average, so that the value identifies the step"""

    def __init__(self):
        self.log, self.steps = [], 0

    def state(self, K):
        return np.zeros((K, K), np.int32), np.full(K, 0.5, np.float32)

    def launch(self, running_cm, cm_prev, iou_values, update):
        self.steps += 1
        iou_values += 1

    def slot(self, K):
        return np.full(K, -1.0, np.float32)

    def copy(self, iou_values, slot):
        slot[:] = iou_values

    def view(self, slot):
        return slot

    def event(self):
        return _FakeEvent(self.log)

    def record(self, event):
        event.recorded = self.steps


@pytest.mark.parametrize("lag", [0, 1])
def test_tracker_lag(lag):
    from miccai2021_cataract_semantic_segmentation_amd.utils import IoUTracker
    be = _FakeBackend()
    t = IoUTracker(3, 0.3, lag=lag, backend=be)
    assert np.array_equal(t.host(), np.full(3, 0.5, np.float32)) and be.log == []      # nothing published: the starting values, no wait
    seen = []
    for step in range(1, 6):
        t.step(None)
        t.publish()
        v = t.host()
        seen.append(float(v[0]))
        want_step = step - lag
        if want_step <= 0:
            assert be.log == []                                   # lag 1, first step: no wait at all
        else:
            assert be.log[-1] == ("wait", want_step)              # the event of step n - lag, never the running step's at lag 1
    assert seen == [0.5 + max(s - lag, 0) for s in range(1, 6)]
    with pytest.raises(ValueError):
        IoUTracker(3, 0.3, lag=2, backend=be)


def test_tracker_never_overwrites_the_slot_the_host_reads():
    from miccai2021_cataract_semantic_segmentation_amd.utils import IoUTracker
    for lag in (0, 1):
        t = IoUTracker(2, 1, lag=lag, backend=_FakeBackend())
        t.step(None)
        t.publish()
        t.step(None)
        t.publish()
        view = t.host()
        kept = view.copy()
        t.step(None)
        t.publish()                                               # the next copy goes to another slot
        assert np.array_equal(view, kept)


# ---- the C ABI of include/catseg_census.h
EINVAL = 1
A = [0x10000 * (i + 1) for i in range(8)]     # fake device pointers: a refusal returns before anything is launched


def test_census_signature_table_matches_the_header():
    from miccai2021_cataract_semantic_segmentation_amd import _lib
    protos = _abi.prototypes("catseg_census.h")
    assert sorted(protos) == ["catseg_iou_ema", "catseg_label_census_u8"]
    for name, (res, args, _) in protos.items():
        assert _lib._SIGS[name] == (res, args), "%s: header %r, _lib._SIGS %r" % (name, (res, args), _lib._SIGS[name])
        assert hasattr(_lib.lib, name)


def _census_args(**kw):
    f = dict(lbl=A[0], B=2, H=5, W=7, lut=None, nbins=36, counts=A[1], accumulate=0, stream=None)
    f.update(kw)
    return tuple(f.values())


def _ema_args(**kw):
    f = dict(cm_running=A[0], cm_prev=A[1], K=8, w_old=0.7, w_new=0.3, iou_values=A[2], iou_batch=None, stream=None)
    f.update(kw)
    return tuple(f.values())


CENSUS_DEFECTS = [
    ("B = 0", dict(B=0), b"bad dims"),
    ("H = 0", dict(H=0), b"bad dims"),
    ("W < 0", dict(W=-3), b"bad dims"),
    ("too many frames", dict(B=70000), b"bad dims"),
    ("a frame of 2^31 pixels", dict(H=65536, W=32768), b"2^31"),
    ("nbins = 0", dict(nbins=0), b"nbins"),
    ("nbins = 257", dict(nbins=257), b"nbins"),
    ("a NULL label map", dict(lbl=None), b"label map is NULL"),
    ("NULL counts", dict(counts=None), b"counts is NULL"),
    ("misaligned counts", dict(counts=A[1] + 4), b"8-byte aligned"),
]
EMA_DEFECTS = [
    ("K = 0", dict(K=0), b"K must be"),
    ("K = 257", dict(K=257), b"K must be"),
    ("no running matrix", dict(cm_running=None), b"are required"),
    ("no previous matrix", dict(cm_prev=None), b"are required"),
    ("no averages", dict(iou_values=None), b"are required"),
    ("the same matrix twice", dict(cm_prev=A[0]), b"must not be the running matrix"),
    ("misaligned averages", dict(iou_values=A[2] + 2), b"4-byte aligned"),
    ("a misaligned batch vector", dict(iou_batch=A[3] + 1), b"4-byte aligned"),
]


@pytest.mark.parametrize("what,fields,message", CENSUS_DEFECTS, ids=[c[0] for c in CENSUS_DEFECTS])
def test_label_census_rejects_one_defect(what, fields, message):
    from miccai2021_cataract_semantic_segmentation_amd import _lib
    rc = _lib.lib.catseg_label_census_u8(*_census_args(**fields))
    err = _lib.lib.catseg_last_error()
    assert rc == EINVAL and err.startswith(b"catseg_label_census_u8: ") and message in err, (what, rc, err)


@pytest.mark.parametrize("what,fields,message", EMA_DEFECTS, ids=[c[0] for c in EMA_DEFECTS])
def test_iou_ema_rejects_one_defect(what, fields, message):
    from miccai2021_cataract_semantic_segmentation_amd import _lib
    rc = _lib.lib.catseg_iou_ema(*_ema_args(**fields))
    err = _lib.lib.catseg_last_error()
    assert rc == EINVAL and err.startswith(b"catseg_iou_ema: ") and message in err, (what, rc, err)


# ---- configuration
def test_data_defaults_carry_the_reference_keys():
    from miccai2021_cataract_semantic_segmentation_amd.managers.base import DATA_DEFAULTS, merge_defaults
    want = {"weighted_random": [0, 0], "weighted_random_mode": "v1", "oversampling": [0, 0], "oversampling_frac": 0.2,
            "oversampling_preset": "default", "adaptive_batching": [0, 0], "adaptive_sel_size": 10, "adaptive_iou_update": 1,
            "repeat_factor": [0, 0], "repeat_factor_freq_thresh": 0.2, "label_table": None, "adaptive_iou_lag": 0}
    for k, v in want.items():
        assert DATA_DEFAULTS[k] == v, k
    a = merge_defaults({"loss": {}, "data": {"oversampling": [1]}})
    b = merge_defaults({"loss": {}})
    a["data"]["oversampling"].append(9)
    b["data"]["adaptive_batching"].append(9)
    assert DATA_DEFAULTS["oversampling"] == [0, 0] and DATA_DEFAULTS["adaptive_batching"] == [0, 0]      # the defaults' lists are not shared
