"""Host side of the running weight average (optim.WeightAverage, include/catseg_ema.h): the schedule of weights pinned to stock
torch.optim.swa_utils.AveragedModel in fp64, every refusal of the three entry points before a launch, the prototypes against
_lib._SIGS, and config['train']['ema']."""
import os

import numpy as np
import pytest
import torch
from torch.optim.swa_utils import AveragedModel, get_ema_multi_avg_fn

import _abi

STEPS, START = 12, 3


class _Tiny(torch.nn.Module):
    def __init__(self):
        super().__init__()
        self.conv = torch.nn.Conv2d(2, 3, 3)
        self.bn = torch.nn.BatchNorm2d(3)


def _parameter_sets():
    """12 synthetic states of the tiny module (every floating-point tensor of its state dict), fp64"""
    gen = torch.Generator().manual_seed(5)
    m = _Tiny().double()
    keys = [k for k, v in m.state_dict().items() if v.is_floating_point()]
    sets = []
    for step in range(STEPS):
        sets.append({k: torch.randn(m.state_dict()[k].shape, generator=gen, dtype=torch.float64) * (1.0 + 0.1 * step) for k in keys})
    return m, keys, sets


def _replay(sets, keys, mode, decay, warmup, start_step):
    """numpy fp64: the schedule of optim.average_weight and the two-sided lerp of catseg_ema.h, from a zero shadow"""
    from miccai2021_cataract_semantic_segmentation_amd.optim import average_weight
    avg = {k: np.zeros(tuple(sets[0][k].shape)) for k in keys}
    weights = []
    for step, s in enumerate(sets, start=1):
        w = average_weight(max(0, step - 1 - start_step), mode, decay, warmup)
        weights.append(w)
        for k in keys:
            p, a = s[k].numpy(), avg[k]
            avg[k] = a + w * (p - a) if w < 0.5 else p - (p - a) * (1.0 - w)
    return avg, weights


@pytest.mark.parametrize("case", ["ema", "swa", "ema-warmup"])
def test_schedule_against_stock_averaged_model(case):
    """the floating-point tensors after 12 updates, start_step = 3: the stock model sees the states behind the tracking phase only (its
    first update is a copy, as the tracking phase's last is here).  num_batches_tracked is left out: stock torch averages the integer
    with a truncating cast, which is deliberately not reproduced."""
    m, keys, sets = _parameter_sets()
    decay = 0.9
    if case == "ema":
        stock = AveragedModel(m, multi_avg_fn=get_ema_multi_avg_fn(decay), use_buffers=True)
    elif case == "swa":
        stock = AveragedModel(m, use_buffers=True)
    else:
        def avg_fn(averaged, current, num_averaged):
            d = min(decay, (1.0 + float(num_averaged)) / (10.0 + float(num_averaged)))
            return d * averaged + (1.0 - d) * current
        stock = AveragedModel(m, avg_fn=avg_fn, use_buffers=True)
    for s in sets[START:]:
        m.load_state_dict(s, strict=False)
        stock.update_parameters(m)
    assert int(stock.n_averaged) == STEPS - START
    got, weights = _replay(sets, keys, "swa" if case == "swa" else "ema", decay, case == "ema-warmup", START)
    assert weights[:START + 1] == [1.0] * (START + 1) and all(0 < w < 1 for w in weights[START + 1:])
    if case == "swa":
        assert weights[START + 1:] == [1.0 / (n + 1) for n in range(1, STEPS - START)]
    want = stock.module.state_dict()
    for k in keys:
        ref = want[k].numpy()
        err = np.abs(got[k] - ref).max() / np.abs(ref).max()
        assert err <= 1e-12, (case, k, err)
    # the tracking phase: with every step up to start_step the shadow IS the live state
    tracked, _ = _replay(sets[:START], keys, "ema", decay, False, START)
    for k in keys:
        assert np.array_equal(tracked[k], sets[START - 1][k].numpy())


def test_average_weight_table():
    from miccai2021_cataract_semantic_segmentation_amd.optim import average_weight
    assert average_weight(0, "ema", 0.999) == 1.0 and average_weight(0, "swa") == 1.0
    assert average_weight(5, "ema", 0.75) == 0.25
    assert average_weight(1, "ema", 0.999, warmup=True) == 1.0 - 2.0 / 11.0
    assert average_weight(100000, "ema", 0.999, warmup=True) == 1.0 - 0.999
    assert average_weight(3, "swa") == 0.25
    for bad in ((-1, "ema"), (1, "mean")):
        with pytest.raises(ValueError, match="average_weight"):
            average_weight(*bad)


def test_refusals_before_any_launch():
    """every CATSEG_EINVAL case of the three entry points, with fake aligned device pointers: nothing is launched"""
    from miccai2021_cataract_semantic_segmentation_amd import _lib
    lib = _lib.lib
    A = [0x10000 * (i + 1) for i in range(4)]
    nan = float("nan")
    upd = lambda **k: lib.catseg_ema_update(*[dict(dict(p=A[0], avg=A[1], n=1000, w=0.5, wd=None, st=None), **k)[q] for q in ("p", "avg", "n", "w", "wd", "st")])
    swap = lambda **k: lib.catseg_ema_swap(*[dict(dict(a=A[0], b=A[1], n=1000, st=None), **k)[q] for q in ("a", "b", "n", "st")])
    tab = lambda **k: lib.catseg_ema_table(*[dict(dict(t=A[0], c=3, sh=A[1], mode=0, w=0.5, wd=None, st=None), **k)[q]
                                            for q in ("t", "c", "sh", "mode", "w", "wd", "st")])
    cases = [(upd, dict(n=0), b"positive"), (upd, dict(n=-4), b"positive"), (upd, dict(p=None), b"required"), (upd, dict(avg=None), b"required"),
             (upd, dict(p=A[0] + 4), b"16-byte"), (upd, dict(avg=A[1] + 8), b"16-byte"), (upd, dict(w=-0.01), b"[0, 1]"),
             (upd, dict(w=1.5), b"[0, 1]"), (upd, dict(w=nan), b"[0, 1]"), (upd, dict(wd=A[2] + 2), b"4-byte"),
             (swap, dict(n=0), b"positive"), (swap, dict(a=None), b"required"), (swap, dict(b=None), b"required"),
             (swap, dict(a=A[0] + 4), b"16-byte"), (swap, dict(b=A[1] + 12), b"16-byte"),
             (tab, dict(c=0), b"count"), (tab, dict(c=-1), b"count"), (tab, dict(t=None), b"table"), (tab, dict(t=A[0] + 4), b"table"),
             (tab, dict(sh=None), b"shadow"), (tab, dict(sh=A[1] + 2), b"shadow"), (tab, dict(mode=2), b"unknown mode"),
             (tab, dict(mode=-1), b"unknown mode"), (tab, dict(w=1.25), b"[0, 1]"), (tab, dict(w=nan), b"[0, 1]"), (tab, dict(w=-1.0), b"[0, 1]"),
             (tab, dict(wd=A[2] + 1), b"4-byte")]
    names = {upd: b"catseg_ema_update:", swap: b"catseg_ema_swap:", tab: b"catseg_ema_table:"}
    for fn, kw, msg in cases:
        rc = fn(**kw)
        err = lib.catseg_last_error()
        assert rc == 1 and msg in err and err.startswith(names[fn]), (kw, rc, err)
    assert lib.catseg_ema_grid_cap() >= 1


def test_signature_table_matches_the_extension_header():
    """include/catseg_ema.h declares the four averaging entry points; each has the header's signature in _lib._SIGS and is exported; the
    entry record's numpy mirror has the header's size"""
    from miccai2021_cataract_semantic_segmentation_amd import _lib, ops
    assert "#define CATSEG_EMA_ENTRY_BYTES %d" % np.dtype(ops.EMA_ENTRY).itemsize in open(os.path.join(_abi.INCLUDE, "catseg_ema.h")).read()
    protos = _abi.prototypes("catseg_ema.h")
    assert sorted(protos) == ["catseg_ema_grid_cap", "catseg_ema_swap", "catseg_ema_table", "catseg_ema_update"]
    for name, (res, args, _) in protos.items():
        assert _lib._SIGS[name] == (res, args), "%s: header %r, table %r" % (name, (res, args), _lib._SIGS[name])
        assert hasattr(_lib.lib, name)
    assert (ops.EMA_LERP, ops.EMA_SWAP) == (0, 1)


def test_config_key():
    """unknown and ill-typed entries are refused; the defaults; without the key nothing is built or attached"""
    from miccai2021_cataract_semantic_segmentation_amd.optim import (FusedAdam, FusedSGD, WeightAverage, average_config, build_average)
    assert average_config(None) is None
    assert average_config({}) == {"decay": 0.999, "mode": "ema", "warmup": False, "start_step": 0, "buffers": True, "validate": "ema", "infer": True}
    assert average_config({"mode": "swa", "validate": "both", "start_step": 7})["start_step"] == 7
    for bad, msg in (({"decai": 0.9}, "unknown key"), ({"update_every": 2}, "unknown key"), ({"decay": 1.0}, "decay"), ({"decay": "0.9"}, "decay"),
                     ({"decay": True}, "decay"), ({"decay": -0.1}, "decay"), ({"mode": "mean"}, "mode"), ({"warmup": 1}, "warmup"),
                     ({"start_step": -1}, "start_step"), ({"start_step": 1.5}, "start_step"), ({"buffers": "yes"}, "buffers"),
                     ({"validate": "all"}, "validate"), ({"infer": 0}, "infer"), ([("decay", 0.9)], "dictionary")):
        with pytest.raises(ValueError, match=msg):
            average_config(bad)
    model = _Tiny()
    opt = FusedAdam(model, lr=1e-3)
    assert build_average(model, opt, None) is None and opt._avg is None
    avg = build_average(model, opt, {"decay": 0.9, "start_step": 2})
    assert isinstance(avg, WeightAverage) and opt._avg is avg and avg.optimiser is opt
    assert (avg.decay, avg.mode, avg.start_step, avg.use_buffers) == (0.9, "ema", 2, True)
    # the count is the optimiser's step count, seen from the attachment: no second counter
    assert (avg.steps, avg.n_averaged, avg.ready) == (0, 0, False)
    opt._steps = 2
    assert (avg.steps, avg.n_averaged, avg.weight()) == (2, 0, 1.0)
    opt._steps = 3
    assert (avg.steps, avg.n_averaged, avg.weight()) == (3, 1, 1.0)        # the first counted update is still the copy
    opt._steps = 4
    assert (avg.n_averaged, avg.weight()) == (2, 1.0 - 0.9)
    sgd = FusedSGD(model, lr=1e-3, momentum=0.9)
    sgd._steps = 5
    late = sgd.attach_average(WeightAverage(model, mode="swa"))
    assert late.steps == 0
    sgd._steps = 8
    assert (late.n_averaged, late.weight()) == (3, 1.0 / 3.0)
    with pytest.raises(ValueError, match="own model"):
        opt.attach_average(WeightAverage(_Tiny()))
    with pytest.raises(TypeError, match="fused optimiser"):
        build_average(model, torch.optim.SGD(model.parameters(), lr=0.1), {})
    for kw in (dict(decay=1.0), dict(mode="x"), dict(start_step=-2)):
        with pytest.raises(ValueError, match="WeightAverage"):
            WeightAverage(model, **kw)
    assert sgd.attach_average(None) is None and sgd._avg is None and late.optimiser is None
