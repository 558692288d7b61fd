"""The running weight average on whole networks (optim.WeightAverage, FusedOptimizer.attach_average, graph.py, the managers'
config['train']['ema']): eager steps against stock torch.optim.swa_utils.AveragedModel in fp64 with its fp32 run as the yardstick, hipGraph
replays against eager steps bit for bit, applied() against a model loaded from the average, and the managers' checkpoints.

Run with -s to collect the RATIO lines."""
import os
import sys

import numpy as np
import pytest
import torch
from torch.optim.swa_utils import AveragedModel, get_ema_multi_avg_fn

pytestmark = pytest.mark.gpu
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

f32 = lambda x: float(np.float32(x))
# The C ABI takes float: the decay is given so that 1 - decay IS the float32 value the kernel sees (1 - (1 - float32(0.1)) is exact in
# double), on both sides.
DECAY = 1.0 - f32(0.1)
ENCDEC = {"encoder": {"model": "ResNet18", "pretrained": False}, "decoder": {"model": "UPerNet"}}


def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")


def _bn_net(seed=3):
    """EncDec(ResNet18 + UPerNet) in training mode at 2 x 3 x 64 x 64: (model, three batches, loss over the model's output)"""
    from miccai2021_cataract_semantic_segmentation_amd.losses import LossWrapper
    from miccai2021_cataract_semantic_segmentation_amd.managers import SyntheticCataractDataset
    from miccai2021_cataract_semantic_segmentation_amd.models import EncDec
    torch.manual_seed(seed)
    model = EncDec(ENCDEC, 1).cuda().train()
    ds = SyntheticCataractDataset(2, 64, 64, model.num_classes, seed=seed)
    img = torch.stack([ds[i][0] for i in range(2)]).cuda()
    lbl = torch.stack([ds[i][1] for i in range(2)]).cuda()
    crit = LossWrapper({"losses": {"LovaszSoftmax": 1}, "experiment": 1, "device": "cuda"})
    batches = [(img, lbl), (img.flip(0).contiguous(), lbl.flip(0).contiguous()), ((img * 0.5).contiguous(), lbl)]
    return model, batches, lambda out, l: crit(out[0], out[1], l)


def _snapshot(model):
    return {k: v.detach().clone() for k, v in model.state_dict().items()}


def _step(model, opt, loss_fn, xb, lb):
    opt.zero_grad()
    loss = loss_fn(model(xb), lb)
    loss.backward()
    opt.step()
    return float(loss.detach())


class _Holder(torch.nn.Module):
    """a state dict as a module on the CPU (what AveragedModel averages: its parameters, and with use_buffers its buffers)"""

    def __init__(self, sd, param_names, dtype):
        super().__init__()
        self.names = {k: k.replace(".", "__") for k in sd}
        for k, v in sd.items():
            v = v.detach().cpu()
            v = v.to(dtype) if v.is_floating_point() else v.clone()
            if k in param_names:
                self.register_parameter(self.names[k], torch.nn.Parameter(v))
            else:
                self.register_buffer(self.names[k], v)

    def load(self, sd):
        with torch.no_grad():
            for k, v in sd.items():
                getattr(self, self.names[k]).copy_(v.detach().cpu())

    def get(self, k):
        return getattr(self, self.names[k]).detach()


@pytest.mark.parametrize("mode", ["ema", "swa"])
def test_eager_steps_against_stock_averaged_model(mode):
    """five FusedAdam steps with the average attached; the live state after every step feeds AveragedModel(use_buffers=True) on the CPU"""
    _need_gpu()
    from _yardstick import within
    from miccai2021_cataract_semantic_segmentation_amd.optim import FusedAdam, WeightAverage
    model, batches, loss_fn = _bn_net()
    opt = FusedAdam(model, lr=f32(1e-3))
    avg = opt.attach_average(WeightAverage(model, decay=DECAY, mode=mode, buffers=True))
    assert avg.buffers()[0].numel() == model.flat().flat.numel() and len(avg.buffers()) == 2 and not bool(avg.buffers()[0].any())
    params = {k for k, _ in model.named_parameters()}
    sd0 = _snapshot(model)
    stats = [k for k in sd0 if k.endswith(("running_mean", "running_var"))]
    assert len(stats) >= 20 and avg.buffers()[1].numel() == sum(sd0[k].numel() for k in stats)
    holders, stocks = {}, {}
    for dt in (torch.float64, torch.float32):
        holders[dt] = _Holder(sd0, params, dt)
        kw = dict(multi_avg_fn=get_ema_multi_avg_fn(DECAY)) if mode == "ema" else {}
        stocks[dt] = AveragedModel(holders[dt], use_buffers=True, **kw)
    for step in range(5):
        _step(model, opt, loss_fn, *batches[step % 3])
        sd = _snapshot(model)
        for dt in holders:
            holders[dt].load(sd)
            stocks[dt].update_parameters(holders[dt])
        assert avg.n_averaged == step + 1 == int(stocks[torch.float64].n_averaged)
        if step not in (0, 4):
            continue
        got = avg.state_dict()
        rec = got.pop(WeightAverage.META)
        assert rec["n_averaged"] == step + 1 and rec["mode"] == mode and list(got) == list(sd)
        for k in sd:
            if k.endswith("num_batches_tracked"):
                assert torch.equal(got[k], sd[k]) and int(sd[k]) == step + 1
        if step == 0:       # the first update is the copy
            assert all(torch.equal(got[k], sd[k]) for k in sd)
            continue
        cat = lambda src, keys: torch.cat([src(k).flatten().cpu() for k in keys])
        for what, keys in (("parameters", sorted(params)), ("statistics", stats)):
            within("WeightAverage", "%s step%d %s" % (mode, step + 1, what), cat(lambda k: got[k], keys),
                   cat(stocks[torch.float64].module.get, keys), cat(stocks[torch.float32].module.get, keys))
    fp = model.flat()
    pad = torch.ones(fp.flat.numel(), dtype=torch.bool, device=fp.flat.device)
    for p in fp.params:
        pad[fp.offsets[id(p)]:fp.offsets[id(p)] + p.numel()] = False
    assert not bool(avg.shadow[pad].any()), "a padding element of the shadow moved"


@pytest.mark.parametrize("which", ["adam", "sgd"])
def test_graph_replay_equals_eager_steps(which):
    """three GraphedTrainStep replays == three eager steps bit for bit: parameters, module buffers, both shadows, n_averaged.  adam: the
    catseg_adam_step_dev path; sgd: momentum.  start_step = 1: a weight frozen into the graph would show (1, 1, 1 - decay)."""
    _need_gpu()
    from miccai2021_cataract_semantic_segmentation_amd.graph import GraphedTrainStep
    from miccai2021_cataract_semantic_segmentation_amd.optim import FusedAdam, FusedSGD, WeightAverage
    model, batches, loss_fn = _bn_net(5)
    fp = model.flat()
    w0, b0 = fp.flat.clone(), [b.clone() for b in model.buffers()]
    from miccai2021_cataract_semantic_segmentation_amd import engine

    def make():
        opt = FusedAdam(model, lr=f32(1e-3)) if which == "adam" else FusedSGD(model, lr=f32(1e-2), momentum=f32(0.9))
        return opt, opt.attach_average(WeightAverage(model, decay=DECAY, start_step=1))

    def run(step_fn, opt, avg):
        losses = [step_fn(xb, lb) for xb, lb in batches]
        torch.cuda.synchronize()
        engine.flush_bn_counters(model)
        return (losses, fp.flat.clone(), [b.clone() for b in model.buffers()], [b.clone() for b in avg.buffers()], avg.n_averaged, opt._steps,
                [b.clone() for b in opt.state_buffers()])

    opt, avg = make()
    e = run(lambda xb, lb: _step(model, opt, loss_fn, xb, lb), opt, avg)
    assert e[4] == 2 and e[5] == 3 and len(e[3]) == 2 and not torch.equal(e[1], w0)
    assert not torch.equal(e[3][0], e[1]), "the shadow is the live buffer: nothing was averaged"
    assert len(e[6]) == (4 if which == "adam" else 3) and all(torch.equal(a, b) for a, b in zip(e[6][-2:], e[3]))
    with torch.no_grad():
        fp.flat.copy_(w0)
        for b, s in zip(model.buffers(), b0):
            b.copy_(s)
    opt2, avg2 = make()
    graphed = GraphedTrainStep(model, loss_fn, opt2, *batches[0])
    torch.cuda.synchronize()
    assert avg2.steps == 0 and not any(bool(b.any()) for b in avg2.buffers()), "the warm-up left a trace in the shadows"
    assert torch.equal(fp.flat, w0)
    g = run(lambda xb, lb: float(graphed(xb, lb)), opt2, avg2)
    graphed.release()
    assert g[0] == e[0] and g[4] == e[4] and g[5] == e[5]
    assert torch.equal(g[1], e[1]), "parameters differ in %d elements" % int((g[1] != e[1]).sum())
    assert all(torch.equal(a, b) for a, b in zip(g[2], e[2])), "module buffers differ"
    for name, a, b in zip(("parameter shadow", "statistics shadow"), g[3], e[3]):
        assert torch.equal(a, b), "%s differs in %d elements" % (name, int((a != b).sum()))


def test_applied_swaps_in_place_and_back():
    _need_gpu()
    from miccai2021_cataract_semantic_segmentation_amd.models import EncDec
    from miccai2021_cataract_semantic_segmentation_amd.optim import FusedAdam, WeightAverage
    model, batches, loss_fn = _bn_net(7)
    opt = FusedAdam(model, lr=f32(1e-2))
    avg = opt.attach_average(WeightAverage(model, decay=DECAY))
    with pytest.raises(RuntimeError, match="no weights yet"):
        with avg.applied():
            pass
    for i in range(3):
        _step(model, opt, loss_fn, *batches[i])
    fp = model.flat()
    x = batches[0][0]
    sd = avg.state_dict()           # (like the model's own state_dict(), it flushes the pending num_batches_tracked counts first)
    sd.pop(WeightAverage.META)
    live_w, live_b, ptr0 = fp.flat.clone(), [b.clone() for b in model.buffers()], fp.flat.data_ptr()
    shadows = [b.clone() for b in avg.buffers()]
    fresh = EncDec(ENCDEC, 1)
    fresh.load_state_dict(sd)
    fresh.cuda().eval()
    model.eval()
    with torch.no_grad():
        want = [o.clone() for o in fresh(x)]
        live_out = [o.clone() for o in model(x)]
        with avg.applied():
            assert fp.flat.data_ptr() == ptr0 and torch.equal(fp.flat, shadows[0]) and torch.equal(avg.shadow, live_w)
            got = [o.clone() for o in model(x)]
            inside = avg.state_dict()
            with pytest.raises(RuntimeError, match="re-entrant"):
                with avg.applied():
                    pass
    assert all(torch.equal(a, b) for a, b in zip(got, want)), "the forward inside applied() is not that of a model loaded from the average"
    assert not all(torch.equal(a, b) for a, b in zip(got, live_out))
    assert all(torch.equal(inside[k], sd[k]) for k in sd), "state_dict() inside applied() is not the average"
    torch.cuda.synchronize()
    assert torch.equal(fp.flat, live_w) and all(torch.equal(a, b) for a, b in zip(model.buffers(), live_b)), "the swap back is not exact"
    assert all(torch.equal(a, b) for a, b in zip(avg.buffers(), shadows))
    # an exception inside the block still swaps back
    with pytest.raises(KeyError):
        with avg.applied():
            raise KeyError("x")
    assert torch.equal(fp.flat, live_w) and all(torch.equal(a, b) for a, b in zip(avg.buffers(), shadows)) and not avg._swapped
    # a stream capture is refused (nothing is recorded: the capture stays empty)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.stream(side):
        graph.capture_begin()
        try:
            with pytest.raises(RuntimeError, match="stream capture"):
                with avg.applied():
                    pass
        finally:
            graph.capture_end()
    torch.cuda.current_stream().wait_stream(side)
    # a recorded pass that awaits its backward is refused
    model.train()
    opt.zero_grad()
    model._keep_pass = True
    try:
        pending = loss_fn(model(x), batches[0][1])
        with pytest.raises(RuntimeError, match="awaits its backward"):
            with avg.applied():
                pass
    finally:
        model._keep_pass = False
    pending.backward()
    model._last_pass = model._last_outputs = None
    opt.step()
    torch.cuda.synchronize()
    from miccai2021_cataract_semantic_segmentation_amd import engine
    engine.flush_bn_counters(model)
    after_swap = [fp.flat.clone()] + [b.clone() for b in model.buffers()] + [b.clone() for b in avg.buffers()]
    # the same fourth step in a run that never swapped
    model2, batches2, loss_fn2 = _bn_net(7)
    opt2 = FusedAdam(model2, lr=f32(1e-2))
    avg2 = opt2.attach_average(WeightAverage(model2, decay=DECAY))
    for i in range(3):
        _step(model2, opt2, loss_fn2, *batches2[i])
    _step(model2, opt2, loss_fn2, *batches2[0])
    torch.cuda.synchronize()
    engine.flush_bn_counters(model2)
    never = [model2.flat().flat.clone()] + [b.clone() for b in model2.buffers()] + [b.clone() for b in avg2.buffers()]
    assert len(never) == len(after_swap) and all(torch.equal(a, b) for a, b in zip(after_swap, never)), "the step after a swap differs"


# ---------------------------------------------------------------------------------------------------------------- managers
def _fcn_cfg(tmp_path, epochs, **train):
    return {"name": "fcn", "mode": "training", "manager": "FCN", "log_path": str(tmp_path), "graph": {"model": "FCN", "width": 0.25},
            "data": {"experiment": 2, "batch_size": 2}, "loss": {"name": "LovaszSoftmax"},
            "train": dict({"learning_rate": 1e-3, "epochs": epochs}, **train), "log_every_n_epochs": 1, "seed": 0}


def _sets():
    from miccai2021_cataract_semantic_segmentation_amd import managers
    tr = managers.SyntheticCataractDataset(6, 64, 96, 17, seed=1)
    va = managers.SyntheticCataractDataset(2, 64, 96, 17, seed=2)
    return tr, va, torch.utils.data.SequentialSampler(tr)        # (a fixed frame order: runs are compared bit for bit)


def _seeded(cls, *args):
    """(the managers seed torch after the model is built, as the reference does: runs that are compared start from one generator state)"""
    torch.manual_seed(11)
    return cls(*args)


def _last(m, epoch):
    return torch.load(str(m.log_dir / "chkpts" / "chkpt_epoch_{:03d}.pt".format(epoch)), weights_only=False)


@pytest.mark.parametrize("optimiser", [None, {"name": "SGD", "momentum": 0.9}], ids=["adam", "sgd"])
def test_manager_eager_graph_and_resume(tmp_path, optimiser):
    """two epochs with train.ema, eager and as a hipGraph, write bit-identical ema_state_dicts under the model's keys; a run checkpointed
    after its first epoch and resumed ends with the shadows of the uninterrupted run"""
    _need_gpu()
    from miccai2021_cataract_semantic_segmentation_amd import managers
    tr, va, order = _sets()
    ema = {"decay": DECAY, "start_step": 1, "validate": "both"}
    extra = {} if optimiser is None else {"optimiser": optimiser}
    runs = {}
    for name, kw in (("eager", {}), ("graph", {"hip_graph": True})):
        m = _seeded(managers.FCNManager, _fcn_cfg(tmp_path / name, 2, ema=ema, **dict(extra, **kw)), tr, va, order)
        assert m.average is not None and m.optimiser._avg is m.average
        m.train()
        assert m.average.steps == 6 and m.average.n_averaged == 5
        runs[name] = (m, _last(m, 1))
    ck = runs["eager"][1]
    assert set(ck["ema_state_dict"]) == set(ck["model_state_dict"]) and list(ck["ema_state_dict"]) == list(ck["model_state_dict"])
    assert ck["ema"]["n_averaged"] == 5 and ck["ema"]["mode"] == "ema" and ck["ema"]["start_step"] == 1 and ck["ema"]["decay"] == DECAY
    assert not all(torch.equal(ck["ema_state_dict"][k], ck["model_state_dict"][k]) for k in ck["model_state_dict"])
    for k, v in ck["ema_state_dict"].items():
        assert torch.equal(v, runs["graph"][1]["ema_state_dict"][k]), "eager and graph runs differ in %s" % k
        assert torch.equal(ck["model_state_dict"][k], runs["graph"][1]["model_state_dict"][k])
    h = runs["eager"][0].history
    assert all({"valid_miou", "valid_loss", "valid_miou_live", "valid_loss_live"} <= set(r) for r in h)
    # ---- one epoch, checkpoint, resume for one more
    first = _seeded(managers.FCNManager, _fcn_cfg(tmp_path / "first", 1, ema=ema, **extra), tr, va, order)
    first.train()
    second = _seeded(managers.FCNManager, _fcn_cfg(tmp_path / "second", 1, ema=ema, **extra), tr, va, order)
    second.log_dir = first.log_dir
    second.load_checkpoint("last")
    assert second.average.steps == 3 and second.average.n_averaged == 2
    if optimiser is not None:
        assert second.optimiser._steps == 1          # (SGD's format has no step count: the average's count continues all the same)
    second.train()
    resumed = _last(second, 0)
    assert second.average.n_averaged == 5 and resumed["ema"]["n_averaged"] == 5
    for k, v in ck["ema_state_dict"].items():
        assert torch.equal(v, resumed["ema_state_dict"][k]), "the resumed run differs in %s" % k


def test_manager_validates_infers_and_labels_with_the_average(tmp_path):
    """EncDec (BatchNorm): validate() scores the averaged weights and statistics, an inference manager's infer() reproduces that mIoU from
    ema_state_dict, pseudo_label(weights='ema') labels with them; without the key the checkpoint is what it was"""
    _need_gpu()
    from miccai2021_cataract_semantic_segmentation_amd import managers
    from miccai2021_cataract_semantic_segmentation_amd.utils.metrics import t_get_confusion_matrix, t_get_mean_iou
    tr, va, order = _sets()
    cfg = {"name": "upn", "manager": "EncDec", "encoder": ENCDEC["encoder"], "decoder": ENCDEC["decoder"], "loss": {"losses": {"LovaszSoftmax": 1}},
           "data": {"experiment": 2, "batch_size": 2}, "train": {"learning_rate": 1e-3, "epochs": 2, "ema": {"decay": DECAY, "validate": "both"}},
           "log_every_n_epochs": 1, "gpu_device": 0, "log_path": str(tmp_path)}
    m = managers.EncDecManager(cfg, tr, va, order)
    m.train()
    h = m.history[-1]
    assert {"valid_miou", "valid_miou_live", "valid_loss_live"} <= set(h)
    ck = _last(m, 1)
    assert list(ck["ema_state_dict"]) == list(ck["model_state_dict"])
    stats = [k for k in ck["model_state_dict"] if k.endswith("running_var")]
    assert stats and any(not torch.equal(ck["ema_state_dict"][k], ck["model_state_dict"][k]) for k in stats)
    assert all(torch.equal(ck["ema_state_dict"][k], ck["model_state_dict"][k]) for k in ck["model_state_dict"] if k.endswith("num_batches_tracked"))
    # the mIoU of a model loaded from ema_state_dict IS what validate() recorded for the last epoch
    def score(state):
        net = managers.EncDecManager(dict(cfg, mode="inference", load_checkpoint=m.run_id), None, va).model
        net.load_state_dict(state)
        net.eval()
        net.get_features = False
        cm = torch.zeros((net.num_classes,) * 2, dtype=torch.int32, device="cuda")
        with torch.no_grad():
            for i in range(len(va)):
                t_get_confusion_matrix(net(va[i][0][None].cuda().float()), va[i][1][None].cuda(), cm)
        return round(float(t_get_mean_iou(cm, 2)), 4)
    assert score(ck["ema_state_dict"]) == h["valid_miou"] and score(ck["model_state_dict"]) == h["valid_miou_live"]
    # inference mode: the 'best' checkpoint's averaged weights (the key's infer, default true); "infer": false scores the live ones
    best = torch.load(str(m.log_dir / "chkpts" / "chkpt_best.pt"), weights_only=False)
    assert "ema_state_dict" in best
    inf = managers.EncDecManager(dict(cfg, mode="inference", load_checkpoint=m.run_id), None, va)
    assert round(inf.infer()[0], 4) == m.metrics["best_miou"] == score(best["ema_state_dict"])
    assert all(torch.equal(v, best["ema_state_dict"][k].cuda()) for k, v in inf.model.state_dict().items())
    live_cfg = dict(cfg, mode="inference", load_checkpoint=m.run_id, train=dict(cfg["train"], ema={"infer": False}))
    inf_live = managers.EncDecManager(live_cfg, None, va)
    inf_live.infer()
    assert all(torch.equal(v, best["model_state_dict"][k].cuda()) for k, v in inf_live.model.state_dict().items())
    # pseudo labels of the teacher: byte for byte those of a model that holds ema_state_dict
    frames = [va[i] for i in range(2)]
    maps, want = {}, {}
    m.model.train()              # (between two steps of a mean-teacher loop)
    was = [b.clone() for b in [m.model.flat().flat] + list(m.model.buffers())]
    assert m.pseudo_label(frames, lambda i, lab: maps.__setitem__(i, lab), weights="ema") == 2
    assert all(torch.equal(a, b) for a, b in zip(was, [m.model.flat().flat] + list(m.model.buffers()))) and m.model.training
    teacher = managers.EncDecManager(dict(cfg, mode="inference", load_checkpoint=m.run_id), None, va)
    teacher.load_inference_weights = lambda: teacher.model.load_state_dict(ck["ema_state_dict"])
    assert teacher.pseudo_label(frames, lambda i, lab: want.__setitem__(i, lab)) == 2
    assert sorted(maps) == [0, 1] and all(maps[i].dtype == np.uint8 and maps[i].tobytes() == want[i].tobytes() for i in maps)
    with pytest.raises(ValueError, match="weights='ema'"):
        teacher.pseudo_label(frames, lambda i, lab: None, weights="ema")
    # ---- without the key: nothing attached, the checkpoint's keys of old
    plain = managers.EncDecManager(dict(cfg, train={"learning_rate": 1e-3, "epochs": 1}, log_path=str(tmp_path / "plain")), tr, va, order)
    assert plain.average is None and plain.optimiser._avg is None
    plain.train()
    assert set(_last(plain, 0)) == {"global_step", "epoch", "model_state_dict", "optimiser_state_dict", "best_loss", "best_miou", "is_best",
                                    "scheduler_state_dict"}
    assert len(plain.optimiser.state_buffers()) == 2
    with pytest.raises(ValueError, match="unknown key"):
        managers.EncDecManager(dict(cfg, train=dict(cfg["train"], ema={"momentum": 0.9})), tr, va, order)
