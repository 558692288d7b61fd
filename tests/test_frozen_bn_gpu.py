"""Frozen BatchNorm through whole networks (engine.freeze_bn, conv_bn_act's frozen route, graph.GraphedTrainStep, the managers).

Gradients: tests/_calib.calibrated_grad_check at its defaults, against the CPU oracle with the SAME-NAMED BatchNorm layers evaluated with
training=False (the oracle is functional: its one BatchNorm function is wrapped for the duration of a forward).  Selections: every
BatchNorm, the trunk, and bn1 alone / bn2 alone of the first residual block -- a frozen producer in front of an unfrozen private_in
consumer, and the reverse."""
import contextlib
import json
import os
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

pytestmark = pytest.mark.gpu
T = torch.from_numpy


def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")


@contextlib.contextmanager
def frozen_oracle(names):
    """the oracle's BatchNorm layers named in `names` run with training=False (running statistics, no update, no batch count)"""
    from oracle import hrnet as OH, nets as ON, upernet as OU
    names = set(names)
    plain = ON.bn

    def bn(S, p, x, train, *a, **k):
        return plain(S, p, x, train and p not in names, *a, **k)
    saved = (ON.bn, OU.bn, OH._bn_generic)
    ON.bn = OU.bn = OH._bn_generic = bn
    try:
        yield
    finally:
        ON.bn, OU.bn, OH._bn_generic = saved


def frozen_forward(names, forward):
    def run(S, x):
        with frozen_oracle(names):
            return forward(S, x)
    return run


def running_buffers(model):
    model.state_dict()          # (flushes the lazily counted num_batches_tracked)
    return {k: v.detach().clone() for k, v in model.named_buffers() if "running" in k or "num_batches" in k}


def moved_and_kept(model, before):
    """frozen modules: running_mean, running_var, num_batches_tracked bit-unchanged; unfrozen ones moved"""
    after = running_buffers(model)
    frozen = set(model.frozen_bn)
    assert frozen
    for k, v in after.items():
        if k.rsplit(".", 1)[0] in frozen:
            assert torch.equal(v, before[k]), "a frozen BatchNorm's %s changed" % k
        else:
            assert not torch.equal(v, before[k]), "an unfrozen BatchNorm's %s did not move" % k


# ---- the three networks: (model, spec, seed, oracle forward, oracle loss, HIP loss of the model's outputs, x, lbl)
def _encdec(select):
    from oracle import losses as OL, upernet as OU
    from oracle.state import spec_of
    from miccai2021_cataract_semantic_segmentation_amd.losses import LossWrapper
    from miccai2021_cataract_semantic_segmentation_amd.models import EncDec
    cfg = {"encoder": {"model": "ResNet18", "pretrained": False}, "decoder": {"model": "UPerNet"}}
    if select is not None:
        cfg["freeze_bn"] = select
    model = EncDec(cfg, 2)          # experiment 2: K = 17
    g = torch.Generator().manual_seed(61)
    x = torch.rand(2, 3, 64, 64, generator=g)
    lbl = torch.randint(0, 17, (2, 8, 8), generator=g).repeat_interleave(8, 1).repeat_interleave(8, 2)
    crit = LossWrapper({"losses": {"LovaszSoftmax": 1}, "experiment": 2, "device": "cuda"})
    return dict(model=model, spec=spec_of(model.state_dict()), seed=62, x=x, lbl=lbl, loss=lambda out, l: crit(out[0], out[1], l),
                forward=lambda S, x_: OU.encdec_forward(S, x_, "ResNet18", train=True)[1], oracle_loss=lambda o, l: OL.lovasz_softmax(o, l),
                label="frozen EncDec(ResNet18+UPerNet) %r" % (select,))


P_DROP = 0.25


def _ocrnet_oracle(S, x, mults):
    """oracle.nets.ocrnet_forward with the two Dropout2d layers of the heads as given multiplier tables [B, 512] (models/OCR.py:87, 311-316)"""
    from oracle import nets as ON
    size = x.shape[-2:]
    f = ON.resnet_features(S, x, "resnet50", ON.rswd_for(8), True)
    low, high = f[3], f[4]
    h = F.relu(ON.bn(S, "interm_prediction_head.1", ON.conv(S, "interm_prediction_head.0", low, 1, 1), True))
    interm = ON.conv(S, "interm_prediction_head.4", h * mults[0].to(h.dtype)[:, :, None, None])
    xh = F.relu(ON.bn(S, "conv_high_map.1", ON.conv(S, "conv_high_map.0", high, 1, 1), True))
    proxy = ON.spatial_gather(xh, interm)
    ctx = ON.object_attention(S, "spatial_ocr_head.object_context_block", xh, proxy, True)
    o = torch.cat([ctx, xh], 1)
    o = F.relu(ON.bn(S, "spatial_ocr_head.conv_bn_dropout.1", ON.conv(S, "spatial_ocr_head.conv_bn_dropout.0", o), True))
    logits = ON.conv(S, "conv_out", o * mults[1].to(o.dtype)[:, :, None, None])
    up = F.interpolate(logits, size=size, mode="bilinear", align_corners=True)
    return F.interpolate(interm, size=size, mode="bilinear", align_corners=True), up


def _ocrnet(select, fixed=True):
    import _dropout_ref as R
    from oracle import losses as OL
    from oracle.state import spec_of
    from miccai2021_cataract_semantic_segmentation_amd.engine import dropout_layers
    from miccai2021_cataract_semantic_segmentation_amd.losses import TwoScaleLoss
    from miccai2021_cataract_semantic_segmentation_amd.models import OCRNet
    cfg = {"backbone": "resnet50", "out_stride": 8, "pretrained": False, "dropout": P_DROP}
    if select is not None:
        cfg["freeze_bn"] = select
    model = OCRNet(cfg, 3)
    g = torch.Generator().manual_seed(71)
    x = torch.rand(2, 3, 64, 64, generator=g)
    lbl = torch.randint(0, 26, (2, 8, 8), generator=g).repeat_interleave(8, 1).repeat_interleave(8, 2)
    mults = []
    for d in sorted(dropout_layers(model), key=lambda d: d.layer):
        keep01 = (torch.rand(2, 512, generator=g) >= P_DROP).float()
        if fixed:
            d.fixed_mask = keep01
        mults.append(keep01 * float(R.keep_of(P_DROP)))
    crit = TwoScaleLoss({"experiment": 3, "interm": {"name": "LovaszSoftmax", "args": [], "weight": 0.4},
                         "final": {"name": "LovaszSoftmax", "args": [], "weight": 1.0}})
    return dict(model=model, spec=spec_of(model.state_dict()), seed=72, x=x, lbl=lbl, loss=lambda out, l: crit(out[0], out[1], l),
                forward=lambda S, x_: _ocrnet_oracle(S, x_, mults), oracle_loss=lambda o, l: OL.two_scale_lovasz(o[0], o[1], l),
                label="frozen OCRNet(ResNet50 OS8, dropout) %r" % (select,))


def _hrnet(select, golden):
    from oracle import hrnet as OH, losses as OL
    from miccai2021_cataract_semantic_segmentation_amd.losses import CrossEntropyLoss
    from miccai2021_cataract_semantic_segmentation_amd.models import HRNetv2
    g = golden("hrnetv2_e3_tiny")           # the reduced-width network and the weights of tests/test_hrnet_gpu.py
    model = HRNetv2({} if select is None else {"freeze_bn": select}, 3)
    ce = CrossEntropyLoss(ignore_index=25)
    # NOT that fixture's 2 x 3 x 64 x 96 input: it leaves 12 positions per channel in the fourth branch, where ONE ReLU input within rounding
    # of zero -- the fp64 forward has about a hundred within 1e-5 of their tensor's scale -- moves every gradient upstream of it by 1e-2 in
    # whichever fp32 evaluation rounds it to the other side.  The check is then a draw between the kernels' flips and the three CPU
    # variants' (measured: one selection at max 69.5 with fp32 kernels and 0.17 with bf16x3, forward errors alike; the CPU variants show
    # the same 5e-3 jumps on other selections).  At 2 x 3 x 128 x 192 a position weighs a quarter of that
    gen = torch.Generator().manual_seed(81)
    x = torch.rand(2, 3, 128, 192, generator=gen)
    lbl = torch.randint(0, 26, (2, 16, 24), generator=gen).repeat_interleave(8, 1).repeat_interleave(8, 2)
    return dict(model=model, spec=json.loads(str(g["spec"])), seed=int(g["seed"]), x=x, lbl=lbl, loss=lambda out, l: ce(out, l),
                forward=lambda S, x_: OH.hrnetv2_forward(S, x_, train=True), oracle_loss=lambda o, l: OL.cross_entropy(o, l, 3),
                label="frozen HRNetv2 %r" % (select,))


def _load(net):
    from oracle.state import fill_state
    net["model"].load_state_dict(fill_state(net["spec"], net["seed"]))
    return net["model"].cuda().train()


def _gradient_check(net):
    from _calib import calibrated_grad_check
    model = _load(net)
    assert model.frozen_bn
    before = running_buffers(model)
    out = model(net["x"].cuda())
    net["loss"](out, net["lbl"].cuda()).backward()
    torch.cuda.synchronize()
    frozen = set(model.frozen_bn)           # one forward: the frozen statistics stayed, the others moved
    for k, v in running_buffers(model).items():
        assert torch.equal(v, before[k]) == (k.rsplit(".", 1)[0] in frozen), k
    calibrated_grad_check(model, net["spec"], net["seed"], frozen_forward(model.frozen_bn, net["forward"]), net["oracle_loss"], net["x"], net["lbl"],
                          label=net["label"])


RESNET_SELECTIONS = ["all", "backbone", ["backbone.layer1.0.bn1"], ["backbone.layer1.0.bn2"]]


@pytest.fixture(scope="module", params=range(4), ids=["all", "backbone", "bn1", "bn2"])
def pick(request):
    """module-scoped, so that the two precisions of one selection run back to back and share the CPU evaluations of _calib's cache"""
    return request.param


def test_encdec_resnet18_upernet_gradients(pick, precision):
    _need_gpu()
    select = RESNET_SELECTIONS[pick]
    if isinstance(select, list):
        select = [s.replace("backbone.", "enc_model.") for s in select]      # (EncDec names its trunk enc_model)
    _gradient_check(_encdec(select))


def test_ocrnet_resnet50_dropout_gradients(pick, precision):
    _need_gpu()
    _gradient_check(_ocrnet(RESNET_SELECTIONS[pick]))


def test_hrnetv2_gradients(pick, precision, golden):
    """HRNetv2 has no module named backbone: its trunk selection is the stem and the four stages, its single-layer selections are bn1 of
    the first residual block (a Bottleneck in front of a private_in consumer) and bn2 of the first BasicBlock.

    Measured on an MI355X (fp32 / bf16x3; median, p95, max): all 0.00 0.01 0.01 / 0.02 0.03 0.04; trunk 0.88 1.21 1.95 / 1.81 2.61 6.76;
    bn1 0.34 0.90 0.99 / 0.27 0.84 0.99; bn2 0.27 0.61 1.21 / 0.38 9.13 15.15."""
    _need_gpu()
    select = ["all", ["conv1", "bn1", "conv2", "bn2", "layer1", "transition1", "stage2", "transition2", "stage3", "transition3", "stage4"],
              ["layer1.0.bn1"], ["stage2.0.branches.0.0.bn2"]][pick]
    _gradient_check(_hrnet(select, golden))


# ---- three optimiser steps: statistics, dropout draws, eager against hipGraph replay
def _steps(net, graphed, n=3):
    from miccai2021_cataract_semantic_segmentation_amd.engine import dropout_layers
    from miccai2021_cataract_semantic_segmentation_amd.graph import GraphedTrainStep
    from miccai2021_cataract_semantic_segmentation_amd.optim import FusedAdam
    model = _load(net)
    for d in dropout_layers(model):
        d.reseed(4321)
    opt = FusedAdam(model, lr=1e-3)
    g = torch.Generator().manual_seed(5)
    batches = [(torch.rand(net["x"].shape, generator=g).cuda(), net["lbl"].roll(i, 1).cuda()) for i in range(n)]
    before = running_buffers(model)
    losses = []
    if graphed:
        step = GraphedTrainStep(model, lambda o, l: net["loss"](o, l), opt, *batches[0])
        for x, l in batches:
            losses.append(float(step(x, l)))
        step.release()
    else:
        for x, l in batches:
            opt.zero_grad()
            loss = net["loss"](model(x), l)
            loss.backward()
            opt.step()
            losses.append(float(loss.detach()))
    torch.cuda.synchronize()
    return model, before, losses


@pytest.mark.parametrize("build,select", [(_ocrnet, "backbone"), (_encdec, "all"), (_ocrnet, ["backbone.layer1.0.bn2"])], ids=["ocrnet-backbone", "encdec-all", "ocrnet-bn2"])
def test_three_steps_eager_and_graph_replay(build, select):
    """frozen statistics stay bit for bit while unfrozen ones move; Dropout2d behind a frozen BatchNorm draws once per forward; three eager
    steps and three hipGraph replays agree bit for bit in parameters, buffers and losses"""
    _need_gpu()
    from miccai2021_cataract_semantic_segmentation_amd.engine import dropout_layers
    kw = {"fixed": False} if build is _ocrnet else {}
    eager, before, losses_e = _steps(build(select, **kw), False)
    if select != "all":
        moved_and_kept(eager, before)
    frozen = set(eager.frozen_bn)
    assert all(torch.equal(v, before[k]) for k, v in running_buffers(eager).items() if k.rsplit(".", 1)[0] in frozen)
    assert [int(d.state[3]) for d in dropout_layers(eager)] == [3] * len(dropout_layers(eager))
    graph, _, losses_g = _steps(build(select, **kw), True)
    assert [int(d.state[3]) for d in dropout_layers(graph)] == [3] * len(dropout_layers(graph))
    assert losses_e == losses_g and all(np.isfinite(losses_e))
    assert torch.equal(eager.flat().flat, graph.flat().flat)
    be, bg = running_buffers(eager), running_buffers(graph)
    assert list(be) == list(bg) and all(torch.equal(be[k], bg[k]) for k in be)


# ---- nothing frozen: the launches and the bits of before the attribute existed
def test_nothing_frozen_launches_and_computes_what_it_did(monkeypatch):
    _need_gpu()
    from miccai2021_cataract_semantic_segmentation_amd import engine, ops
    from _route_trace import diff

    def step():
        net = _ocrnet(None, fixed=True)
        model = _load(net)
        assert model.frozen_bn == []
        ops.PROFILE = []
        try:
            out = model(net["x"].cuda())
            net["loss"](out, net["lbl"].cuda()).backward()
            torch.cuda.synchronize()
            trace = [(p[0], p[1]) for p in ops.PROFILE]
        finally:
            ops.PROFILE = None
        return trace, [o.detach().clone() for o in out], model.flat().grad.clone(), running_buffers(model)
    with_attr = step()
    monkeypatch.delattr(engine.BatchNorm2d, "frozen")
    assert not hasattr(engine.BatchNorm2d(4), "frozen")
    without = step()
    assert len(with_attr[0]) > 100 and diff(with_attr[0], without[0]) is None
    assert all(torch.equal(a, b) for a, b in zip(with_attr[1], without[1])) and torch.equal(with_attr[2], without[2])
    assert all(torch.equal(with_attr[3][k], without[3][k]) for k in with_attr[3])


def test_frozen_layers_take_the_one_pass_backward():
    """the launch trace of a frozen trunk: one hbm:bn_backward bracket per BatchNorm as before, the frozen ones at 3 (4 with a residual
    branch) tensor transfers instead of 5 (6), the direct stem kernel where it was, Dropout2d behind the heads as before"""
    _need_gpu()
    from miccai2021_cataract_semantic_segmentation_amd import ops
    traces = {}
    for select in (None, "backbone"):
        net = _ocrnet(select)
        model = _load(net)
        ops.PROFILE = []
        try:
            net["loss"](model(net["x"].cuda()), net["lbl"].cuda()).backward()
            torch.cuda.synchronize()
            traces[select] = [(p[0], p[1]) for p in ops.PROFILE]
        finally:
            ops.PROFILE = None
    kinds = {s: [k for k, _ in t] for s, t in traces.items()}
    assert kinds["backbone"].count("hbm:bn_backward") + kinds["backbone"].count("hbm:head_backward_drop") \
        == kinds[None].count("hbm:bn_backward") + kinds[None].count("hbm:head_backward_drop")
    assert kinds["backbone"].count("hbm:stem7") == kinds[None].count("hbm:stem7")              # (the direct stem kernel, where it ran)
    assert kinds["backbone"].count("hbm:dropout2d_apply") + 2 * kinds["backbone"].count("hbm:head_fwd_drop") == 4
    bytes_of = {s: sum(f for k, f in t if k == "hbm:bn_backward") for s, t in traces.items()}
    assert bytes_of["backbone"] < 0.8 * bytes_of[None]


def test_planes_route_producer_in_front_of_a_frozen_consumer(precision):
    """an HRNet BasicBlock at a width of the planes route: with bn2 frozen conv2's backward-weight reads bn1's output as fp32, so that output
    may not exist as planes only; both single-layer selections run, leave finite gradients and keep the frozen statistics"""
    _need_gpu()
    from miccai2021_cataract_semantic_segmentation_amd import engine
    from miccai2021_cataract_semantic_segmentation_amd.models.HRNetv2 import BasicBlock

    class Net(engine.EngineNet):
        def __init__(self):
            super().__init__()
            self.pre = engine.Conv2d(8, 96, 1, bias=False)
            self.pre_bn = engine.BatchNorm2d(96)
            self.a, self.b = BasicBlock(96, 96), BasicBlock(96, 96)

        def _body(self, cx, x):
            t = engine.conv_bn_act(cx, x.permute(0, 2, 3, 1).contiguous(), self.pre, self.pre_bn)
            return [self.b.run(cx, self.a.run(cx, t))]
    for select in (["b.bn2"], ["b.bn1"], ["a.bn2", "b.bn1"]):
        torch.manual_seed(3)
        net = Net().cuda().train()
        assert engine.freeze_bn(net, select) == select
        before = running_buffers(net)
        x = torch.randn(2, 8, 40, 48, device="cuda")
        out = net(x)
        out = out[0] if isinstance(out, (tuple, list)) else out
        out.backward(torch.randn_like(out))
        torch.cuda.synchronize()
        assert all(p.grad is not None and bool(torch.isfinite(p.grad).all()) and float(p.grad.abs().max()) > 0 for p in net.parameters())
        after = running_buffers(net)
        for k in after:
            assert torch.equal(after[k], before[k]) == (k.rsplit(".", 1)[0] in select), k


# ---- the manager: one epoch eager and with hip_graph, checkpoint, resume, validate()
def test_encdec_manager_with_a_frozen_trunk(tmp_path):
    _need_gpu()
    from miccai2021_cataract_semantic_segmentation_amd import managers

    def cfg(path, **train):
        return {"name": "frozen", "mode": "training", "manager": "EncDec", "log_path": str(path), "freeze_bn": "backbone",
                "encoder": {"model": "ResNet18", "pretrained": False}, "decoder": {"model": "UPerNet"}, "loss": {"losses": {"LovaszSoftmax": 1}},
                "data": {"experiment": 2, "batch_size": 2, "num_workers": 0},
                "train": dict({"learning_rate": 1e-3, "lr_fct": "exponential", "lr_restarts": [], "lr_restart_vals": 1, "lr_batchwise": False,
                               "epochs": 1}, **train), "gpu_device": 0, "seed": 0, "log_every_n_epochs": 1}
    tr = managers.SyntheticCataractDataset(6, 64, 96, 17, seed=1)
    va = managers.SyntheticCataractDataset(2, 64, 96, 17, seed=2)
    runs = []
    for hip_graph in (False, True):
        torch.manual_seed(0)
        m = managers.EncDecManager(cfg(tmp_path / ("graph" if hip_graph else "eager"), hip_graph=hip_graph), tr, va)
        assert len(m.model.frozen_bn) == 20 and all(n.startswith("enc_model.") for n in m.model.frozen_bn)
        before = running_buffers(m.model)
        torch.manual_seed(1)            # (the loader's shuffle)
        m.train()
        assert m.global_step == 3 and np.isfinite(m.history[0]["train_loss"]) and "valid_miou" in m.history[0]
        moved_and_kept(m.model, before)
        assert json.load(open(m.log_dir / "info.json"))["frozen_bn_modules"] == 20
        runs.append(m)
    eager, graph = runs
    assert eager.history[0]["train_loss"] == graph.history[0]["train_loss"] and torch.equal(eager.model.flat().flat, graph.model.flat().flat)
    # the checkpoint has the reference's keys (no trace of the attribute), and a resumed manager continues with the trunk frozen
    ck = torch.load(str(eager.log_dir / "chkpts" / "chkpt_best.pt"), weights_only=False)
    plain = managers.EncDecManager(dict(cfg(tmp_path / "plain"), freeze_bn=None), tr, va)
    assert list(ck["model_state_dict"]) == list(plain.model.state_dict()) and plain.model.frozen_bn == []
    again = managers.EncDecManager(cfg(tmp_path / "again"), tr, va)
    again.log_dir = eager.log_dir
    again.load_checkpoint("last")
    assert again.global_step == 3 and torch.equal(again.model.flat().flat, eager.model.flat().flat)
    before = running_buffers(again.model)
    assert all(torch.equal(before[k], v) for k, v in running_buffers(eager.model).items())
    again.train_loader, again.valid_loader = again.loaders()
    again.epoch, again.scheduler = 0, None          # (the restored schedule is the one-epoch run's: it has no entry for a further epoch)
    again.train_one_epoch()
    moved_and_kept(again.model, before)
    assert np.isfinite(again.validate()) and not again.model.training
    assert len(again.model.frozen_bn) == 20 and again.model.enc_model.bn1.frozen
