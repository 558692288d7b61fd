"""PointRend's train-mode forward and backward on the GPU: engine.pointrend_train alone against fp64 autograd of the restatement
(tests/_pointrend_train_ref.py) at fixed points, the whole EncDec + PointRend step with the device draw (eager steps against hipGraph
replays, two ranks), and EncDecManager's training loop with its checkpoint."""
import copy
import os
import sys

import numpy as np
import pytest
import torch
from torch import nn

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _pointrend_ref as PR  # noqa: E402
import _pointrend_train_ref as TR  # noqa: E402
from _yardstick import within  # noqa: E402

pytestmark = pytest.mark.gpu


def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")


def _nhwc(t):
    return t.permute(0, 2, 3, 1).contiguous().cuda()


class _Head(nn.Module):
    """a point head with the interface engine.pointrend_train reads (StandardPointHead's), built from given tensors: layers of any widths"""

    def __init__(self, head):
        super().__init__()
        self.num_fc = len(head["fc"])
        for i, (w, b) in enumerate(list(head["fc"]) + [head["predictor"]], 1):
            m = nn.Conv1d(w.shape[1], w.shape[0], 1)
            m.weight.data.copy_(w)
            m.bias.data.copy_(b)
            setattr(self, "fc%d" % i if i <= self.num_fc else "predictor", m)
        self.coarse_pred_each_layer = head["coarse_in_each_layer"]

    @property
    def fc_layers(self):
        return [getattr(self, "fc%d" % i) for i in range(1, self.num_fc + 1)]


def _train_points(N, P, g):
    """fixed points with three on one pixel (the last wins), neighbours that share taps, the corners and the outer half cell"""
    pts = torch.rand(N, P, 2, generator=g)
    top = 1.0 - 2.0 ** -24
    special = [(0.0, 0.0), (top, top), (0.4, 0.6), (0.4, 0.6), (0.4, 0.6), (0.43, 0.6), (0.4, 0.62), (0.01, 0.5), (0.5, 0.99), (0.5, 0.5)]
    pts[:, :len(special)] = torch.tensor(special)
    return pts


# ------------------------------------------------------------------------------------------------------------ engine.pointrend_train alone
@pytest.mark.parametrize("shape", ["fixture", "non-nested", "mixed widths", "coarse once"])
def test_pointrend_train_against_fp64_autograd_at_fixed_points(shape):
    """Forward (point logits, pred) and every gradient -- the four stages, the coarse logits, every head parameter -- within the project's
    measured bar (_yardstick.within: 4 x the distance of the fp32 torch-CPU restatement from fp64) of fp64 autograd of the restatement."""
    _need_gpu()
    from miccai2021_cataract_semantic_segmentation_amd import engine, ops
    coarse, feats, head = PR.seam_inputs(shape, 3)
    N, K, hc, wc = coarse.shape
    P, scale = 48, 4
    g = torch.Generator().manual_seed(17)
    pts = _train_points(N, P, g)
    dpl, dpred = torch.randn(N, K, P, generator=g), torch.randn(N, K, hc * scale, wc * scale, generator=g) * 0.1

    def reference(dtype):
        lc = coarse.to(dtype).requires_grad_()
        lf = [f.to(dtype).requires_grad_() for f in feats]
        lh = {"fc": [(w.to(dtype).requires_grad_(), b.to(dtype).requires_grad_()) for w, b in head["fc"]],
              "predictor": tuple(t.to(dtype).requires_grad_() for t in head["predictor"]), "coarse_in_each_layer": head["coarse_in_each_layer"]}
        pl, pred, pix = TR.forward(lc, lf, lh, pts, scale, dtype)
        ((pl * dpl.to(dtype)).sum() + (pred * dpred.to(dtype)).sum()).backward()
        params = [t for pair in lh["fc"] for t in pair] + list(lh["predictor"])
        return pl.detach(), pred.detach(), pix, lc.grad, [f.grad for f in lf], [t.grad for t in params]

    r64, r32 = reference(torch.float64), reference(torch.float32)
    assert int(torch.stack([torch.bincount(r, minlength=1).max() for r in r64[2]]).min()) >= 3       # three points on one pixel

    mod = _Head(head).cuda()
    for p in mod.parameters():
        p.grad = torch.full_like(p, float("nan"))           # the tape WRITES parameter gradients
    sampler = engine.PointSampler().cuda()
    sampler.fixed_points = pts
    cd = ops.new_act(N, hc, wc, K, "cuda", ld=32, zero=True)
    cd.copy_(coarse.permute(0, 2, 3, 1))
    fd = [_nhwc(f) for f in feats]
    cx = engine.Ctx(True, True)
    got = {}
    cx.push(lambda: got.update(coarse=cx.take(cd), feats=[cx.take(f) for f in fd]))      # (pushed first: runs last)
    coords4, pl, pred = engine.pointrend_train(cx, cd, fd, mod, sampler, P, 3, 0.75, scale)
    assert torch.equal(coords4.cpu().view(N, P, 2), pts) and sampler.state.tolist() == [0, 0, 0, 0]
    case = "%s" % shape
    within("train point_logits", case, pl.permute(0, 3, 1, 2).squeeze(3), r64[0], r32[0])
    within("train pred", case, pred.permute(0, 3, 1, 2), r64[1], r32[1])
    cx.give(pl, dpl.permute(0, 2, 1).unsqueeze(2).contiguous().cuda())
    cx.give(pred, _nhwc(dpred))
    cx.backward()
    torch.cuda.synchronize()
    within("train d coarse", case, got["coarse"].permute(0, 3, 1, 2), r64[3], r32[3])
    assert not bool(ops.widen(got["coarse"])[..., K:].any())
    for i, (gf, a, b) in enumerate(zip(got["feats"], r64[4], r32[4])):
        within("train d stage", "%s stage %d" % (case, i), gf.permute(0, 3, 1, 2), a, b)
    names = [n for n, _ in mod.named_parameters()]
    for n, p, a, b in zip(names, mod.parameters(), r64[5], r32[5]):
        within("train d head", "%s %s" % (case, n), p.grad.reshape(a.shape), a, b)


# ------------------------------------------------------------------------------------------------------------ the whole network, device draw
def _config(P=48):
    cfg = PR.model_config(96)
    cfg["decoder"].update(pr_train_num_pts=P, pr_train_on_device=True)
    return cfg


def _model(seed=5):
    from miccai2021_cataract_semantic_segmentation_amd.models import EncDec
    model = EncDec(_config(), 2)
    spec = [(k, tuple(v.shape)) for k, v in model.state_dict().items()]
    model.load_state_dict(PR.fill_state(spec, seed))
    return model.cuda().train()


def _loss_fn():
    from miccai2021_cataract_semantic_segmentation_amd import losses, ops
    ce = losses.CrossEntropyLoss(ignore_index=17)

    def fn(out, lbl):
        _, coords, point_logits, seg_logits, pred = out
        assert seg_logits is pred
        labels = ops.pointrend_point_labels(coords, lbl)
        return ce(seg_logits, lbl) + ce(point_logits.unsqueeze(3), labels.unsqueeze(2))
    return fn


def _batches(n, g):
    out = []
    for _ in range(n):
        lbl = torch.randint(0, 18, (2, 8, 8), generator=g).repeat_interleave(8, 1).repeat_interleave(8, 2)
        out.append((torch.rand(2, 3, 64, 64, generator=g).cuda(), lbl.cuda()))
    return out


def test_train_forward_returns_the_reference_tuple_and_draws_from_its_state():
    _need_gpu()
    model = _model()
    model.dec_model.reseed(1234)
    x, lbl = _batches(1, torch.Generator().manual_seed(3))[0]
    deep, coords, point_logits, seg_logits, pred = model(x)
    assert seg_logits is pred and pred.shape == (2, 17, 64, 64) and point_logits.shape == (2, 17, 48) and coords.shape == (2, 48, 2)
    assert deep.shape[:2] == (2, 512) and not coords.requires_grad and pred.requires_grad and point_logits.requires_grad
    M, kb, R = TR.counts(48, 3, 0.75)
    assert (M, kb, R) == (144, 36, 12)
    cand, rest = TR.draw(1234, 0, 0, 0, 2, M), TR.draw(1234, 0, 0, 1, 2, R)            # two draws per forward: candidates, then the rest
    assert torch.equal(coords[:, kb:].cpu(), rest)
    picked = coords[:, :kb].cpu()
    assert all(bool((cand[b][:, None] == picked[b][None]).all(2).any(0).all()) for b in range(2))      # every selected point is a candidate
    assert model.dec_model.sampler.state.tolist()[3] == 2
    # the scattered pixels of pred hold the point logits (the last point of a pixel)
    pix = TR.pixel_index(coords.cpu(), 64, 64)
    want = TR.scatter_last(pred.detach().cpu(), pix, point_logits.detach().cpu())
    assert torch.equal(want, pred.detach().cpu())
    # two ranks draw different points from the same seed
    other = _model()
    other.dec_model.reseed(1234, rank=1)
    assert not torch.equal(other(x)[1], coords) and torch.equal(other(x)[1][:, kb:].cpu(), TR.draw(1234, 0, 1, 3, 2, R))
    # the state dict keeps the reference's keys: the sampler's state is not in it
    assert not any("sampler" in k for k in model.state_dict())


def test_three_eager_steps_equal_three_graph_replays_bit_for_bit():
    _need_gpu()
    from miccai2021_cataract_semantic_segmentation_amd.graph import GraphedTrainStep
    from miccai2021_cataract_semantic_segmentation_amd.optim import FusedAdam
    batches = _batches(3, torch.Generator().manual_seed(9))
    loss_fn = _loss_fn()

    def run(graphed):
        model = _model()
        model.dec_model.reseed(77)
        opt = FusedAdam(model, lr=1e-3)
        step = GraphedTrainStep(model, loss_fn, opt, *batches[0]) if graphed else None
        seen = []
        for x, lbl in batches:
            if graphed:
                loss = step(x, lbl)
                out = step.outputs
            else:
                opt.zero_grad()
                out = model(x)
                loss = loss_fn(out, lbl)
                loss.backward()
                opt.step()
            torch.cuda.synchronize()
            seen.append((float(loss.detach()), out[1].detach().clone(), out[4].detach().clone(), model.flat().flat.clone()))
        return seen, model.dec_model.sampler.state.tolist()

    (eager, se), (graph, sg) = run(False), run(True)
    assert se == sg and se[3] == 6                              # two draws per step; warm-up and capture consumed none
    for (le, ce, pe, we), (lg, cg, pg, wg) in zip(eager, graph):
        assert le == lg and torch.equal(ce, cg) and torch.equal(pe, pg) and torch.equal(we, wg)
    assert not torch.equal(eager[0][1], eager[1][1])            # every step draws new points
    assert all(np.isfinite(l) for l, *_ in eager) and not torch.equal(eager[0][3], eager[2][3])


# ------------------------------------------------------------------------------------------------------------ the reference's fixture
def test_selection_on_the_fixtures_candidates_is_the_references_outside_the_band(golden):
    """The reference's recorded draws through the device's sampling (uncertainty, top-k, compose): outside the recorded band -- candidates
    within 4e-3 of the logit scale of the k-th uncertainty, which another evaluation may select either way -- the selected set is the
    reference's; the composed coordinates are the selected candidates followed by the random rest."""
    _need_gpu()
    from miccai2021_cataract_semantic_segmentation_amd import ops
    T = torch.from_numpy
    g = golden(TR.FIXTURE)
    cand, rest, coarse = T(g["cand0"]), T(g["rest0"]), T(g["coarse"])
    M, kb, R = TR.counts(TR.FIXTURE_P, TR.FIXTURE_RATIO, TR.FIXTURE_BETA)
    cd = ops.new_act(2, 16, 16, 17, "cuda", ld=32, zero=True)
    cd.copy_(coarse.permute(0, 2, 3, 1))
    unc = ops.pointrend_point_uncertainty(cd, cand.cuda())
    within("point_uncertainty", "fixture", unc, TR.point_uncertainty(coarse.double(), cand), T(g["unc"]))
    sel = ops.pointrend_topk(unc, kb)
    band = TR.band(T(g["unc"]), T(g["kth"][0]), float(g["scale"]))
    assert (band.sum(1) - 1).tolist() == g["band"].tolist()
    _, ref_idx = TR.select_points(T(g["unc"]), cand, rest, kb)
    assert not bool(((PR.selected(sel.cpu(), M) != PR.selected(ref_idx, M)) & ~band).any())
    coords, pix, _ = ops.pointrend_compose(cand.cuda(), sel, rest.cuda(), 64, 64)
    want = torch.cat((torch.gather(cand, 1, sel.cpu().long().unsqueeze(2).expand(-1, -1, 2)), rest), 1)
    assert torch.equal(coords.cpu(), want) and torch.equal(pix.cpu().long(), TR.pixel_index(want, 64, 64))
    if torch.equal(sel.cpu().long(), ref_idx):                   # the same selection: the reference's point SET (its order is torch.topk's)
        assert torch.equal(torch.sort(coords.cpu().view(2, -1, 1, 2)[:, :, 0, 0], 1)[0], torch.sort(T(g["coords0"])[:, :, 0], 1)[0])


class _Grads4d:
    """the model's gradients as tests/_calib.py's oracle state has them: an nn.Conv1d weight [O, I, 1] is a [O, I, 1, 1] tensor there"""

    def __init__(self, model):
        self.model = model

    def named_parameters(self):
        import types
        for k, p in self.model.named_parameters():
            yield k, types.SimpleNamespace(grad=p.grad.reshape(tuple(p.shape) + (1,)) if p.dim() == 3 and p.grad is not None else p.grad)


@pytest.mark.usefixtures("precision")
def test_encdec_pointrend_training_matches_reference_fixture(golden):
    """fixed_points = the reference's recorded coordinates.  The bars of tests/test_encdec_gpu.py: point_logits and pred within 1e-3 of the
    logit scale, both losses within 2e-4, gradient norms at rtol 5e-2, per-parameter gradients through _calib.calibrated_grad_check with the
    restatement as the forward; the two Adam steps that follow at the bars of tests/test_nets_gpu.py (5e-3 and 2e-2 of the loss)."""
    _need_gpu()
    import json
    from _calib import calibrated_grad_check
    from miccai2021_cataract_semantic_segmentation_amd import losses, ops
    from miccai2021_cataract_semantic_segmentation_amd.models import EncDec
    from miccai2021_cataract_semantic_segmentation_amd.optim import FusedAdam
    T = torch.from_numpy
    g = golden(TR.FIXTURE)
    spec = json.loads(str(g["spec"]))
    model = EncDec(TR.model_config(), 2)
    assert [k for k, _ in spec] == list(model.state_dict().keys())
    model.load_state_dict(PR.fill_state(spec, int(g["seed"])))
    model.cuda().train()
    x, lbl = T(g["x"]).cuda(), T(g["lbl"]).cuda()
    crit = losses.LossWrapper({"losses": {"CrossEntropyLoss": 1}, "experiment": 2, "device": "cuda"})
    ce = losses.CrossEntropyLoss(ignore_index=17)
    opt = FusedAdam(model, lr=1e-4)
    scale = float(g["scale"])
    seen = []
    for step in range(3):
        pts = T(g["coords%d" % step])
        model.dec_model.sampler.fixed_points = pts
        opt.zero_grad()
        deep, coords, pl, seg, pred = model(x)
        assert seg is pred and torch.equal(coords.cpu(), pts)
        labels = ops.pointrend_point_labels(coords, lbl)
        lc, lp = crit(deep, seg, lbl), ce(pl.unsqueeze(3), labels.unsqueeze(2))
        (lc + lp).backward()
        seen.append([float(lc.detach()), float(lp.detach())])
        if step == 0:
            e_pl, e_pred = float((pl.detach().cpu() - T(g["point_logits"])).abs().max()), float((pred.detach().cpu() - TR.fixture_pred(g)).abs().max())
            print("pointrend train fixture: point_logits err %.3g, pred err %.3g, bar %.3g; losses %s vs %s" % (e_pl, e_pred, 1e-3 * scale, seen[0], g["losses"][0].tolist()))
            assert e_pl <= 1e-3 * scale and e_pred <= 1e-3 * scale
            assert torch.equal(labels.cpu(), T(g["point_labels"]))
            assert abs(seen[0][0] - g["losses"][0][0]) < 2e-4 and abs(seen[0][1] - g["losses"][0][1]) < 2e-4
            names = json.loads(str(g["grad_names"]))
            P = dict(model.named_parameters())
            norms = np.array([float(P[k].grad.double().norm()) for k in names])
            np.testing.assert_allclose(norms, g["grad_norms"], rtol=5e-2, atol=1e-6)
            spec4 = [(k, tuple(s) + (1,) if len(s) == 3 else tuple(s)) for k, s in spec]
            calibrated_grad_check(_Grads4d(model), spec4, int(g["seed"]), lambda S_, x_: TR.network_forward(S_, x_, pts)[2:4],
                                  lambda o, l: sum(TR.manager_losses(o[0], o[1], l, pts)), T(g["x"]), T(g["lbl"]), label="EncDec(ResNet18+PointRend, train)")
        opt.step()
    print("pointrend train fixture: losses per step %s, reference %s" % (seen, g["losses"].tolist()))
    for s, (a, b) in enumerate(zip(seen, g["losses"].tolist())):
        assert abs(sum(a) - sum(b)) <= (2e-4 if s == 0 else (5e-3, 2e-2)[s - 1] * abs(sum(b)) + 1e-5), (s, seen, g["losses"].tolist())


# ------------------------------------------------------------------------------------------------------------ EncDecManager
@pytest.mark.parametrize("hip_graph", [False, True], ids=["eager", "hip_graph"])
def test_encdec_manager_trains_pointrend_and_its_checkpoint_validates(tmp_path, hip_graph, monkeypatch):
    _need_gpu()
    from miccai2021_cataract_semantic_segmentation_amd.graph import GraphedTrainStep
    replayed, replay = [], GraphedTrainStep.__call__
    monkeypatch.setattr(GraphedTrainStep, "__call__", lambda self, img, lbl: (lambda loss: (replayed.append(float(loss)), loss)[1])(replay(self, img, lbl)))
    from torch.utils.data import DataLoader
    from miccai2021_cataract_semantic_segmentation_amd import managers, models
    cfg = dict(_config(), name="prt", mode="training", manager="EncDec", log_path=str(tmp_path), data={"experiment": 2, "batch_size": 2},
               loss={"losses": {"CrossEntropyLoss": 1}}, train={"learning_rate": 1e-3, "epochs": 1, "hip_graph": hip_graph}, log_every_n_epochs=1, seed=0)
    torch.manual_seed(123)
    tr, va = managers.SyntheticCataractDataset(16, 64, 64, 17, seed=1), managers.SyntheticCataractDataset(2, 64, 64, 17, seed=2)
    m = managers.EncDecManager(copy.deepcopy(cfg), tr, va)
    assert isinstance(m.model.dec_model, models.PointRend) and m.model.dec_model.train_on_device
    steps, inner = [], m.forward_loss

    def spy(img, lbl):
        loss, out = inner(img, lbl)
        if m.model.training:
            steps.append((m.loss_coarse.detach(), m.loss_points.detach(), loss.detach()))
        return loss, out
    m.forward_loss = spy
    m.train()
    torch.cuda.synchronize()
    assert m.optimiser._steps == 8 and len(m.history) == 1 and np.isfinite(m.history[0]["train_loss"]) and np.isfinite(m.history[0]["valid_miou"])
    assert float(m.loss_coarse) > 0 and float(m.loss_points) > 0
    if hip_graph:                                               # (a replayed step runs forward_loss on the host once, at the capture)
        totals = replayed
    else:
        assert all(float(c + p) == float(t) for c, p, t in steps)
        totals = [float(t) for _, _, t in steps]
    assert len(totals) == 8
    first, last = totals[0] + totals[1], totals[-2] + totals[-1]
    print("PointRend training (%s), one epoch of 8 steps: loss %.4f -> %.4f" % ("hip_graph" if hip_graph else "eager", first / 2, last / 2))
    assert last < first
    # the checkpoint keeps the reference's keys and loads into an eval-mode model whose validate() runs
    ck = sorted((m.log_dir / "chkpts").glob("*.pt"))
    assert ck
    sd = torch.load(str(ck[0]), weights_only=False)["model_state_dict"]
    plain = models.EncDec(PR.model_config(96), 2)
    assert list(sd.keys()) == list(plain.state_dict().keys())
    plain.load_state_dict(sd)
    ev = managers.EncDecManager(dict(copy.deepcopy(cfg), mode="inference", load_checkpoint=m.run_id, train=dict(cfg["train"], epochs=5)), None, va)
    ev.load_checkpoint("last")
    ev.metrics["best_miou"] = 2.0                               # (an inference manager has no optimiser to save: validate() finds no new best)
    ev.load_loss()
    ev.valid_loader = DataLoader(va, batch_size=1, shuffle=False)
    assert np.isfinite(ev.validate()) and not ev.model.training
