"""Gradient accumulation on whole networks (optim.FusedOptimizer.set_accumulation / fold, graph.GraphedTrainStep(accumulate=n),
config['train']['accumulate']): the fold bit for bit, windows against the stock torch optimisers on the CPU in fp64 with their fp32 run as
the yardstick, a window of one against the step without a window, hipGraph replay against the eager loop bit for bit, the managers, the
refusals.  The network is the tiny FCN of tests/test_optim_gpu.py (no BatchNorm), whose helpers and recipes are used as they are.

Run with -s to collect the RATIO lines."""
import os
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from test_optim_gpu import (BETAS, EPS, LR, MU, SGD_RECIPE, _cat, _cfg, _fcn, _groups, _make, _need_gpu, _state_cat, _stock, f32)  # noqa: E402


def _batches(model, count, seed=11):
    """`count` different micro-batches of 2 x 3 x 64 x 96"""
    from miccai2021_cataract_semantic_segmentation_amd.managers import SyntheticCataractDataset
    ds = SyntheticCataractDataset(2 * count, 64, 96, model.num_classes, seed=seed)
    return [(torch.stack([ds[2 * k][0], ds[2 * k + 1][0]]).cuda().float().contiguous(),
             torch.stack([ds[2 * k][1], ds[2 * k + 1][1]]).cuda().long().contiguous()) for k in range(count)]


def _micro(model, opt, crit, xb, lb):
    """one micro-step up to (not including) the fold; returns the loss"""
    opt.zero_grad()
    loss = crit(model(xb), lb)
    loss.backward()
    return float(loss.detach())


def _padding(fp):
    pad = torch.ones(fp.flat.numel(), dtype=torch.bool, device=fp.flat.device)
    for p in fp.params:
        pad[fp.offsets[id(p)]:fp.offsets[id(p)] + p.numel()] = False
    return pad


# ------------------------------------------------------------------------------------------------------------ 1. the fold
def test_fold_is_exact():
    """n = 3: the window holds (g1 + g2) + g3 as the device adds them, bit for bit; padding stays 0; fold() leaves the gradient buffer
    alone; step() empties the window"""
    _need_gpu()
    model, img, lbl, crit = _fcn()
    opt = _make("sgd", model, _groups(model)).set_accumulation(3)
    fp = model.flat()
    assert fp.grad.numel() % 64 == 0 and opt._acc is None
    w0 = fp.flat.clone()
    gs = []
    for k, (xb, lb) in enumerate(_batches(model, 3)):
        _micro(model, opt, crit, xb, lb)
        g = fp.grad.clone()
        assert not opt.window_full()
        opt.fold()
        assert torch.equal(fp.grad, g), "fold() wrote the gradient buffer"
        assert opt._folded == k + 1
        gs.append(g)
    assert opt.window_full() and not torch.equal(gs[0], gs[1]) and not torch.equal(gs[1], gs[2])
    want = (gs[0] + gs[1]) + gs[2]
    torch.cuda.synchronize()
    acc = opt._acc
    assert acc.shape == fp.grad.shape and acc.data_ptr() != fp.grad.data_ptr()
    assert torch.equal(acc, want), "the window differs from g1 + g2 + g3 in %d elements" % int((acc != want).sum())
    assert bool(want.any()) and not bool(acc[_padding(fp)].any()), "a padding element moved"
    assert any(b is acc for b in opt.state_buffers())
    opt.step()
    torch.cuda.synchronize()
    assert opt._acc is acc and not bool(acc.any()) and opt._folded == 0 and opt._steps == 1 and not opt.window_full()
    assert not torch.equal(fp.flat, w0) and float(opt.last_grad_norm[0]) > 0
    with pytest.raises(RuntimeError, match="empty accumulation window"):
        opt.step()
    assert opt._steps == 1


# ------------------------------------------------------------------------------------------------------------ 2. the stock optimisers
@pytest.mark.parametrize("n", [3, 4])
@pytest.mark.parametrize("which", ["sgd", "adamw"])
def test_windows_against_the_stock_optimisers(which, n):
    """two windows of n micro-batches.  Reference: the stock optimiser on the CPU, whose .grad accumulates the micro-batches' gradients
    (read back from the device after each backward) as g_k / n -- the (loss / n).backward() form -- with clip_grad_norm_ in front of
    step(); truth = its fp64 run, yardstick = its fp32 run, bar = 4 x (tests/_yardstick.within) on parameters and every state tensor.
    n = 4: the norm the step leaves in last_grad_norm against ||sum g_k / 4|| in fp64, to 2 ulp.

    Measured on an MI355X (the RATIO / NORM lines): worst ratio 0.64 for SGD, 1.00 for AdamW; the norm within 0.47 ulp."""
    _need_gpu()
    from _yardstick import within
    model, img, lbl, crit = _fcn()
    groups = _groups(model)
    opt = _make(which, model, groups).set_accumulation(n)
    if which == "sgd":
        kw, stock, keys, kernel = dict(lr=LR, momentum=MU, dampening=0.5), torch.optim.SGD, ["momentum_buffer"], "FusedSGD+window"
    else:
        kw, stock, keys = dict(lr=f32(1e-3), betas=BETAS, eps=EPS, amsgrad=True), torch.optim.AdamW, ["exp_avg", "exp_avg_sq", "max_exp_avg_sq"]
        kernel = "FusedAdamW+window"
    p64, o64 = _stock(stock, model, groups, torch.float64, **kw)
    p32, o32 = _stock(stock, model, groups, torch.float32, **kw)
    batches = _batches(model, 2 * n)
    for window in range(2):
        for o in (o64, o32):
            o.zero_grad(set_to_none=True)
        for xb, lb in batches[window * n:(window + 1) * n]:
            _micro(model, opt, crit, xb, lb)
            opt.fold()
            for params, dt in ((p64, torch.float64), (p32, torch.float32)):
                for c, p in zip(params, model.parameters()):
                    term = p.grad.detach().cpu().to(dt).contiguous() / n
                    c.grad = term if c.grad is None else c.grad + term
        assert opt.window_full()
        norm64 = float(torch.linalg.vector_norm(torch.cat([c.grad.flatten() for c in p64])))
        for params, o in ((p64, o64), (p32, o32)):
            torch.nn.utils.clip_grad_norm_(params, 1.0)
            o.step()
        opt.step()
        torch.cuda.synchronize()
        assert opt._steps == window + 1 and opt._folded == 0
        case = "%s n%d window%d" % (which, n, window + 1)
        if n == 4:
            got = float(opt.last_grad_norm[0])
            ulp = float(np.spacing(np.float32(norm64)))
            print("NORM %s: kernel %.9g ref %.17g  |diff| / ulp %.3f" % (case, got, norm64, abs(got - norm64) / ulp))
            assert abs(got - norm64) <= 2 * ulp, (case, got, norm64)
        within(kernel, case + " p", _cat(model.parameters()), _cat(p64), _cat(p32))
        sd, sd64, sd32 = opt.state_dict(), o64.state_dict(), o32.state_dict()
        for k in keys:
            within(kernel, case + " " + k, _state_cat(sd, k), _state_cat(sd64, k), _state_cat(sd32, k))
    fp = model.flat()
    pad = _padding(fp)
    for t in [fp.flat] + opt.state_buffers():
        assert not bool(t[pad].any()), "a padding element moved"


# ------------------------------------------------------------------------------------------------------------ 3. a window of one
@pytest.mark.parametrize("which", ["sgd", "adamw", "adam"])
def test_a_window_of_one_is_the_step_without_a_window(which, monkeypatch):
    """three eager steps with set_accumulation(1) and fold() behind every backward == three steps of an untouched optimiser: parameters
    and state bit for bit, the same launch records (ops._Timed), no axpy and no window buffer"""
    _need_gpu()
    from miccai2021_cataract_semantic_segmentation_amd import ops
    from miccai2021_cataract_semantic_segmentation_amd.optim import FusedAdam
    model, img, lbl, crit = _fcn(5)
    fp = model.flat()
    w0 = fp.flat.clone()
    batches = _batches(model, 3)
    make = (lambda: FusedAdam(model, lr=f32(1e-3))) if which == "adam" else (lambda: _make(which, model, _groups(model)))
    folds = []
    real_axpy = ops.axpy
    monkeypatch.setattr(ops, "axpy", lambda *a, **k: (folds.append(1), real_axpy(*a, **k))[1])

    def run(opt, windowed):
        with torch.no_grad():
            fp.flat.copy_(w0)
        kinds = []
        for xb, lb in batches:
            _micro(model, opt, crit, xb, lb)
            seen = len(folds)
            ops.PROFILE = []
            try:
                if windowed:
                    opt.fold()
                opt.step()
                kinds.append([k for k, *_ in ops.PROFILE])
            finally:
                ops.PROFILE = None
            assert len(folds) == seen, "the optimiser launched an axpy"
        torch.cuda.synchronize()
        return kinds, fp.flat.clone(), [b.clone() for b in opt.state_buffers()], opt._steps

    k_a, w_a, s_a, n_a = run(make(), False)
    opt = make().set_accumulation(1)
    k_b, w_b, s_b, n_b = run(opt, True)
    assert k_a == k_b and k_a[0] == {"sgd": ["hbm:grad_norm", "hbm:sgd"], "adamw": ["hbm:grad_norm", "hbm:adam_ex"], "adam": ["hbm:adam"]}[which]
    assert n_a == n_b == 3 and opt._acc is None and opt._folded == 0
    assert torch.equal(w_a, w_b) and not torch.equal(w_a, w0)
    assert len(s_a) == len(s_b) and all(torch.equal(a, b) for a, b in zip(s_a, s_b))


# ------------------------------------------------------------------------------------------------------------ 4. graph = eager
def _lam(e):
    return [1.0, 0.25, 0.25][min(e, 2)]


def _eager_run(model, crit, opt, batches, probe):
    """the eager loop over `batches`, the schedule stepped behind every optimiser step, a partial window flushed at the end; probe(i)
    is called behind micro-step i"""
    sched = torch.optim.lr_scheduler.LambdaLR(opt, _lam)
    losses = []
    for i, (xb, lb) in enumerate(batches):
        losses.append(_micro(model, opt, crit, xb, lb))
        opt.fold()
        if opt.window_full():
            opt.step()
            sched.step()
        probe(i)
    if opt._folded:
        opt.step()
        sched.step()
    return losses


def _snapshot(model, opt):
    torch.cuda.synchronize()
    return model.flat().flat.clone(), [b.clone() for b in opt.state_buffers()], opt.last_grad_norm.clone(), opt._steps


@pytest.mark.parametrize("ema", [False, True], ids=["plain", "ema"])
@pytest.mark.parametrize("which", ["sgd", "adamw"])
def test_graph_replay_equals_the_eager_loop(which, ema):
    """7 micro-batches, n = 3: windows of 3, 3 and a flushed 1.  The schedule changes the rate after the first optimiser step (a scalar
    frozen into the tail graph shows), SGD runs with dampening (a frozen first-step flag shows), the flushed window takes its mean over
    one micro-step (a frozen 1 / 3 shows).  Parameters, every state buffer (the window and, with an average attached, its shadow
    included), last_grad_norm, the step count, the losses of all 7 micro-steps and the window in the middle of the second one: equal."""
    _need_gpu()
    from miccai2021_cataract_semantic_segmentation_amd.graph import GraphedTrainStep
    from miccai2021_cataract_semantic_segmentation_amd.optim import WeightAverage
    model, img, lbl, crit = _fcn(5)
    fp = model.flat()
    w0 = fp.flat.clone()
    batches = _batches(model, 7)

    def build():
        with torch.no_grad():
            fp.flat.copy_(w0)
        opt = _make(which, model, _groups(model)).set_accumulation(3)
        avg = opt.attach_average(WeightAverage(model, decay=0.9)) if ema else None
        return opt, avg

    mid = {}

    def probe(tag, opt):
        def at(i):
            if i == 4:          # two micro-steps into the second window
                torch.cuda.synchronize()
                mid[tag] = (opt._acc.clone(), opt._folded, opt._steps)
        return at

    opt, avg = build()
    l_e = _eager_run(model, crit, opt, batches, probe("eager", opt))
    w_e, s_e, n_e, k_e = _snapshot(model, opt)
    assert k_e == 3 and opt._folded == 0 and not torch.equal(w_e, w0)
    assert len(s_e) == (1 if which == "sgd" else 3) + 1 + (1 if ema else 0) and not bool(opt._acc.any())
    if ema:
        assert avg.n_averaged == 3
        shadow_e = avg.shadow.clone()

    opt2, avg2 = build()
    graphed = GraphedTrainStep(model, crit, opt2, *batches[0], accumulate=3)
    assert opt2._steps == 0 and opt2._folded == 0 and not bool(opt2._acc.any()) and torch.equal(fp.flat, w0)      # the warm-up left no trace
    sched = torch.optim.lr_scheduler.LambdaLR(opt2, _lam)
    l_g = []
    for i, (xb, lb) in enumerate(batches):
        before = opt2._steps
        l_g.append(float(graphed(xb, lb)))
        if opt2._steps != before:
            sched.step()
        probe("graph", opt2)(i)
    assert opt2._folded == 1 and opt2._steps == 2
    graphed.flush()
    sched.step()
    graphed.flush()                                  # an empty window: nothing
    w_g, s_g, n_g, k_g = _snapshot(model, opt2)
    assert graphed.replays == 7 and graphed.steps == 3 and k_g == 3 and opt2._folded == 0
    graphed.release()
    assert l_g == l_e, (l_g, l_e)
    assert mid["graph"][1:] == mid["eager"][1:] == (2, 1) and torch.equal(mid["graph"][0], mid["eager"][0]) and bool(mid["eager"][0].any())
    assert torch.equal(w_g, w_e), "parameters differ in %d elements" % int((w_g != w_e).sum())
    assert len(s_g) == len(s_e) and all(torch.equal(a, b) for a, b in zip(s_g, s_e)) and torch.equal(n_g, n_e)
    if ema:
        assert avg2.n_averaged == 3 and torch.equal(avg2.shadow, shadow_e) and bool(shadow_e.any())


def test_an_eager_loop_continues_the_window_a_graph_began():
    """n = 3: two replays, release(), the third micro-step and the step in the eager loop == the eager loop throughout"""
    _need_gpu()
    from miccai2021_cataract_semantic_segmentation_amd.graph import GraphedTrainStep
    model, img, lbl, crit = _fcn(5)
    fp = model.flat()
    w0 = fp.flat.clone()
    batches = _batches(model, 3)
    opt = _make("sgd", model, _groups(model)).set_accumulation(3)
    l_e = _eager_run(model, crit, opt, batches, lambda i: None)
    w_e, s_e, n_e, k_e = _snapshot(model, opt)
    with torch.no_grad():
        fp.flat.copy_(w0)
    opt2 = _make("sgd", model, _groups(model)).set_accumulation(3)
    graphed = GraphedTrainStep(model, crit, opt2, *batches[0], accumulate=3)
    l_g = [float(graphed(xb, lb)) for xb, lb in batches[:2]]
    assert opt2._folded == 2 and opt2._steps == 0
    graphed.release()
    l_g += _eager_run(model, crit, opt2, batches[2:], lambda i: None)
    w_g, s_g, n_g, k_g = _snapshot(model, opt2)
    assert l_g == l_e and k_g == k_e == 1 and torch.equal(w_g, w_e) and not torch.equal(w_e, w0)
    assert all(torch.equal(a, b) for a, b in zip(s_g, s_e)) and torch.equal(n_g, n_e)


# ------------------------------------------------------------------------------------------------------------ 5. the managers
def _sets():
    from miccai2021_cataract_semantic_segmentation_amd import managers
    return managers.SyntheticCataractDataset(10, 64, 96, 17, seed=1), managers.SyntheticCataractDataset(2, 64, 96, 17, seed=2)


def test_fcn_manager_accumulates_eager_and_graphed(tmp_path):
    """config['train']['accumulate'] = 2 with the SGD recipe on 10 frames at batch size 2: 5 micro-steps, windows of 2, 2 and a flushed 1
    in front of the scheduler; the hipGraph epoch ends bit-identical to the eager one; a checkpoint resumes with an empty window and
    a fixed batch scores a lower loss after two epochs than before the first"""
    _need_gpu()
    from miccai2021_cataract_semantic_segmentation_amd import managers
    tr, va = _sets()
    torch.manual_seed(123)                                      # (the model's default initialisation draws from the global generator)
    m = managers.FCNManager(_cfg(tmp_path / "a", optimiser=SGD_RECIPE, accumulate=2), tr, va)
    assert m.accumulate == 2 and m.optimiser._accum == 2
    img = torch.stack([tr[i][0] for i in range(2)]).cuda()
    lbl = torch.stack([tr[i][1] for i in range(2)]).cuda()

    def score(man):
        man.model.eval()
        with torch.no_grad():
            return float(man.forward_loss(img, lbl)[0])
    first = score(m)
    w_start = m.model.flat().flat.clone()
    m.train()
    assert m.global_step == 5 and m.optimiser._steps == 3 and m.history[-1]["optimiser_steps"] == 3 and np.isfinite(m.history[0]["train_loss"])
    assert m.optimiser._folded == 0 and not bool(m.optimiser._acc.any())
    torch.manual_seed(123)
    m2 = managers.FCNManager(_cfg(tmp_path / "b", optimiser=SGD_RECIPE, accumulate=2, hip_graph=True), tr, va)
    assert torch.equal(m2.model.flat().flat, w_start)
    m2.train()
    torch.cuda.synchronize()
    assert m2.global_step == 5 and m2.optimiser._steps == 3 and m2.history[-1]["optimiser_steps"] == 3
    assert m2.history[0]["train_loss"] == m.history[0]["train_loss"]
    assert torch.equal(m2.model.flat().flat, m.model.flat().flat), "the graphed epoch's parameters differ from the eager epoch's"
    assert torch.equal(m2.optimiser.state_buffers()[0], m.optimiser.state_buffers()[0]) and bool(m.optimiser.state_buffers()[0].any())
    assert m2.optimiser._folded == 0 and not bool(m2.optimiser._acc.any())
    m3 = managers.FCNManager(_cfg(tmp_path / "c", optimiser=SGD_RECIPE, accumulate=2), tr, va)
    m3.log_dir = m.log_dir
    m3.load_checkpoint("best")
    assert m3.global_step == 5 and torch.equal(m3.model.flat().flat, m.model.flat().flat)
    assert torch.equal(m3.optimiser.state_buffers()[0], m.optimiser.state_buffers()[0])
    window = m3.optimiser.state_buffers()[1]
    assert window is m3.optimiser._acc and not bool(window.any()) and m3.optimiser._folded == 0
    m3.train()
    assert m3.global_step == 10 and m3.history[-1]["optimiser_steps"] == 3 and m3.optimiser._folded == 0
    last = score(m3)
    print("LOSS fixed batch: %.6f before the first step, %.6f after two epochs of 3 optimiser steps; epoch means %.6f, %.6f"
          % (first, last, m.history[0]["train_loss"], m3.history[0]["train_loss"]))
    assert last < first


def test_fcn_manager_without_the_key(tmp_path):
    _need_gpu()
    from miccai2021_cataract_semantic_segmentation_amd import managers
    tr, va = _sets()
    m = managers.FCNManager(_cfg(tmp_path, optimiser=SGD_RECIPE), tr, va)
    m.train()
    assert m.accumulate == 1 and m.global_step == 5 and m.optimiser._steps == m.global_step
    assert "optimiser_steps" not in m.history[-1] and m.optimiser._acc is None and len(m.optimiser.state_buffers()) == 1


# ------------------------------------------------------------------------------------------------------------ 6. refusals
def test_refusals():
    _need_gpu()
    from miccai2021_cataract_semantic_segmentation_amd.graph import GraphedTrainStep
    model, img, lbl, crit = _fcn()
    opt = _make("sgd", model, _groups(model)).set_accumulation(2)
    sync = object()
    model._grad_sync = sync
    try:
        with pytest.raises(ValueError, match="exchange of an accumulated window .* is not built"):
            GraphedTrainStep(model, crit, opt, img, lbl, accumulate=2)
        assert model._grad_sync is sync and opt._hyper_dev is None and opt._acc is None          # refused before anything was touched
    finally:
        model._grad_sync = None
    with pytest.raises(ValueError, match="set_accumulation"):
        GraphedTrainStep(model, crit, opt, img, lbl)
    with pytest.raises(ValueError, match="set_accumulation"):
        GraphedTrainStep(model, crit, opt, img, lbl, accumulate=4)
    with pytest.raises(ValueError, match="int >= 1"):
        GraphedTrainStep(model, crit, opt, img, lbl, accumulate=0)
    # the tape still overwrites: the window is filled by fold(), never by a second backward()
    _micro(model, opt, crit, img, lbl)
    opt.fold()
    loss = crit(model(img), lbl)
    with pytest.raises(RuntimeError, match="second backward"):
        loss.backward()
