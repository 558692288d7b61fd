"""The fused optimisers on whole networks (optim.py, graph.py, the managers): per-step updates against the stock torch optimisers on the CPU
in fp64 and fp32, hipGraph replay against eager steps bit for bit, checkpoints in the stock format both ways, and the managers'
config['train']['optimiser'].

Run with -s to collect the RATIO lines."""
import os
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

f32 = lambda x: float(np.float32(x))
# The C ABI takes float: hyperparameters are given as the values the kernels see, on both sides.  It matters for beta2 alone, whose
# float32 rounding moves 1 - beta2 by 1.3e-5 relative (catseg_adam_step has always formed 1 - beta in float32).
WD, LR, MU, BETAS, EPS = f32(1e-2), f32(1e-2), f32(0.9), (f32(0.9), f32(0.999)), f32(1e-8)


def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")


def _fcn(seed=3):
    """the tiny FCN of the manager tests, one real backward behind it: (model, batch, loss function)"""
    from miccai2021_cataract_semantic_segmentation_amd.losses import LovaszSoftmax
    from miccai2021_cataract_semantic_segmentation_amd.managers import SyntheticCataractDataset
    from miccai2021_cataract_semantic_segmentation_amd.models import FCN
    torch.manual_seed(seed)
    model = FCN({"width": 0.25}, 2).cuda().train()
    ds = SyntheticCataractDataset(2, 64, 96, model.num_classes, seed=seed)
    img = torch.stack([ds[i][0] for i in range(2)]).cuda()
    lbl = torch.stack([ds[i][1] for i in range(2)]).cuda()
    crit = LovaszSoftmax({"experiment": 2})
    return model, img, lbl, crit


def _backward(model, img, lbl, crit):
    model.zero_grad()
    loss = crit(model(img), lbl)
    loss.backward()
    return float(loss.detach())


def _groups(model):
    from miccai2021_cataract_semantic_segmentation_amd.optim import param_groups
    return param_groups(model, WD, no_decay=("norm", "bias"), lr_mult={"conv1": 0.1})


def _stock(cls, model, groups, dtype, **kw):
    """the stock optimiser over CPU copies (logical OIHW shape) of the model's parameters, in the same groups; copies in model order"""
    copy = {id(p): torch.nn.Parameter(p.detach().cpu().to(dtype).contiguous()) for p in model.parameters()}
    gs = []
    for g in groups:
        d = {"params": [copy[id(p)] for p in g["params"]], "weight_decay": g["weight_decay"]}
        if "lr_mult" in g:
            d["lr"] = kw["lr"] * g["lr_mult"]
        gs.append(d)
    return [copy[id(p)] for p in model.parameters()], cls(gs, **kw)


def _set_grads(params, model, dtype):
    for c, p in zip(params, model.parameters()):
        c.grad = p.grad.detach().cpu().to(dtype).contiguous()


def _cat(ts):
    return torch.cat([t.detach().flatten().cpu() for t in ts])


def _state_cat(sd, key):
    return torch.cat([sd["state"][i][key].detach().flatten().cpu() for i in sorted(sd["state"])])


@pytest.mark.parametrize("which", ["sgd", "adamw"])
def test_per_step_update_on_a_whole_network(which):
    """three steps on the gradients of one real backward (halved from step to step), a LambdaLR between them; parameters and every state
    tensor against the stock optimiser in fp64, with its fp32 evaluation as the yardstick"""
    _need_gpu()
    from _yardstick import within
    from miccai2021_cataract_semantic_segmentation_amd.optim import FusedAdamW, FusedSGD
    model, img, lbl, crit = _fcn()
    _backward(model, img, lbl, crit)
    groups = _groups(model)
    assert len(groups) == 4 and [g["weight_decay"] for g in groups] == [WD, 0.0, WD, 0.0]
    fp = model.flat()
    norm64 = float(torch.linalg.vector_norm(fp.grad.double()))
    if which == "sgd":
        max_norm = 0.7 * norm64                          # the first step is clipped, the later ones (gradients / 2, / 4) are not
        opt = FusedSGD(model, lr=LR, momentum=MU, nesterov=True, weight_decay=WD, groups=groups, max_grad_norm=max_norm)
        kw, stock, keys, kernel = dict(lr=LR, momentum=MU, nesterov=True), torch.optim.SGD, ["momentum_buffer"], "FusedSGD"
    else:
        max_norm = None
        opt = FusedAdamW(model, lr=LR, betas=BETAS, eps=EPS, amsgrad=True, weight_decay=WD, groups=groups)
        kw, stock, keys, kernel = dict(lr=LR, betas=BETAS, eps=EPS, amsgrad=True), torch.optim.AdamW, ["exp_avg", "exp_avg_sq", "max_exp_avg_sq"], "FusedAdamW"
    assert [g["lr"] for g in opt.param_groups] == [LR, LR, LR * 0.1, LR * 0.1]
    p64, o64 = _stock(stock, model, groups, torch.float64, **kw)
    p32, o32 = _stock(stock, model, groups, torch.float32, **kw)
    lam = lambda e: [1.0, 0.5, 0.125][min(e, 2)]
    scheds = [torch.optim.lr_scheduler.LambdaLR(o, lam) for o in (opt, o64, o32)]
    factors = []
    for step in range(3):
        for params, o, dt in ((p64, o64, torch.float64), (p32, o32, torch.float32)):
            _set_grads(params, model, dt)
            if max_norm is not None:
                torch.nn.utils.clip_grad_norm_(params, max_norm)
            o.step()
        opt.step()
        torch.cuda.synchronize()
        if max_norm is not None:
            factors.append(float(opt.last_grad_norm[1]))
            assert abs(float(opt.last_grad_norm[0]) - norm64 * 0.5 ** step) <= 1e-6 * norm64
        within(kernel, "%s step%d p" % (which, step + 1), _cat(model.parameters()), _cat(p64), _cat(p32))
        sd, sd64, sd32 = opt.state_dict(), o64.state_dict(), o32.state_dict()
        for k in keys:
            within(kernel, "%s step%d %s" % (which, step + 1, k), _state_cat(sd, k), _state_cat(sd64, k), _state_cat(sd32, k))
        for s in scheds:
            s.step()
        assert [g["lr"] for g in opt.param_groups] == [g["lr"] for g in o32.param_groups]
        fp.grad.mul_(0.5)
    if max_norm is not None:
        assert factors[0] < 1 and factors[1] == 1.0 and factors[2] == 1.0, factors
    pad = torch.ones(fp.flat.numel(), dtype=torch.bool, device=fp.flat.device)
    for p in fp.params:
        pad[fp.offsets[id(p)]:fp.offsets[id(p)] + p.numel()] = False
    for t in [fp.flat] + opt.state_buffers():
        assert not bool(t[pad].any()), "a padding element moved"


def _make(which, model, groups):
    from miccai2021_cataract_semantic_segmentation_amd.optim import FusedAdamW, FusedSGD
    if which == "sgd":
        return FusedSGD(model, lr=LR, momentum=MU, dampening=0.5, weight_decay=WD, groups=groups, max_grad_norm=1.0)
    return FusedAdamW(model, lr=f32(1e-3), betas=BETAS, eps=EPS, amsgrad=True, weight_decay=WD, groups=groups, max_grad_norm=1.0)


@pytest.mark.parametrize("which", ["sgd", "adamw"])
def test_graph_replay_equals_eager_steps(which):
    """three eager steps == three GraphedTrainStep replays bit for bit (parameters, every state buffer, last_grad_norm); the schedule changes
    the rate after step 1, so a scalar frozen into the graph shows; SGD runs with dampening, so a frozen first-step flag shows too"""
    _need_gpu()
    from miccai2021_cataract_semantic_segmentation_amd.graph import GraphedTrainStep
    model, img, lbl, crit = _fcn(5)
    batches = [(img, lbl), (img.flip(0).contiguous(), lbl.flip(0).contiguous()), (img * 0.5, lbl)]
    fp = model.flat()
    w0 = fp.flat.clone()
    lam = lambda e: [1.0, 0.25, 0.25][min(e, 2)]

    def run(step_fn, opt):
        sched = torch.optim.lr_scheduler.LambdaLR(opt, lam)
        losses = []
        for xb, lb in batches:
            losses.append(step_fn(xb, lb))
            sched.step()
        torch.cuda.synchronize()
        return losses, fp.flat.clone(), [b.clone() for b in opt.state_buffers()], opt.last_grad_norm.clone(), opt._steps

    opt = _make(which, model, _groups(model))

    def eager(xb, lb):
        opt.zero_grad()
        loss = crit(model(xb), lb)
        loss.backward()
        opt.step()
        return float(loss.detach())
    l_e, w_e, s_e, n_e, k_e = run(eager, opt)
    assert k_e == 3 and not torch.equal(w_e, w0) and len(s_e) == (1 if which == "sgd" else 3)
    with torch.no_grad():
        fp.flat.copy_(w0)
    opt2 = _make(which, model, _groups(model))
    graphed = GraphedTrainStep(model, crit, opt2, *batches[0])
    l_g, w_g, s_g, n_g, k_g = run(lambda xb, lb: float(graphed(xb, lb)), opt2)
    graphed.release()
    assert l_g == l_e and k_g == 3 and graphed.replays == 3
    assert torch.equal(w_g, w_e), "parameters differ in %d elements" % int((w_g != w_e).sum())
    assert all(torch.equal(a, b) for a, b in zip(s_g, s_e)) and torch.equal(n_g, n_e)


@pytest.mark.parametrize("which", ["sgd", "adamw"])
def test_checkpoints_speak_the_stock_format(which):
    """state_dict() loads into the stock optimiser of the same groups on the CPU and has a stock instance's keys and shapes; a stock state
    dict loads back and the next fused step equals the step taken without the round trip, bit for bit"""
    _need_gpu()
    model, img, lbl, crit = _fcn(7)
    _backward(model, img, lbl, crit)
    groups = _groups(model)
    opt = _make(which, model, groups)
    opt.step()
    sd = opt.state_dict()
    stock = torch.optim.SGD if which == "sgd" else torch.optim.AdamW
    kw = dict(lr=LR, momentum=MU, dampening=0.5) if which == "sgd" else dict(lr=f32(1e-3), betas=BETAS, eps=EPS, amsgrad=True)
    params, ref = _stock(stock, model, groups, torch.float32, **kw)
    _set_grads(params, model, torch.float32)
    ref.step()
    sd_ref = ref.state_dict()
    assert sorted(sd["state"]) == sorted(sd_ref["state"]) == list(range(len(params)))
    for i in sd_ref["state"]:
        assert list(sd["state"][i]) == list(sd_ref["state"][i])
        assert all(sd["state"][i][k].shape == sd_ref["state"][i][k].shape and sd["state"][i][k].dtype == sd_ref["state"][i][k].dtype
                   for k in sd_ref["state"][i])
    assert [list(g) for g in sd["param_groups"]] == [list(g) for g in sd_ref["param_groups"]]
    assert [g["params"] for g in sd["param_groups"]] == [g["params"] for g in sd_ref["param_groups"]]
    _, loaded = _stock(stock, model, groups, torch.float32, **kw)
    loaded.load_state_dict(sd)                                    # the stock optimiser takes it
    back = loaded.state_dict()
    key = "momentum_buffer" if which == "sgd" else "max_exp_avg_sq"
    assert all(torch.equal(back["state"][i][key].cpu(), sd["state"][i][key].cpu()) for i in sd["state"])
    fp = model.flat()
    w1 = fp.flat.clone()
    opt.step()                                                    # step 2 without the round trip (the same gradients)
    torch.cuda.synchronize()
    w_a, s_a = fp.flat.clone(), [b.clone() for b in opt.state_buffers()]
    with torch.no_grad():
        fp.flat.copy_(w1)
    opt_b = _make(which, model, groups)
    opt_b.load_state_dict(back)
    assert opt_b._steps == 1
    opt_b.step()
    torch.cuda.synchronize()
    assert torch.equal(fp.flat, w_a) and all(torch.equal(a, b) for a, b in zip(opt_b.state_buffers(), s_a))
    assert not torch.equal(w_a, w1)


SGD_RECIPE = {"name": "SGD", "momentum": 0.9, "nesterov": True, "weight_decay": 1e-4, "no_decay": ["norm", "bias"], "lr_mult": {"conv1": 0.1},
              "clip_grad_norm": 1.0}


def _cfg(tmp_path, **train):
    return {"name": "fcn", "mode": "training", "manager": "FCN", "log_path": str(tmp_path), "graph": {"model": "FCN", "width": 0.25},
            "data": {"experiment": 2, "batch_size": 2}, "loss": {"name": "LovaszSoftmax"},
            "train": dict({"learning_rate": 0.5, "epochs": 1}, **train), "log_every_n_epochs": 1, "seed": 0}


def test_fcn_manager_with_the_sgd_recipe(tmp_path):
    """config['train']['optimiser']: one epoch eager (4 steps), checkpoint, resume in a second manager that replays its epoch as a hipGraph
    (4 more steps); a fixed batch scores a lower loss after the eight steps than before the first"""
    _need_gpu()
    from miccai2021_cataract_semantic_segmentation_amd import managers
    from miccai2021_cataract_semantic_segmentation_amd.optim import FusedSGD
    tr = managers.SyntheticCataractDataset(8, 64, 96, 17, seed=1)
    va = managers.SyntheticCataractDataset(2, 64, 96, 17, seed=2)
    m = managers.FCNManager(_cfg(tmp_path, optimiser=SGD_RECIPE), tr, va)
    assert type(m.optimiser) is FusedSGD and len(m.optimiser.param_groups) == 4 and m.optimiser.max_grad_norm == 1.0
    assert [g["lr"] for g in m.optimiser.param_groups] == [0.5, 0.5, 0.05, 0.05] and m.optimiser.param_groups[0]["nesterov"]
    img = torch.stack([tr[i][0] for i in range(2)]).cuda()
    lbl = torch.stack([tr[i][1] for i in range(2)]).cuda()

    def score(man):
        man.model.eval()
        with torch.no_grad():
            return float(man.forward_loss(img, lbl)[0])
    first = score(m)
    m.train()
    assert m.global_step == 4 and m.optimiser._steps == 4 and np.isfinite(m.history[0]["train_loss"])
    assert float(m.optimiser.last_grad_norm[0]) > 0
    ck = torch.load(str(m.log_dir / "chkpts" / "chkpt_best.pt"), weights_only=False)
    assert set(ck["optimiser_state_dict"]["state"][0]) == {"momentum_buffer"} and len(ck["optimiser_state_dict"]["param_groups"]) == 4
    m2 = managers.FCNManager(_cfg(tmp_path, optimiser=SGD_RECIPE, hip_graph=True), tr, va)
    m2.log_dir = m.log_dir
    m2.load_checkpoint("best")
    assert m2.start_epoch == 0 and m2.global_step == 4 and m2.optimiser._steps == 1          # (SGD's format has no step count: "past the first")
    buf = m.optimiser.state_buffers()[0]
    assert torch.equal(m2.optimiser.state_buffers()[0], buf) and torch.equal(m2.model.flat().flat, m.model.flat().flat)
    m2.train()
    assert m2.global_step == 8 and np.isfinite(m2.history[0]["train_loss"])
    last = score(m2)
    print("LOSS fixed batch: %.6f before the first step, %.6f after eight; epoch means %.6f, %.6f"
          % (first, last, m.history[0]["train_loss"], m2.history[0]["train_loss"]))
    assert last < first
    with pytest.raises(ValueError, match="unknown optimiser"):
        managers.FCNManager(_cfg(tmp_path, optimiser={"name": "Lion"}), tr, va)
    with pytest.raises(ValueError, match="unknown key"):
        managers.FCNManager(_cfg(tmp_path, optimiser={"name": "SGD", "beta": 0.9}), tr, va)


def test_managers_without_the_key_launch_the_kernel_of_old(tmp_path):
    """no config['train']['optimiser']: FusedAdam(lr), whose step launches catseg_adam_step (the 'hbm:adam' record of ops._Timed), in
    FCNManager's own load_optimiser and in BaseManager's"""
    _need_gpu()
    from miccai2021_cataract_semantic_segmentation_amd import managers, ops
    from miccai2021_cataract_semantic_segmentation_amd.optim import FusedAdam
    tr = managers.SyntheticCataractDataset(2, 64, 96, 17, seed=1)
    for cls, cfg in ((managers.FCNManager, _cfg(tmp_path)),
                     (managers.DeepLabv3PlusManager, dict(_cfg(tmp_path), manager="DeepLabv3Plus"))):
        m = cls(cfg, tr, None)
        assert type(m.optimiser) is FusedAdam and m.optimiser._plain() and len(m.optimiser.param_groups) == 1
        img = torch.stack([tr[i][0] for i in range(2)]).cuda()
        lbl = torch.stack([tr[i][1] for i in range(2)]).cuda()
        m.model.train()
        m.optimiser.zero_grad()
        m.forward_loss(img, lbl)[0].backward()
        ops.PROFILE = []
        try:
            m.optimiser.step()
            kinds = [k for k, *_ in ops.PROFILE]
        finally:
            ops.PROFILE = None
        assert kinds == ["hbm:adam"], kinds
    # ... and the optimisers of the key launch the new kernels: the norm pair right in front of the update
    from miccai2021_cataract_semantic_segmentation_amd.optim import build_optimiser
    for recipe, want in ((SGD_RECIPE, ["hbm:grad_norm", "hbm:sgd"]), ({"name": "AdamW", "amsgrad": True}, ["hbm:adam_ex"])):
        opt = build_optimiser(m.model, recipe, 1e-3)
        ops.PROFILE = []
        try:
            opt.step()
            kinds = [k for k, *_ in ops.PROFILE]
        finally:
            ops.PROFILE = None
        assert kinds == want, kinds
