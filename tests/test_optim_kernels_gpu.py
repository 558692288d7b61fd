"""The optimiser kernels of include/catseg_optim.h on the GPU, through the C ABI: the option-free launch against catseg_adam_step
bit for bit, every option against the stock torch optimisers evaluated on the CPU in fp64 and fp32 (tests/_yardstick.within), the
deterministic gradient norm against its derived 2-ulp bound, clipped updates, and the refusals with real device buffers.

Run with -s to collect the RATIO lines."""
import os
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

f32 = lambda x: float(np.float32(x))           # the C ABI takes float: these are the values the kernels see
B1, B2, EPS = f32(0.9), f32(0.999), f32(1e-8)
SIZES = [1, 63, 64, 65, 200, 4099]             # laid out as engine.FlatParams does: every parameter on a 64-float boundary, zero gaps
GROUP_OF = [0, 1, 2, 0, 1, 2]                  # three groups alternate over the parameters
LRS = [f32(1e-2), f32(3e-3), f32(5e-4)]
WDS = [f32(1e-2), 0.0, f32(0.3)]               # one group without decay


def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")


def _ops():
    from miccai2021_cataract_semantic_segmentation_amd import ops
    return ops


def adam_grad(n, g):
    """the gradient pattern of tests/test_small_kernels_gpu.py: zeros and 1e-25 (squares to a denormal / zero in float32) mixed in"""
    gr = torch.randn(n, generator=g)
    r = torch.rand(n, generator=g)
    gr[r < 0.1] = 0.0
    gr[(r >= 0.1) & (r < 0.2)] = 1e-25
    return gr


def _layout():
    offs, o = [], 0
    for n in SIZES:
        offs.append(o)
        o += (n + 63) // 64 * 64
    return offs, o


OFFS, TOTAL = _layout()


def _to_flat(parts):
    flat = torch.zeros(TOTAL)
    for o, t in zip(OFFS, parts):
        flat[o:o + t.numel()] = t.flatten().float()
    return flat


def _real(flat):
    flat = flat.detach().cpu()
    return torch.cat([flat[o:o + n] for o, n in zip(OFFS, SIZES)])


def _padding(flat):
    keep = torch.ones(TOTAL, dtype=torch.bool)
    for o, n in zip(OFFS, SIZES):
        keep[o:o + n] = False
    return flat.detach().cpu()[keep]


def _group_map(dev):
    from miccai2021_cataract_semantic_segmentation_amd.optim import chunk_group_map
    return torch.from_numpy(chunk_group_map(OFFS, SIZES, GROUP_OF, TOTAL)).to(dev)


# ---------------------------------------------------------------------------------------------------------------- the reference side
STOCK = {"adam": torch.optim.Adam, "adamw": torch.optim.AdamW, "sgd": torch.optim.SGD}
STATE_KEYS = {"adam": ["exp_avg", "exp_avg_sq", "max_exp_avg_sq"], "adamw": ["exp_avg", "exp_avg_sq", "max_exp_avg_sq"], "sgd": ["momentum_buffer"]}


def _stock(kind, parts, dtype, wds, **kw):
    params = [torch.nn.Parameter(t.to(dtype).clone()) for t in parts]
    groups = [{"params": [p for p, gi in zip(params, GROUP_OF) if gi == k], "lr": LRS[k], "weight_decay": wds[k]} for k in range(3)]
    if kind != "sgd":
        kw = dict(kw, betas=(B1, B2), eps=EPS)
    return params, STOCK[kind](groups, **kw)


def _seed_state(opt, params, kind, state, step):
    """non-zero state into a stock optimiser (through its own state-dict format: indices run over the groups in group order)"""
    sd = opt.state_dict()
    order = [i for k in range(3) for i, gi in enumerate(GROUP_OF) if gi == k]
    sd["state"] = {}
    for idx, i in enumerate(order):
        entry = {key: state[key][i].clone() for key in state}
        if kind != "sgd":
            entry["step"] = torch.tensor(float(step))
        sd["state"][idx] = entry
    opt.load_state_dict(sd)


def _ref_state(opt, params, key):
    return torch.cat([opt.state[p][key].detach().flatten() if key in opt.state.get(p, {}) and opt.state[p][key] is not None
                      else torch.zeros(p.numel(), dtype=p.dtype) for p in params])


# ---------------------------------------------------------------------------------------------------------------- the kernel side
class Fused:
    """one optimiser state on the device, stepped through the C ABI with the scalars by value ('host') or from a device row ('dev')"""

    def __init__(self, kind, parts, wds, form, amsgrad=False, momentum=0.0, dampening=0.0, nesterov=False, grad_scale=1.0, max_norm=None):
        ops = _ops()
        dev = torch.device("cuda")
        self.kind, self.form, self.wds, self.gs = kind, form, wds, grad_scale
        self.amsgrad, self.mu, self.damp, self.nesterov, self.max_norm = amsgrad, f32(momentum), f32(dampening), nesterov, max_norm
        self.p = _to_flat(parts).to(dev)
        self.map = _group_map(dev)
        self.state = {}
        names = (["exp_avg", "exp_avg_sq"] + (["max_exp_avg_sq"] if amsgrad else [])) if kind != "sgd" else (["momentum_buffer"] if momentum else [])
        for k in names:
            self.state[k] = torch.zeros(TOTAL, device=dev)
        self.row = torch.zeros(20)
        self.row_dev = torch.zeros(20, device=dev)
        self.out = torch.zeros(2, device=dev)
        self.ws = torch.zeros(max(ops.grad_norm_workspace(TOTAL), 8), dtype=torch.uint8, device=dev)

    def load(self, state):
        for k, parts in state.items():
            if k in self.state:
                self.state[k].copy_(_to_flat(parts))

    def step(self, g_flat, step):
        ops = _ops()
        b1, b2 = (B1, B2) if self.kind != "sgd" else (0.0, 0.0)
        ops.optim_hyper(self.row, step, b1, b2, self.gs, self.damp, LRS, self.wds)
        hyper = self.row
        if self.form == "dev":
            self.row_dev.copy_(self.row)
            hyper = self.row_dev
        clip = None
        if self.max_norm is not None:
            clip = ops.grad_norm(g_flat, self.out, self.ws, self.max_norm, self.gs, hyper if self.form == "dev" else None)
        s = self.state
        if self.kind == "sgd":
            ops.sgd_step(self.p, g_flat, s.get("momentum_buffer"), hyper, G=3, group_map=self.map, momentum=self.mu, nesterov=self.nesterov,
                         use_wd=any(self.wds), clip=clip)
        else:
            mode = ops.WD_NONE if not any(self.wds) else (ops.WD_DECOUPLED if self.kind == "adamw" else ops.WD_COUPLED)
            ops.adam_step_ex(self.p, g_flat, s["exp_avg"], s["exp_avg_sq"], hyper, G=3, group_map=self.map, vmax=s.get("max_exp_avg_sq"),
                             beta1=B1, beta2=B2, eps=EPS, wd_mode=mode, clip=clip)


def _same(a, b, what):
    assert torch.equal(a.p, b.p), "%s: parameters differ between the by-value and the device form" % what
    for k in a.state:
        assert torch.equal(a.state[k], b.state[k]), "%s: %s differs between the by-value and the device form" % (what, k)


CASES = {
    "adam-coupled-wd": ("adam", WDS, dict()),
    "adamw": ("adamw", WDS, dict()),
    "adam-amsgrad": ("adam", [0.0, 0.0, 0.0], dict(amsgrad=True)),
    "adamw-amsgrad": ("adamw", WDS, dict(amsgrad=True)),
    "sgd-plain-wd": ("sgd", WDS, dict(momentum=0.0)),
    "sgd-momentum": ("sgd", [0.0, 0.0, 0.0], dict(momentum=0.9)),
    "sgd-momentum-wd": ("sgd", WDS, dict(momentum=0.9)),
    "sgd-nesterov-wd": ("sgd", WDS, dict(momentum=0.9, nesterov=True)),
    "sgd-dampening-wd": ("sgd", WDS, dict(momentum=0.9, dampening=0.5)),
}


def _stock_kw(kw):
    out = dict(kw)
    for k in ("momentum", "dampening"):
        if k in out:
            out[k] = f32(out[k])
    return out


def _check(kernel, case, fused, p64, o64, p32, o32, kind):
    from _yardstick import within
    within(kernel, case + " p", _real(fused.p), torch.cat([p.detach().flatten() for p in p64]), torch.cat([p.detach().flatten() for p in p32]))
    for k in fused.state:
        within(kernel, case + " " + k, _real(fused.state[k]), _ref_state(o64, p64, k), _ref_state(o32, p32, k))


@pytest.mark.parametrize("case", list(CASES))
def test_options_against_stock_torch(case):
    """5 steps from zero state and one late step (step 1000, non-zero state); the by-value and the device form agree bit for bit"""
    _need_gpu()
    kind, wds, kw = CASES[case]
    kernel = "sgd_step" if kind == "sgd" else "adam_step_ex"
    gen = torch.Generator().manual_seed(sum(map(ord, case)))
    parts = [torch.randn(n, generator=gen) for n in SIZES]
    grads0 = [adam_grad(n, gen) for n in SIZES]
    # amsgrad needs gradients that shrink for part of the elements (v falls below vmax) and grow for the rest (vmax follows v)
    shrink = [torch.rand(n, generator=gen) < 0.5 for n in SIZES]
    p64, o64 = _stock(kind, parts, torch.float64, wds, **_stock_kw(kw))
    p32, o32 = _stock(kind, parts, torch.float32, wds, **_stock_kw(kw))
    fh, fd = Fused(kind, parts, wds, "host", **kw), Fused(kind, parts, wds, "dev", **kw)
    for step in range(1, 6):
        grads = [torch.where(s, g * 0.01 ** (step - 1), g * 2.0 ** (step - 1)) for g, s in zip(grads0, shrink)]
        for params, opt in ((p64, o64), (p32, o32)):
            for p, g in zip(params, grads):
                p.grad = g.to(p.dtype).clone()
            opt.step()
        gf = _to_flat(grads).cuda()
        fh.step(gf, step)
        fd.step(gf, step)
        _same(fh, fd, "%s step %d" % (case, step))
        _check(kernel, "%s step%d" % (case, step), fh, p64, o64, p32, o32, kind)
        if step == 1 and kw.get("dampening"):
            # torch's first step: buf = g' exactly (here through momentum * 0 + (1 - 0) * g')
            per = [wds[k] for k in GROUP_OF]
            gp = [g.add(p0, alpha=wd) for g, p0, wd in zip(grads, parts, per)]                  # (the reference's own g')
            assert torch.equal(_ref_state(o32, p32, "momentum_buffer"), torch.cat(gp)), "the reference's first buffer is not its g'"
            gk = [g + p0 * wd for g, p0, wd in zip(grads, parts, per)]                           # (the kernel's: product and sum rounded apart)
            assert torch.equal(_real(fh.state["momentum_buffer"]), torch.cat(gk)), "buf after step 1 is not g' exactly"
    if kw.get("amsgrad"):
        v, vmax = _ref_state(o32, p32, "exp_avg_sq"), _ref_state(o32, p32, "max_exp_avg_sq")
        assert (vmax != v).float().mean() >= 0.25 and (vmax == v).float().mean() >= 0.25, "the amsgrad case does not exercise both branches"
        vk, xk = _real(fh.state["exp_avg_sq"]), _real(fh.state["max_exp_avg_sq"])
        assert (xk >= vk).all() and (xk != vk).float().mean() >= 0.25
    for t in [fh.p] + list(fh.state.values()):
        assert (_padding(t) == 0).all(), "%s: a padding element moved" % case
    # ---- one late step: non-zero state, step 1000
    state = {"exp_avg": [torch.randn(n, generator=gen) * 0.1 for n in SIZES], "exp_avg_sq": [torch.rand(n, generator=gen) * 0.01 for n in SIZES]}
    state["max_exp_avg_sq"] = [v * (1 + (torch.rand(v.numel(), generator=gen) < 0.5) * torch.rand(v.numel(), generator=gen)) for v in state["exp_avg_sq"]]
    state["momentum_buffer"] = [torch.randn(n, generator=gen) for n in SIZES]
    state = {k: v for k, v in state.items() if k in fh.state}
    parts = [torch.randn(n, generator=gen) for n in SIZES]
    grads = [adam_grad(n, gen) for n in SIZES]
    p64, o64 = _stock(kind, parts, torch.float64, wds, **_stock_kw(kw))
    p32, o32 = _stock(kind, parts, torch.float32, wds, **_stock_kw(kw))
    fh, fd = Fused(kind, parts, wds, "host", **kw), Fused(kind, parts, wds, "dev", **kw)
    for params, opt in ((p64, o64), (p32, o32)):
        if state:
            _seed_state(opt, params, kind, state, 999)
        for p, g in zip(params, grads):
            p.grad = g.to(p.dtype).clone()
        opt.step()
    gf = _to_flat(grads).cuda()
    for f in (fh, fd):
        f.load(state)
        f.step(gf, 1000)
    _same(fh, fd, case + " late step")
    _check(kernel, case + " step1000", fh, p64, o64, p32, o32, kind)
    for t in [fh.p] + list(fh.state.values()):
        assert (_padding(t) == 0).all(), "%s: a padding element moved in the late step" % case


# ---------------------------------------------------------------------------------------------------------------- option-free identity
def _sweep():
    from miccai2021_cataract_semantic_segmentation_amd import _lib
    return _lib.lib.catseg_optim_grid_cap() * 256 * 4       # elements one sweep of the new kernel's capped grid covers


@pytest.mark.parametrize("n", [1, 3, 6, 64, 65, 1003, "sweep+1"])
@pytest.mark.parametrize("gs", [1.0, 1 / 128])
def test_option_free_launch_writes_the_bits_of_adam_step(n, gs):
    """one group, no decay, no vmax, no clip, no map: catseg_adam_step_ex (both scalar forms) == catseg_adam_step == catseg_adam_step_dev on
    p, m and v, over three steps from zero state and one step at step 1000"""
    _need_gpu()
    ops = _ops()
    n = _sweep() + 1 if n == "sweep+1" else n
    lr = f32(1e-3)
    gen = torch.Generator().manual_seed(n % 1000 + 7)
    p0 = torch.randn(n, generator=gen).cuda()
    row, row_dev, old_row = torch.zeros(20), torch.zeros(20, device="cuda"), torch.zeros(4)
    old_dev = torch.zeros(4, device="cuda")
    runs = {k: [p0.clone(), torch.zeros_like(p0), torch.zeros_like(p0)] for k in ("old", "old_dev", "ex", "ex_dev")}
    for step in (1, 2, 3, 1000):
        g = adam_grad(n, gen).cuda()
        ops.optim_hyper(row, step, B1, B2, gs, 0.0, [lr], [0.0])
        row_dev.copy_(row)
        ops.lib.catseg_adam_hyper(lr, B1, B2, step, gs, old_row.data_ptr())
        old_dev.copy_(old_row)
        ops.adam_step(runs["old"][0], g, runs["old"][1], runs["old"][2], lr, step, B1, B2, EPS, gs)
        ops.adam_step_dev(runs["old_dev"][0], g, runs["old_dev"][1], runs["old_dev"][2], old_dev, B1, B2, EPS)
        ops.adam_step_ex(runs["ex"][0], g, runs["ex"][1], runs["ex"][2], row, beta1=B1, beta2=B2, eps=EPS)
        ops.adam_step_ex(runs["ex_dev"][0], g, runs["ex_dev"][1], runs["ex_dev"][2], row_dev, beta1=B1, beta2=B2, eps=EPS)
        torch.cuda.synchronize()
        for k in ("old_dev", "ex", "ex_dev"):
            for name, a, b in zip("pmv", runs["old"], runs[k]):
                assert torch.equal(a, b), "n = %d, step %d: %s of %s differs from catseg_adam_step in %d elements" % (
                    n, step, name, k, int((a != b).sum()))
    assert not torch.equal(runs["old"][0], p0)


# ---------------------------------------------------------------------------------------------------------------- the gradient norm
def _norm_input(kind, n, gen):
    if kind == "zeros":
        return torch.zeros(n)
    g = torch.randn(n, generator=gen)
    return g * {"normal": 1.0, "huge": 1e19, "tiny": 1e-30}[kind]      # 1e19 squares past fp32's range, the norm does not leave it


@pytest.mark.parametrize("n", [1, 64, 1003, 8388609, 20000003])
@pytest.mark.parametrize("kind", ["zeros", "normal", "huge", "tiny"])
def test_grad_norm_within_two_ulp_and_deterministic(n, kind):
    """|norm - ref| <= 2 ulp_fp32(ref): the square of an fp32 value is exact in fp64, the fp64 sum of n <= 2^27 such terms is off by less
    than n 2^-53 < 2^-26 relative, what remains is the square root, the product with the scale and one rounding to fp32"""
    _need_gpu()
    ops = _ops()
    gen = torch.Generator().manual_seed(n % 997 + len(kind))
    g_cpu = _norm_input(kind, n, gen)
    g = g_cpu.cuda()
    ref_norm = float(torch.linalg.vector_norm(g_cpu.double()))
    ws = torch.zeros(max(ops.grad_norm_workspace(n), 8), dtype=torch.uint8, device="cuda")
    for gs in (1.0, 1 / 8):
        for max_norm in (1.0, f32(0.37)):
            out, again = torch.full((2,), -1.0, device="cuda"), torch.full((2,), -2.0, device="cuda")
            ops.grad_norm(g, out, ws, max_norm, gs)
            ops.grad_norm(g, again, ws, max_norm, gs)
            row_dev = torch.zeros(20, device="cuda")
            row_dev[2] = gs
            via_row = torch.full((2,), -3.0, device="cuda")
            ops.grad_norm(g, via_row, ws, max_norm, 55.0, row_dev)          # the device row's scale wins over the by-value one
            torch.cuda.synchronize()
            assert torch.equal(out, again) and torch.equal(out, via_row), "two launches over the same gradients differ"
            norm, factor = np.float32(out[0].item()), np.float32(out[1].item())
            ref = ref_norm * gs
            ulp = float(np.spacing(np.float32(ref)))
            print("NORM n %d %s gs %g: kernel %.9g ref %.17g  |diff| / ulp %.3f" % (n, kind, gs, norm, ref, abs(float(norm) - ref) / ulp))
            if kind == "zeros":
                assert norm == 0.0 and factor == 1.0
            assert abs(float(norm) - ref) <= 2 * ulp, (n, kind, gs, float(norm), ref)
            want = np.minimum(np.float32(1.0), np.float32(max_norm) / (norm + np.float32(1e-6)))
            assert factor == want and isinstance(want, np.float32), (n, kind, gs, max_norm, factor, want)


# ---------------------------------------------------------------------------------------------------------------- clipped updates
@pytest.mark.parametrize("kind,kw", [("sgd", dict(momentum=0.9)), ("adamw", dict(amsgrad=True))], ids=["sgd", "adamw"])
def test_clipped_update_against_clip_grad_norm(kind, kw):
    """torch.nn.utils.clip_grad_norm_ + the stock optimiser on the CPU against grad_norm + the fused update: above max_norm the factor is
    < 1; below it the factor is exactly 1 and the update equals the unclipped launch bit for bit"""
    _need_gpu()
    kernel = "sgd_step+clip" if kind == "sgd" else "adam_step_ex+clip"
    max_norm = 1.0
    gen = torch.Generator().manual_seed(11 + len(kind))
    parts = [torch.randn(n, generator=gen) for n in SIZES]
    p64, o64 = _stock(kind, parts, torch.float64, WDS, **_stock_kw(kw))
    p32, o32 = _stock(kind, parts, torch.float32, WDS, **_stock_kw(kw))
    fh, fd = Fused(kind, parts, WDS, "host", max_norm=max_norm, **kw), Fused(kind, parts, WDS, "dev", max_norm=max_norm, **kw)
    for step in (1, 2):
        grads = [adam_grad(n, gen) for n in SIZES]                        # norm ~ sqrt(0.8 * 4492) ~ 60: clipped
        for params, opt in ((p64, o64), (p32, o32)):
            for p, g in zip(params, grads):
                p.grad = g.to(p.dtype).clone()
            total = torch.nn.utils.clip_grad_norm_(params, max_norm)
            assert float(total) > max_norm
            opt.step()
        gf = _to_flat(grads).cuda()
        fh.step(gf, step)
        fd.step(gf, step)
        _same(fh, fd, "%s clipped step %d" % (kind, step))
        assert torch.equal(fh.out, fd.out) and 0 < float(fh.out[1]) < 1 and float(fh.out[0]) > max_norm
        _check(kernel, "%s clipped step%d" % (kind, step), fh, p64, o64, p32, o32, kind)
    # below max_norm: the factor is 1 and nothing changes against the launch without a clip pointer
    grads = [adam_grad(n, gen) * 1e-3 for n in SIZES]
    gf = _to_flat(grads).cuda()
    plain = Fused(kind, parts, WDS, "host", **kw)
    plain.p.copy_(fh.p)
    for k in plain.state:
        plain.state[k].copy_(fh.state[k])
    for params, opt in ((p64, o64), (p32, o32)):
        for p, g in zip(params, grads):
            p.grad = g.to(p.dtype).clone()
        assert float(torch.nn.utils.clip_grad_norm_(params, max_norm)) < max_norm
        opt.step()
    fh.step(gf, 3)
    plain.step(gf, 3)
    assert float(fh.out[1]) == 1.0 and 0 < float(fh.out[0]) < max_norm
    assert torch.equal(fh.p, plain.p) and all(torch.equal(fh.state[k], plain.state[k]) for k in plain.state)
    _check(kernel, "%s unclipped step3" % kind, fh, p64, o64, p32, o32, kind)
    for t in [fh.p] + list(fh.state.values()):
        assert (_padding(t) == 0).all()


# ---------------------------------------------------------------------------------------------------------------- refusals
def test_refusals_with_device_buffers():
    """CATSEG_EINVAL before anything is launched: the buffers are untouched afterwards"""
    _need_gpu()
    from miccai2021_cataract_semantic_segmentation_amd import _lib
    lib, EINVAL = _lib.lib, 1
    n = 1000
    p, g, m, v = (torch.full((n + 4,), float(i + 1), device="cuda") for i in range(4))
    row = torch.zeros(20)
    st = torch.cuda.current_stream().cuda_stream
    P = lambda t, off=0: t.data_ptr() + off

    def adam(pp=P(p), G=1, vmax=None):
        return lib.catseg_adam_step_ex(pp, P(g), P(m), P(v), vmax, n, None, G, P(row), None, B1, B2, EPS, 0, None, st)

    def sgd(gg=P(g), G=1, buf=P(m)):
        return lib.catseg_sgd_step(P(p), gg, buf, n, None, G, P(row), None, 0.9, 0, 0, None, st)
    need = lib.catseg_grad_norm_workspace(1 << 20)
    ws, out = torch.zeros(need, dtype=torch.uint8, device="cuda"), torch.zeros(2, device="cuda")
    big = torch.zeros(1 << 20, device="cuda")

    def norm(workspace=P(ws), nbytes=need, gg=P(big)):
        return lib.catseg_grad_norm(gg, 1 << 20, 1.0, None, 1.0, workspace, nbytes, P(out), st)
    assert need == 128 * 8
    for call in (lambda: adam(pp=P(p, 4)), lambda: adam(vmax=P(v, 8)), lambda: adam(G=0), lambda: adam(G=9), lambda: sgd(gg=P(g, 4)),
                 lambda: sgd(buf=P(m, 4)), lambda: sgd(G=0), lambda: sgd(G=9), lambda: norm(workspace=None), lambda: norm(nbytes=need - 1),
                 lambda: norm(gg=P(big, 4))):
        assert call() == EINVAL and lib.catseg_last_error().startswith(b"catseg_")
    torch.cuda.synchronize()
    assert all(bool((t == float(i + 1)).all()) for i, t in enumerate((p, g, m, v))) and not bool(out.any())
