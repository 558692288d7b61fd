"""Host side of the fused optimisers (optim.py): the chunk map, the parameter-group builder, every refusal, the index order of the
stock-format state dictionaries, and the C ABI of include/catseg_optim.h (prototypes, the step-scalar row)."""

import numpy as np
import pytest
import torch

import _abi

SIZES = [1, 63, 64, 65, 200, 4099]          # the parameter sizes of tests/test_optim_kernels_gpu.py


def _layout(sizes, align=64):
    offs, o = [], 0
    for n in sizes:
        offs.append(o)
        o += (n + align - 1) // align * align
    return offs, o


def test_chunk_map_against_a_hand_written_map():
    from miccai2021_cataract_semantic_segmentation_amd.optim import chunk_group_map
    offs, total = _layout(SIZES)
    assert offs == [0, 64, 128, 192, 320, 576] and total == 576 + 4160
    groups = [0, 1, 2, 0, 1, 2]
    # 1 -> 1 chunk, 63 -> 1, 64 -> 1, 65 -> 2, 200 -> 4, 4099 -> 65 chunks
    want = [0] + [1] + [2] + [0, 0] + [1] * 4 + [2] * 65
    got = chunk_group_map(offs, SIZES, groups, total)
    assert got.dtype == np.uint8 and got.tolist() == want and len(want) == total // 64
    # a buffer that does not end on a chunk boundary still gets its last, partial chunk
    assert chunk_group_map([0, 64], [3, 2], [4, 7], 66).tolist() == [4, 7]
    for bad in (([0, 32], [1, 1], [0, 0], 128), ([0, 64], [65, 1], [0, 0], 128), ([0, 64], [1, 1], [0, 8], 128), ([64], [1], [0], 128),
                ([0, 64], [1, 1], [0], 128)):
        with pytest.raises(ValueError, match="chunk_group_map"):
            chunk_group_map(*bad)


class _Tree(torch.nn.Module):
    def __init__(self):
        super().__init__()
        self.backbone = torch.nn.Sequential(torch.nn.Conv2d(3, 4, 3), torch.nn.BatchNorm2d(4), torch.nn.Conv2d(4, 4, 1, bias=False))
        self.head = torch.nn.Sequential(torch.nn.Conv2d(4, 8, 1), torch.nn.GroupNorm(2, 8), torch.nn.Linear(8, 2))
        self.scale = torch.nn.Parameter(torch.ones(1))

    def flat(self):
        from miccai2021_cataract_semantic_segmentation_amd.engine import FlatParams
        if not hasattr(self, "_fp"):
            object.__setattr__(self, "_fp", FlatParams(self))
        return self._fp.ensure()


def _names(model, group):
    by_id = {id(p): n for n, p in model.named_parameters()}
    return sorted(by_id[id(p)] for p in group["params"])


def test_param_groups_names_and_prefixes():
    from miccai2021_cataract_semantic_segmentation_amd.optim import param_groups
    m = _Tree()
    gs = param_groups(m, 1e-4)
    assert [g["weight_decay"] for g in gs] == [1e-4, 0.0] and all("lr_mult" not in g for g in gs)
    assert _names(m, gs[0]) == ["backbone.0.weight", "backbone.2.weight", "head.0.weight", "head.2.weight", "scale"]
    assert _names(m, gs[1]) == ["backbone.0.bias", "backbone.1.bias", "backbone.1.weight", "head.0.bias", "head.1.bias", "head.1.weight", "head.2.bias"]
    gs = param_groups(m, 1e-4, no_decay=("bias",), lr_mult={"backbone": 0.1})
    assert [(g["weight_decay"], g.get("lr_mult")) for g in gs] == [(1e-4, None), (0.0, None), (1e-4, 0.1), (0.0, 0.1)]
    assert _names(m, gs[0]) == ["head.0.weight", "head.1.weight", "head.2.weight", "scale"]          # 'norm' is off: GroupNorm's weight decays
    assert _names(m, gs[2]) == ["backbone.0.weight", "backbone.1.weight", "backbone.2.weight"]
    assert _names(m, gs[3]) == ["backbone.0.bias", "backbone.1.bias"]
    # the longest prefix wins; every parameter exactly once under every option
    gs = param_groups(m, 0.5, no_decay=(), lr_mult={"backbone": 0.1, "backbone.2": 0.5})
    assert [(g["weight_decay"], g.get("lr_mult")) for g in gs] == [(0.5, None), (0.5, 0.1), (0.5, 0.5)] and _names(m, gs[2]) == ["backbone.2.weight"]
    for gs in (param_groups(m, 1e-4), param_groups(m, 1e-4, lr_mult={"head": 2.0, "backbone.1": 0.0}), param_groups(m, 0, no_decay=("scale", "norm"))):
        ids = [id(p) for g in gs for p in g["params"]]
        assert sorted(ids) == sorted(id(p) for p in m.parameters()) and len(set(ids)) == len(ids)


def test_group_refusals():
    from miccai2021_cataract_semantic_segmentation_amd.optim import FusedAdam, FusedAdamW, FusedSGD
    m = _Tree()
    ps = list(m.parameters())
    with pytest.raises(ValueError, match="is in parameter groups 0 and 1"):
        FusedSGD(m, groups=[{"params": ps[:5]}, {"params": ps[4:]}])
    with pytest.raises(ValueError, match="in no parameter group"):
        FusedAdam(m, groups=[{"params": ps[:5]}, {"params": ps[6:]}])
    with pytest.raises(ValueError, match="1 to 8 parameter groups, got 9"):
        FusedAdamW(m, groups=[{"params": [p]} for p in ps[:8]] + [{"params": ps[8:]}])
    with pytest.raises(ValueError, match="not a parameter of the model"):
        FusedSGD(m, groups=[{"params": ps + [torch.nn.Parameter(torch.zeros(2))]}])
    with pytest.raises(ValueError, match="'lr' and 'weight_decay' only"):
        FusedSGD(m, momentum=0.9, groups=[{"params": ps[:5]}, {"params": ps[5:], "momentum": 0.5}])
    with pytest.raises(ValueError, match="max_grad_norm"):
        FusedSGD(m, max_grad_norm=-1.0)
    opt = FusedSGD(m, lr=0.5, groups=[{"params": ps[:8], "lr_mult": 0.1, "weight_decay": 1e-4}, {"params": ps[8:]}])      # eight groups at most: fine
    assert [g["lr"] for g in opt.param_groups] == [0.05, 0.5] and all("lr_mult" not in g for g in opt.param_groups)
    assert [g["weight_decay"] for g in opt.param_groups] == [1e-4, 0]
    sched = torch.optim.lr_scheduler.LambdaLR(opt, lambda e: 0.5 ** e)
    sched.step()
    assert [g["lr"] for g in opt.param_groups] == [0.025, 0.25]                 # LambdaLR scales every group's own rate


def test_builder_refusals_and_defaults():
    from miccai2021_cataract_semantic_segmentation_amd.optim import FusedAdam, FusedAdamW, FusedSGD, build_optimiser
    m = _Tree()
    opt = build_optimiser(m, None, 1e-3, 0.5)
    assert type(opt) is FusedAdam and opt._plain() and opt.grad_scale == 0.5 and len(opt.param_groups) == 1
    with pytest.raises(ValueError, match="unknown optimiser 'LAMB'"):
        build_optimiser(m, {"name": "LAMB"}, 1e-3)
    with pytest.raises(ValueError, match=r"unknown key\(s\) \['momentun'\]"):
        build_optimiser(m, {"name": "SGD", "momentun": 0.9}, 1e-3)
    with pytest.raises(ValueError, match=r"unknown key\(s\) \['momentum'\].*for Adam"):
        build_optimiser(m, {"name": "Adam", "momentum": 0.9}, 1e-3)
    with pytest.raises(ValueError, match="with a 'name'"):
        build_optimiser(m, {"weight_decay": 0.1}, 1e-3)
    sgd = build_optimiser(m, {"name": "SGD", "momentum": 0.9, "nesterov": True, "weight_decay": 5e-4, "no_decay": ["norm", "bias"],
                              "lr_mult": {"backbone": 0.1}, "clip_grad_norm": 1.0}, 0.01, 0.25)
    assert type(sgd) is FusedSGD and sgd.max_grad_norm == 1.0 and sgd.grad_scale == 0.25
    assert [(g["lr"], g["weight_decay"], g["momentum"], g["nesterov"]) for g in sgd.param_groups] == \
        [(0.01, 5e-4, 0.9, True), (0.01, 0.0, 0.9, True), (0.001, 5e-4, 0.9, True), (0.001, 0.0, 0.9, True)]
    adamw = build_optimiser(m, {"name": "AdamW", "amsgrad": True, "betas": [0.8, 0.9], "no_decay": ["bias"]}, 1e-3)
    assert type(adamw) is FusedAdamW and [g["weight_decay"] for g in adamw.param_groups] == [1e-2, 0.0]
    assert adamw.param_groups[0]["betas"] == (0.8, 0.9) and adamw.param_groups[0]["amsgrad"] and adamw.param_groups[0]["decoupled_weight_decay"]
    assert not adamw._plain() and not FusedAdam(m, weight_decay=0.1)._plain() and not FusedAdam(m, max_grad_norm=1.0)._plain()


def test_state_dict_speaks_the_stock_format_in_group_order():
    """indices run consecutively over the groups in group order (not in model.parameters() order), and the stock optimisers load it"""
    from miccai2021_cataract_semantic_segmentation_amd.engine import FlatParams
    from miccai2021_cataract_semantic_segmentation_amd.optim import FusedAdam, FusedSGD
    m = _Tree()
    ps = list(m.parameters())
    order = [ps[i] for i in (3, 0, 7)], [ps[i] for i in (1, 2, 4, 5, 6, 8, 9, 10, 11)]
    groups = [{"params": order[0], "lr": 0.1, "weight_decay": 0.01}, {"params": order[1]}]
    torch.manual_seed(0)
    for cls, kw, keys, stock in ((FusedSGD, dict(momentum=0.9, dampening=0.5), ["momentum_buffer"], torch.optim.SGD),
                                 (FusedAdam, dict(amsgrad=True), ["step", "exp_avg", "exp_avg_sq", "max_exp_avg_sq"], torch.optim.Adam)):
        ref = stock([dict(g) for g in groups], lr=0.5, **kw)
        for p in ps:
            p.grad = torch.randn_like(p)
        ref.step()
        ref.step()
        sd_ref = ref.state_dict()
        opt = cls(m, lr=0.3, groups=groups, **kw)
        assert opt.state_dict()["state"] == {}
        opt.load_state_dict(sd_ref)
        fp = m.flat()
        assert opt._steps == (2 if cls is FusedAdam else 1) and [g["lr"] for g in opt.param_groups] == [0.1, 0.5]
        sd = opt.state_dict()
        assert [g["params"] for g in sd["param_groups"]] == [[0, 1, 2], list(range(3, 12))]
        assert [set(g) for g in sd["param_groups"]] == [set(g) for g in sd_ref["param_groups"]]
        flat_order = order[0] + order[1]
        assert sorted(sd["state"]) == list(range(12))
        for i, p in enumerate(flat_order):
            assert list(sd["state"][i]) == keys
            for k in keys:
                assert torch.equal(sd["state"][i][k], sd_ref["state"][i][k]) and (k == "step" or sd["state"][i][k].shape == p.shape)
        buf = opt._buf if cls is FusedSGD else opt._vmax
        key = keys[-1]
        assert torch.equal(FlatParams._view(buf, fp.offsets[id(ps[3])], ps[3]), sd_ref["state"][0][key])      # index 0 = the first of group 0
        back = stock([dict(g) for g in groups], lr=9.0, **kw)
        back.load_state_dict(sd)
        assert torch.equal(back.state[ps[7]][key], ref.state[ps[7]][key]) and back.param_groups[1]["lr"] == 0.5
    # refusals of what one fused launch cannot represent
    sgd = FusedSGD(m, lr=0.3, momentum=0.9, groups=groups)
    mixed = {"state": {0: {"momentum_buffer": torch.zeros_like(order[0][0])}}, "param_groups": sgd.state_dict()["param_groups"]}
    with pytest.raises(ValueError, match="momentum buffers for 1 of 12 parameters"):
        sgd.load_state_dict(mixed)
    with pytest.raises(ValueError, match="holds a momentum buffer, momentum is 0"):
        plain = FusedSGD(m, lr=0.3, groups=groups)
        plain.load_state_dict(dict(mixed, param_groups=plain.state_dict()["param_groups"]))
    adam = FusedAdam(m, groups=groups)
    sd = adam.state_dict()
    sd["state"] = {i: {"step": torch.tensor(float(1 + (i == 4))), "exp_avg": torch.zeros_like(p), "exp_avg_sq": torch.zeros_like(p)}
                   for i, p in enumerate(order[0] + order[1])}
    with pytest.raises(ValueError, match="step counts differ"):
        adam.load_state_dict(sd)
    with pytest.raises(ValueError, match="2 parameter groups, this optimiser has 1"):
        FusedAdam(m).load_state_dict(sd)
    sd["param_groups"][0]["params"], sd["param_groups"][1]["params"] = [0, 1], list(range(2, 12))
    with pytest.raises(ValueError, match="parameter group 0 of the optimiser state has 2 parameters, here it has 3"):
        adam.load_state_dict(sd)
    with pytest.raises(ValueError, match="unrecognised"):
        sgd.load_state_dict({"foo": 1})


def test_hyper_row_and_validation_without_gpu():
    """catseg_optim_hyper's row, and the refusals that come before any launch (fake, aligned device pointers)"""
    from miccai2021_cataract_semantic_segmentation_amd import _lib, ops
    lib = _lib.lib
    row = torch.full((20,), -1.0)
    ops.optim_hyper(row, 3, 0.9, 0.999, 0.125, 0.5, [0.1, 0.2, 0.3], [0.0, 1e-4, 1e-2])
    f32 = lambda x: float(np.float32(x))
    b1, b2 = f32(0.9), f32(0.999)
    want = [f32(1 - b1 ** 3), f32((1 - b2 ** 3) ** 0.5), 0.125, 0.5, f32(0.1), 0.0, f32(0.2), f32(1e-4), f32(0.3), f32(1e-2)] + [0.0] * 10
    assert row.tolist() == want
    ops.optim_hyper(row, 1, 0.9, 0.999, 1.0, 0.5, [0.1], [0.0])
    assert row[3] == 0.0 and row[0] == f32(1 - b1)                 # the first step runs without dampening
    old = torch.zeros(4)
    lib.catseg_adam_hyper(f32(0.1), 0.9, 0.999, 7, 0.5, old.data_ptr())
    ops.optim_hyper(row, 7, 0.9, 0.999, 0.5, 0.0, [0.1], [0.0])
    assert [row[4], row[0], row[1], row[2]] == old.tolist()        # the same bits as the row of catseg_adam_step_dev
    with pytest.raises(ValueError):
        ops.optim_hyper(row, 1, 0.9, 0.999, 1.0, 0.0, [0.1] * 9, [0.0] * 9)
    A = [0x10000 * (i + 1) for i in range(8)]
    host = row.data_ptr()
    adam = lambda **k: lib.catseg_adam_step_ex(*[dict(dict(p=A[0], g=A[1], m=A[2], v=A[3], vmax=None, n=1000, map=None, G=1, hh=host, hd=None, b1=0.9, b2=0.999,
                                                      eps=1e-8, wd=0, clip=None, st=None), **k)[q] for q in
                                                 ("p", "g", "m", "v", "vmax", "n", "map", "G", "hh", "hd", "b1", "b2", "eps", "wd", "clip", "st")])
    sgd = lambda **k: lib.catseg_sgd_step(*[dict(dict(p=A[0], g=A[1], buf=A[2], n=1000, map=None, G=1, hh=host, hd=None, mu=0.9, nest=0, wd=0, clip=None,
                                                 st=None), **k)[q] for q in ("p", "g", "buf", "n", "map", "G", "hh", "hd", "mu", "nest", "wd", "clip", "st")])
    need = lib.catseg_grad_norm_workspace(1 << 20)
    norm = lambda **k: lib.catseg_grad_norm(*[dict(dict(g=A[0], n=1 << 20, gs=1.0, hd=None, mx=1.0, ws=A[1], wb=need, out=A[2], st=None), **k)[q]
                                              for q in ("g", "n", "gs", "hd", "mx", "ws", "wb", "out", "st")])
    cases = [(adam, dict(p=A[0] + 4), b"16-byte"), (adam, dict(vmax=A[4] + 8), b"16-byte"), (adam, dict(G=0), b"1..8"), (adam, dict(G=9), b"1..8"),
             (adam, dict(n=0), b"positive"), (adam, dict(g=None), b"required"), (adam, dict(hd=A[5]), b"exactly one"), (adam, dict(hh=None), b"exactly one"),
             (adam, dict(wd=3), b"wd_mode"), (sgd, dict(g=A[1] + 4), b"16-byte"), (sgd, dict(buf=A[2] + 4), b"16-byte"), (sgd, dict(G=9), b"1..8"),
             (sgd, dict(G=0), b"1..8"), (sgd, dict(buf=None, nest=1), b"nesterov"), (sgd, dict(hh=None), b"exactly one"),
             (norm, dict(ws=None), b"workspace is NULL"), (norm, dict(wb=need - 1), b"smaller than"), (norm, dict(g=A[0] + 4), b"16-byte"),
             (norm, dict(out=None), b"out is required"), (norm, dict(n=0), b"positive"), (norm, dict(mx=-1.0), b"max_norm"),
             (norm, dict(mx=float("nan")), b"max_norm"), (norm, dict(ws=A[1] + 4), b"8-byte")]
    for fn, kw, msg in cases:
        rc = fn(**kw)
        err = lib.catseg_last_error()
        assert rc == 1 and msg in err and err.startswith((b"catseg_adam_step_ex:", b"catseg_sgd_step:", b"catseg_grad_norm:")), (kw, rc, err)
    # the workspace query is a function of n alone: 8 bytes per block, one block per 8192 elements, 1024 blocks at most
    assert [lib.catseg_grad_norm_workspace(n) for n in (0, 1, 8192, 8193, 1 << 23, 1 << 27)] == [0, 8, 8, 16, 8192, 8192]
    assert lib.catseg_optim_grid_cap() >= 1


def test_signature_table_matches_the_extension_header():
    """include/catseg_optim.h declares the six optimiser entry points; each has the header's signature in _lib._SIGS and is exported"""
    from miccai2021_cataract_semantic_segmentation_amd import _lib
    protos = _abi.prototypes("catseg_optim.h")
    assert sorted(protos) == ["catseg_adam_step_ex", "catseg_grad_norm", "catseg_grad_norm_workspace", "catseg_optim_grid_cap",
                              "catseg_optim_hyper", "catseg_sgd_step"]
    for name, (res, args, _) in protos.items():
        assert _lib._SIGS[name] == (res, args), "%s: header %r, table %r" % (name, (res, args), _lib._SIGS[name])
        assert hasattr(_lib.lib, name)
