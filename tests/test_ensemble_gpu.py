"""The fused ensemble merge (softmax per member, mean / max over members, argmax: one launch), the normalising input transform,
models.Ensemble against the reference fixture and EnsembleManager end to end."""
import ctypes
import json
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _ensemble_ref as ER  # noqa: E402

pytestmark = pytest.mark.gpu

FULL = 544 * 960
# (K, M, P): every K in {8, 17, 25, 64}, M in {1, 2, 3, 8}, P in {1, 255, 4096, 544 * 960}; the first three are the reference fixture's inputs
MERGE_CASES = [(8, 3, 4096), (17, 3, 4096), (25, 3, 4096), (64, 8, 4096), (17, 1, 255), (8, 2, 1), (25, 3, FULL), (64, 2, 255), (25, 8, 1),
               (8, 1, 4096), (17, 2, FULL)]


def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")


def merge_case(K, M, P, mode, fixture=None):
    """inputs and CPU references of one merge case: logits (M x [1, K, 1, P], randn * 4, seed 0), the fp64 restatement, the fp32 torch
    evaluation, its distance d32 to fp64, and the pixels whose fp64 top-2 margin exceeds 4 x the bar (bar = 2 x d32)"""
    if fixture is not None:
        zs = [z.reshape(1, K, 1, P) for z in ER.merge_case_logits(K, M)]
    else:
        g = torch.Generator().manual_seed(0)
        zs = [torch.randn(1, K, 1, P, generator=g) * 4 for _ in range(M)]
    ref64 = ER.merge([z.double() for z in zs], mode)
    ref32 = ER.merge(zs, mode)
    d32 = float((ref32.double() - ref64).abs().max())
    bar = 2.0 * d32
    top2 = ref64.topk(min(2, K), dim=1).values
    keep = (top2[:, 0] - top2[:, 1] > 4.0 * bar).reshape(P) if K > 1 else torch.ones(P, dtype=torch.bool)
    rows = lambda t: t.reshape(K, P).t()                                                   # noqa: E731  [P][K]
    return {"logits": [rows(z).contiguous() for z in zs], "ref64": rows(ref64), "ref32": rows(ref32), "d32": d32, "bar": bar, "keep": keep,
            "excluded": 1.0 - float(keep.float().mean())}


def check_labels_against_fp64(labels, case, who):
    """argmax agreement with fp64 on the pixels whose fp64 top-2 margin exceeds 4 x the bar; at most 0.1 % of pixels may be excluded"""
    assert case["excluded"] <= 1e-3, (who, case["excluded"])
    want = case["ref64"].argmax(1)
    assert torch.equal(labels[case["keep"]], want[case["keep"]]), who


def test_fp32_reference_satisfies_the_label_condition():
    """the seed / input scale of the merge cases: the fp32 CPU evaluation itself agrees with fp64 on every kept pixel, and fewer than
    0.1 % of pixels are excluded (no device needed, but kept with the cases it vouches for)"""
    for K, M, P in MERGE_CASES:
        for mode in ("mean", "max"):
            c = merge_case(K, M, P, mode)
            check_labels_against_fp64(c["ref32"].argmax(1), c, ("fp32 CPU", K, M, P, mode))


GUARD = 4096          # floats / labels of guard band on each side of an output


def run_merge(logits, K, mode, ld_in, ld_probs, want_probs=True, want_labels=True, misalign=0):
    """direct C-ABI call with guard-banded outputs; returns (probs [P][K] CPU, labels [P] CPU, pad columns all zero)"""
    from miccai2021_cataract_semantic_segmentation_amd import _lib, ops
    dev = torch.device("cuda")
    P = logits[0].shape[0]
    ins = []
    for z, ld in zip(logits, ld_in):
        t = ops.new_act(1, 1, P, K, dev, ld=ld, zero=True)
        t.copy_(z.view(1, 1, P, K))
        ins.append(t)
    sentinel = -12345.0
    pbuf = torch.full((2 * GUARD + P * ld_probs,), sentinel, dtype=torch.float32, device=dev)
    lbuf = torch.full((2 * GUARD + P,), -7, dtype=torch.int64, device=dev)
    g0 = GUARD - misalign                                   # misalign: the output does not start on a 16-byte boundary
    probs = pbuf[g0:g0 + P * ld_probs]
    labels = lbuf[GUARD:GUARD + P]
    ptrs = (ctypes.c_void_p * len(ins))(*[t.data_ptr() for t in ins])
    lds = (ctypes.c_int * len(ins))(*[ops.ld_of(t) if P > 1 else ld for t, ld in zip(ins, ld_in)])
    _lib.check(_lib.lib.catseg_ensemble_merge(ptrs, lds, len(ins), P, K, ops.MERGE_MODES[mode], probs.data_ptr() if want_probs else None,
                                              ld_probs, labels.data_ptr() if want_labels else None, _lib.stream()))
    torch.cuda.synchronize()
    ph, lh = pbuf.cpu(), lbuf.cpu()
    assert bool((ph[:g0] == sentinel).all()) and bool((ph[g0 + P * ld_probs:] == sentinel).all()), "probs: written outside [P][ld_probs]"
    assert bool((lh[:GUARD] == -7).all()) and bool((lh[GUARD + P:] == -7).all()), "labels: written outside [P]"
    body = ph[g0:g0 + P * ld_probs].view(P, ld_probs)
    if not want_probs:
        assert bool((body == sentinel).all())
    if not want_labels:
        assert bool((lh == -7).all())
    return body[:, :K], lh[GUARD:GUARD + P], bool((body[:, K:] == 0).all())


@pytest.mark.parametrize("mode", ["mean", "max"])
@pytest.mark.parametrize("compact", [False, True])
@pytest.mark.parametrize("case", MERGE_CASES)
def test_merge_kernel_vs_fp64(case, compact, mode, golden):
    """bar on the probabilities = 2 x the fp32 torch CPU evaluation's own distance to the fp64 restatement on the same inputs (measured
    here, printed); labels == argmax of the kernel's own probabilities exactly; labels == the fp64 argmax wherever the fp64 top-2
    margin exceeds 4 x the bar"""
    _need_gpu()
    K, M, P = case
    fixture = golden("ensemble_merge") if (M, P) == (3, 4096) and K in (8, 17, 25) else None
    c = merge_case(K, M, P, mode, fixture)
    padded = (K + 3) // 4 * 4 if K % 4 else K + 4
    ld = K if compact else padded
    # one member of the padded K = 25 / P = 4096 case sits in a wide buffer (a view into a concat buffer: read without LDS staging)
    ld_in = [ld] * M
    if (K, M, P) == (25, 3, 4096) and not compact:
        ld_in[1] = 96
    misalign = 1 if (K, P) in ((17, 255), (64, 255)) else 0
    probs, labels, pad_zero = run_merge(c["logits"], K, mode, ld_in, ld, misalign=misalign)
    dist = float((probs.double() - c["ref64"]).abs().max())
    print("merge K=%d M=%d P=%d %s ld=%d: |kernel - fp64| = %.3g, |fp32 CPU - fp64| = %.3g, excluded %.2g"
          % (K, M, P, mode, ld, dist, c["d32"], c["excluded"]))
    assert pad_zero
    assert torch.equal(labels, probs.argmax(1))                       # always, all pixels
    assert dist <= c["bar"], (dist, c["d32"])
    check_labels_against_fp64(labels, c, "kernel")
    if fixture is not None and mode == "mean":
        # the reference's own fp32 output sits within d32 of fp64 and the kernel within 2 d32: within 3 d32 of each other
        want = torch.from_numpy(fixture["mean_K%d" % K]).reshape(K, P).t()
        assert torch.equal(want, c["ref32"])
        assert float((probs - want).abs().max()) <= 3.0 * c["d32"]
    # either output alone: the same values, the other buffer untouched
    only_l = run_merge(c["logits"], K, mode, ld_in, ld, want_probs=False)[1]
    only_p = run_merge(c["logits"], K, mode, ld_in, ld, want_labels=False)[0]
    assert torch.equal(only_l, labels) and torch.equal(only_p, probs)


@pytest.mark.parametrize("B", [1, 2])
@pytest.mark.parametrize("size", [(7, 5), (64, 96), (544, 960), (1088, 1920)])
def test_nchw3_to_nhwc4_norm_bit_exact(size, B):
    _need_gpu()
    from miccai2021_cataract_semantic_segmentation_amd import ops
    H, W = size
    x = torch.rand(B, 3, H, W, generator=torch.Generator().manual_seed(H + B))
    want = ER.normalize(x)
    got = ops.nchw3_to_nhwc4_norm(x.cuda()).cpu()
    assert got.shape == (B, H, W, 4)
    assert torch.equal(got[..., :3].permute(0, 3, 1, 2), want)
    assert bool((got[..., 3] == 0).all())
    mean, std = (0.1, -0.2, 0.3), (0.5, 2.0, 0.7)
    assert torch.equal(ops.nchw3_to_nhwc4_norm(x.cuda(), mean, std).cpu()[..., :3].permute(0, 3, 1, 2), ER.normalize(x, mean, std))


def _fixture_ensemble(golden, merge="mean"):
    from oracle.state import fill_state
    from miccai2021_cataract_semantic_segmentation_amd.models import Ensemble
    g = golden("ensemble")
    ens = Ensemble({"merge": merge, "members": ER.member_configs()}, 3)
    for m, spec, seed in zip(ens.members, json.loads(str(g["specs"])), g["seeds"]):
        m.load_state_dict(fill_state(spec, int(seed)))
    return ens.cuda().eval(), g


def test_ensemble_matches_reference_fixture(golden):
    _need_gpu()
    from miccai2021_cataract_semantic_segmentation_amd import ops
    ens, g = _fixture_ensemble(golden)
    assert all(next(m.parameters()).is_cuda and not m.training for m in ens.members)
    x = torch.from_numpy(g["x"])
    want_members = [torch.from_numpy(golden("ensemble_member%d" % i)["logits"]) for i in (1, 2, 3)]
    got_members = [z.permute(0, 3, 1, 2).cpu() for z in ens._member_logits(x.cuda())]
    scales = []
    for name, got, want in zip(ens.members_names, got_members, want_members):
        err, scale = float((got.double() - want.double()).abs().max()), float(want.abs().max())
        print("member %s: |logits - reference| = %.3g, logit scale %.3g" % (name, err, scale))
        assert err <= 3e-3 * scale, (name, err, scale)          # the project's bar for eval forwards through folded BatchNorm
        scales.append(scale)
    out = ens(x.cuda())
    assert out.shape == (1, 25, 64, 96)
    want = torch.from_numpy(g["merged"])
    err = float((out.cpu().double() - want.double()).abs().max())
    print("merged probabilities: |ensemble - reference| = %.3g (bar %.3g)" % (err, 3e-3 * max(scales)))
    assert err <= 3e-3 * max(scales)                            # |dp / dz| <= 1/2 per softmax: the members' logit bar carries over
    assert float((out.argmax(1).cpu() == torch.from_numpy(g["argmax"]).long()).float().mean()) > 0.995
    # the UPerNet member received the normalised frame: the same member alone on the torch-normalised frame, entering the stem in the
    # same NHWC-4 layout, gives the same bits
    alone = ens.members[2](ops.nchw3_to_nhwc4(ER.normalize(x).cuda())).cpu()
    assert torch.equal(alone, got_members[2])
    raw = ens.members[2](x.cuda()).cpu()
    assert not torch.equal(raw, got_members[2])
    for i in (0, 1):
        assert torch.equal(ens.members[i](x.cuda()).cpu(), got_members[i])


def test_predict_determinism_and_max_merge(golden):
    _need_gpu()
    ens, g = _fixture_ensemble(golden)
    x = torch.from_numpy(g["x"]).cuda()
    a = ens(x).cpu().clone()
    b = ens(x).cpu().clone()
    assert torch.equal(a, b)
    lab = ens.predict(x)
    assert lab.shape == (1, 64, 96) and lab.dtype == torch.int64
    assert torch.equal(lab.cpu(), a.argmax(1))
    mx, _ = _fixture_ensemble(golden, "max")
    zs = [z.permute(0, 3, 1, 2).clone() for z in mx._member_logits(x)]
    got = mx(x)
    dev = torch.stack([torch.softmax(z, 1) for z in zs]).max(0).values
    zc = [z.cpu() for z in zs]
    ref64 = ER.merge([z.double() for z in zc], "max")
    d32 = float((ER.merge(zc, "max").double() - ref64).abs().max())
    e_dev, e64 = float((got - dev).abs().max()), float((got.cpu().double() - ref64).abs().max())
    print("max merge: |kernel - torch on device| = %.3g, |kernel - fp64| = %.3g, |fp32 CPU - fp64| = %.3g" % (e_dev, e64, d32))
    assert e_dev <= 2.0 * d32 and e64 <= 2.0 * d32
    assert torch.equal(mx.predict(x).cpu(), got.cpu().argmax(1))


def _train_members(tmp_path, experiment, K):
    from miccai2021_cataract_semantic_segmentation_amd import managers
    tr = managers.SyntheticCataractDataset(4, 64, 96, K, seed=1)
    va = managers.SyntheticCataractDataset(2, 64, 96, K, seed=2)
    base = {"log_path": str(tmp_path), "data": {"experiment": experiment, "batch_size": 2}, "train": {"learning_rate": 1e-4, "epochs": 1},
            "log_every_n_epochs": 1, "seed": 0}
    cfgs = [
        ("OCRNet", dict(base, name="ocr", manager="OCRNet", graph={"model": "OCRNet", "backbone": "resnet50", "out_stride": 8, "pretrained": False},
                        loss={"name": "TwoScaleLoss", "interm": {"name": "LovaszSoftmax", "args": [], "weight": 0.4},
                              "final": {"name": "LovaszSoftmax", "args": [], "weight": 1.0}})),
        ("DeepLabv3Plus", dict(base, name="dlp", manager="DeepLabv3Plus", loss={"name": "LossWrapper", "losses": {"CrossEntropyLoss": 1}},
                               graph={"model": "DeepLabv3Plus", "backbone": "resnet50", "out_stride": 16, "pretrained": False})),
        ("EncDec", dict(base, name="upn", manager="EncDec", encoder={"model": "ResNet18", "pretrained": False}, decoder={"model": "UPerNet"},
                        loss={"losses": {"LovaszSoftmax": 1}})),
    ]
    members = {}
    for i, (kind, cfg) in enumerate(cfgs):
        m = getattr(managers, kind + "Manager")(cfg, tr, va)
        m.train()
        best = m.log_dir / "chkpts" / "chkpt_best.pt"
        if not best.exists():                     # (a one-epoch net may score mIoU 0: the 'best' rule then never fires)
            m.save_checkpoint(is_best=True)
        assert best.exists()
        if kind == "EncDec":
            members[str(i + 1)] = {"model": "UPerNet", "ckpt": m.run_id, "encoder": dict(cfg["encoder"]), "decoder": {"model": "UPerNet"}}
        else:
            members[str(i + 1)] = dict(cfg["graph"], ckpt=m.run_id)
        del m
    return members, va


def test_ensemble_manager_end_to_end(tmp_path):
    _need_gpu()
    import copy
    from torch.utils.data import DataLoader
    from miccai2021_cataract_semantic_segmentation_amd import managers, models
    K = 17
    members, va = _train_members(tmp_path, 2, K)
    cfg = {"name": "ens", "mode": "inference", "manager": "Ensemble", "log_path": str(tmp_path), "data": {"experiment": 2},
           "graph": {"model": "Ensemble", "merge": "mean", "members": copy.deepcopy(members)}, "loss": {"name": "LovaszSoftmax"}}
    em = managers.EnsembleManager(copy.deepcopy(cfg), None, va)
    assert isinstance(em.model, models.Ensemble) and em.model.members_names == ["OCRNet", "DeepLabv3Plus", "UPerNet"]
    assert all(next(m.parameters()).is_cuda and not m.training for m in em.model.members)
    miou = em.infer()
    assert len(miou) == 4 and all(np.isfinite(v) for v in miou)
    # the confusion matrix the manager accumulates against torch's from the three members run individually
    cm, _ = em._eval_pass(DataLoader(va, batch_size=1, shuffle=False), with_loss=False)
    want = torch.zeros((K, K), dtype=torch.int64)
    mean, std = ER.IMAGENET_MEAN, ER.IMAGENET_STD
    for img, lbl, _ in DataLoader(va, batch_size=1, shuffle=False):
        x = img.cuda().float()
        inside = [z.permute(0, 3, 1, 2).clone() for z in em.model._member_logits(x)]
        xn = (x - torch.tensor(mean, device=x.device).view(1, 3, 1, 1)) / torch.tensor(std, device=x.device).view(1, 3, 1, 1)
        with torch.no_grad():
            alone = [m(xn if name == "UPerNet" else x).clone() for m, name in zip(em.model.members, em.model.members_names)]
        assert all(torch.equal(a, b) for a, b in zip(alone, inside))          # same kernels, same weights: the same bits
        pred = torch.stack([torch.softmax(z, 1) for z in alone]).mean(0).argmax(1).cpu().reshape(-1)
        gt = lbl.reshape(-1)
        ok = (gt >= 0) & (gt < K)
        want += torch.bincount(pred[ok] * K + gt[ok], minlength=K * K).view(K, K)
    assert torch.equal(cm.cpu().long(), want)
    from miccai2021_cataract_semantic_segmentation_amd.utils.metrics import t_get_mean_iou
    m2 = tuple(float(v) for v in t_get_mean_iou(cm, 2, True, rare=True))
    assert m2 == miou
    # test-time augmentation wraps the ensemble like any single-output model
    em.config["tta"] = True
    tta = em.infer()
    assert len(tta) == 4 and all(np.isfinite(v) for v in tta) and isinstance(em.model, models.Ensemble)
    # the reference's assertion on the batch size
    with pytest.raises(AssertionError, match="batch size must be one for inference with ensemble"):
        em.model(torch.zeros(2, 3, 64, 96, device="cuda"))
    # an ensemble is not trained
    with pytest.raises(ValueError, match="inference"):
        managers.EnsembleManager(dict(copy.deepcopy(cfg), mode="training"), None, va)
    # checkpoint keys the member lacks: a projector's are ignored, anything else raises
    src = tmp_path / members["2"]["ckpt"] / "chkpts" / "chkpt_best.pt"
    ck = torch.load(str(src), weights_only=False)
    for run, key, ok in (("with_projector", "projector_model.0.weight", True), ("with_stranger", "aux_head.weight", False)):
        (tmp_path / run / "chkpts").mkdir(parents=True)
        sd = dict(ck["model_state_dict"])
        sd[key] = torch.zeros(3)
        torch.save(dict(ck, model_state_dict=sd), tmp_path / run / "chkpts" / "chkpt_best.pt")
        c2 = copy.deepcopy(cfg)
        c2["graph"]["members"]["2"]["ckpt"] = run
        if ok:
            cm2, _ = managers.EnsembleManager(c2, None, va)._eval_pass(DataLoader(va, batch_size=1, shuffle=False), with_loss=False)
            assert torch.equal(cm2, cm)
        else:
            with pytest.raises(RuntimeError, match="only projector_model variables.*aux_head.weight"):
                managers.EnsembleManager(c2, None, va)


def test_full_frame_three_members():
    """1 x 3 x 544 x 960, experiment 3, the three shipped kinds with random weights: ONE merge launch per forward"""
    _need_gpu()
    from miccai2021_cataract_semantic_segmentation_amd import ops
    from miccai2021_cataract_semantic_segmentation_amd.models import Ensemble
    torch.manual_seed(3)
    ens = Ensemble({"merge": "mean", "members": ER.member_configs()}, 3).cuda().eval()
    x = torch.rand(1, 3, 544, 960, generator=torch.Generator().manual_seed(4)).cuda()
    ops.PROFILE = []
    try:
        out = ens(x)
        kinds = [k for k, *_ in ops.PROFILE]
    finally:
        ops.PROFILE = None
    assert kinds.count("hbm:ensemble_merge") == 1
    assert out.shape == (1, 25, 544, 960) and bool(torch.isfinite(out).all())
    assert float((out.sum(1) - 1).abs().max()) <= 1e-5
    lab = ens.predict(x)
    assert lab.shape == (1, 544, 960) and torch.equal(lab.cpu(), out.cpu().argmax(1))
