"""CPU-side checks of the ensemble: the restatement the GPU tests are measured against reproduces the REAL reference's fixture, the
two new C-ABI entry points validate their arguments before any launch, and models.Ensemble handles its configuration like the reference."""
import ctypes
import json
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _ensemble_ref as ER  # noqa: E402


def test_restatement_reproduces_reference_merge_exactly(golden):
    g, members = golden("ensemble"), [torch.from_numpy(golden("ensemble_member%d" % i)["logits"]) for i in (1, 2, 3)]
    want = torch.from_numpy(g["merged"])
    got = ER.merge(members, "mean")
    assert got.dtype == torch.float32 and torch.equal(got, want)
    assert torch.equal(got.argmax(1), torch.from_numpy(g["argmax"]).long())
    gm = golden("ensemble_merge")
    for K in (8, 17, 25):
        assert torch.equal(ER.merge(ER.merge_case_logits(K), "mean"), torch.from_numpy(gm["mean_K%d" % K]))


def test_restatement_normalises_the_upernet_member_only(golden):
    """the fixture's third member (EncDec + UPerNet) saw (x - mean) / std: its stored logits follow from the oracle's network on the
    normalised frame and not on the raw one"""
    from oracle.state import fill_state
    g = golden("ensemble")
    x = torch.from_numpy(g["x"])
    S = fill_state(json.loads(str(g["specs"]))[2], int(g["seeds"][2]))
    want = torch.from_numpy(golden("ensemble_member3")["logits"])
    got = ER.member_logits("UPerNet", S, x)
    scale = float(want.abs().max())
    assert float((got - want).abs().max()) <= 1e-4 * scale
    from oracle import upernet as OU
    with torch.no_grad():
        raw = OU.encdec_forward(S, x, "ResNet18", train=False)
    raw = raw[1] if isinstance(raw, (tuple, list)) else raw
    assert float((raw - want).abs().max()) > 1e-2 * scale


def test_new_entry_points_validate_arguments_without_gpu():
    from miccai2021_cataract_semantic_segmentation_amd import _lib
    lib = _lib.lib
    assert "catseg_ensemble_merge" in _lib.EXPORTS and "catseg_nchw3_to_nhwc4_norm" in _lib.EXPORTS

    def merge(M, K, ld, probs=16, ld_probs=None, labels=16, ptrs=None, mode=0):
        n = max(M, 1)
        p = (ctypes.c_void_p * n)(*(ptrs or [16] * n))
        l = (ctypes.c_int * n)(*([ld] * n))
        return lib.catseg_ensemble_merge(p, l, M, 4096, K, mode, probs, ld if ld_probs is None else ld_probs, labels, None)

    for kw, msg in ((dict(M=0, K=25, ld=28), b"M <= 8"), (dict(M=9, K=25, ld=28), b"M <= 8"), (dict(M=3, K=65, ld=68), b"K <= 64"),
                    (dict(M=3, K=0, ld=4), b"K <= 64"), (dict(M=3, K=25, ld=24, ld_probs=28), b"ld 24 < K"),
                    (dict(M=3, K=25, ld=28, probs=None, labels=None), b"both outputs"),
                    (dict(M=3, K=25, ld=28, ptrs=[16, None, 16]), b"member 1 is NULL"), (dict(M=3, K=25, ld=28, ld_probs=24), b"ld_probs"),
                    (dict(M=3, K=25, ld=28, mode=2), b"mode")):
        assert merge(**kw) == 1, kw                                   # CATSEG_EINVAL, nothing launched
        assert msg in lib.catseg_last_error(), (kw, lib.catseg_last_error())
    mean, std = (ctypes.c_float * 3)(0.485, 0.456, 0.406), (ctypes.c_float * 3)(0.229, 0.224, 0.225)
    assert lib.catseg_nchw3_to_nhwc4_norm(16, 16, 0, 8, 8, mean, std, None) == 1
    assert lib.catseg_nchw3_to_nhwc4_norm(16, 16, 1, 8, 8, None, std, None) == 1
    assert lib.catseg_nchw3_to_nhwc4_norm(16, 24, 1, 8, 8, mean, std, None) == 1 and b"aligned" in lib.catseg_last_error()
    assert lib.catseg_nchw3_to_nhwc4_norm(16, 16, 1, 8, 8, mean, (ctypes.c_float * 3)(0.229, 0.0, 0.225), None) == 1


def test_ensemble_configuration(golden):
    from miccai2021_cataract_semantic_segmentation_amd import managers, models
    assert hasattr(managers, "EnsembleManager")
    ens = models.Ensemble({"merge": "mean", "members": ER.member_configs()}, 3)
    assert ens.members_names == ["OCRNet", "DeepLabv3Plus", "UPerNet"] and ens.ckpt_files == ["member1", "member2", "member3"]
    assert ens.num_classes == 25 and ens.num_models == 3 and ens.merge_op == "mean"
    assert len(ens.state_dict()) == 0 and len(list(ens.parameters())) == 0           # members are not registered sub-modules
    assert ens.members[0].get_intermediate is False and ens.members[2].get_features is False
    specs = json.loads(str(golden("ensemble")["specs"]))                             # checkpoint keys of the reference's members
    for m, spec in zip(ens.members, specs):
        assert [k for k, _ in spec] == list(m.state_dict().keys())
    ens.train()
    assert ens.training and not any(m.training for m in ens.members)                # nobody runs a member in training mode by accident
    ens.eval().double()
    assert all(next(m.parameters()).dtype == torch.float64 for m in ens.members)     # .to() / dtype moves reach the members
    assert models.Ensemble({"merge": "max", "members": {"1": ER.member_configs()["2"]}}, 3).num_models == 1
    with pytest.raises(AssertionError, match="batch size must be one"):
        ens.float()(torch.zeros(2, 3, 32, 32))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ens(torch.zeros(1, 3, 32, 32))
    bad = ER.member_configs()
    bad["2"]["model"] = "PointRend"
    with pytest.raises(ValueError, match="member '2'.*PointRend"):
        models.Ensemble({"merge": "mean", "members": bad}, 3)
    class OCRNet17(models.OCRNet):                       # a member built for another task: 17 classes in an experiment-3 ensemble
        def __init__(self, config, experiment):
            super().__init__(config, 2)

    wrong = {"1": dict(ER.member_configs()["1"], model="OCRNet17")}
    models.OCRNet17 = OCRNet17
    try:
        with pytest.raises(ValueError, match="member '1'.*predicts 17 classes"):
            models.Ensemble({"merge": "mean", "members": wrong}, 3)
    finally:
        del models.OCRNet17
    with pytest.raises(ValueError, match="merge"):
        models.Ensemble({"merge": "median", "members": ER.member_configs()}, 3)

