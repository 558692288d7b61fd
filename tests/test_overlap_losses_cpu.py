"""SoftIoU / GenDiceLoss / FocalLoss without a GPU: the package exports them with the reference's constructor contract, the C ABI
rejects bad arguments before any launch, shape errors are ValueErrors, and the torch restatement (tests/_overlap_ref.py, the oracle
of the large-shape GPU tests) reproduces the reference fixtures."""
import ctypes
import json

import numpy as np
import pytest
import torch

from miccai2021_cataract_semantic_segmentation_amd.losses import FocalLoss, GenDiceLoss, SoftIoU

T = torch.from_numpy


def test_exported_and_resolvable_by_name():
    from miccai2021_cataract_semantic_segmentation_amd import losses
    from miccai2021_cataract_semantic_segmentation_amd.managers.base import BaseManager  # noqa: F401  (load_loss: getattr on the package)
    for name in ("FocalLoss", "SoftIoU", "GenDiceLoss"):
        assert getattr(losses, name).__name__ == name


def test_constructor_contract():
    s = SoftIoU({"experiment": 1})
    assert (s.experiment, s.num_classes, s.naive) == (1, 8, False)
    assert SoftIoU({"experiment": 2}).num_classes == 18 and SoftIoU({"experiment": 3, "naive": True}).naive is True
    d = GenDiceLoss({"experiment": 3})
    assert (d.num_classes, d.weights, d.naive) == (26, None, False)
    assert GenDiceLoss({"experiment": 2, "weights": "auto"}).weights == "auto"
    with pytest.raises(ValueError):
        GenDiceLoss({"experiment": 2, "weights": [1.0] * 5})
    f = FocalLoss({})
    assert f.gamma == 2 and f.alpha is None and dict(f.named_buffers()) == {}
    f = FocalLoss({"gamma": 0.5, "alpha": [0.25, 0.75]})
    assert f.gamma == 0.5 and torch.equal(f.alpha, torch.tensor([0.25, 0.75])) and set(dict(f.named_buffers())) == {"alpha"}
    assert set(f.state_dict()) == {"alpha"}
    # reference configs as BaseManager.load_loss passes them (experiment and device added)
    GenDiceLoss({"name": "GenDiceLoss", "weights": "auto", "experiment": 2, "device": "cuda:0"})


def test_shape_and_device_errors():
    x, y = torch.zeros(1, 8, 4, 4), torch.zeros(1, 4, 4, dtype=torch.long)
    for crit in (SoftIoU({"experiment": 1}), GenDiceLoss({"experiment": 1}), FocalLoss({})):
        with pytest.raises(ValueError):
            crit(x, torch.zeros(1, 4, 5, dtype=torch.long))
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            crit(x, y)
    for crit in (SoftIoU({"experiment": 2}), GenDiceLoss({"experiment": 3})):
        with pytest.raises(ValueError):
            crit(x, y)          # 8 channels, the experiment has 17 / 25 classes


def test_abi_rejects_bad_arguments_without_gpu():
    from miccai2021_cataract_semantic_segmentation_amd import _lib
    lib = _lib.lib
    ws = lib.catseg_overlap_workspace(4177920, 25)
    assert ws >= 1024 * 76 * 8
    # P <= 0, K > 64, workspace too small, null pointers: an error code and a message, nothing launched (no stream exists here)
    assert lib.catseg_overlap_fwd(16, 16, 0, 8, -1, 0, 0, 0, None, 16, 16, 16, 16, ws, None) == 1
    assert b"P" in lib.catseg_last_error()
    assert lib.catseg_overlap_fwd(16, 16, 100, 65, -1, 0, 0, 0, None, 16, 16, 16, 16, 1 << 30, None) == 1
    assert b"K <= 64" in lib.catseg_last_error()
    assert lib.catseg_overlap_fwd(16, 16, 100, 8, -1, 0, 0, 0, None, 16, 16, 16, 16, 8, None) != 0
    assert b"workspace too small" in lib.catseg_last_error()
    assert lib.catseg_overlap_fwd(16, None, 100, 8, -1, 0, 0, 0, None, 16, 16, 16, 16, 1 << 30, None) == 1
    assert b"null pointer" in lib.catseg_last_error()
    assert lib.catseg_overlap_fwd(16, 16, 100, 8, -1, 1, 0, 2, None, 16, 16, 16, 16, 1 << 30, None) == 1   # list weights, none given
    assert lib.catseg_overlap_bwd(16, 16, -5, 8, -1, 16, None, 16, None) == 1
    assert lib.catseg_overlap_bwd(16, 16, 100, 8, -1, None, None, 16, None) == 1
    assert b"null pointer" in lib.catseg_last_error()
    assert lib.catseg_focal_fwd(16, 16, 100, 65, ctypes.c_float(2.0), None, 16, 16, 16, 1 << 30, None) == 1
    assert b"K <= 64" in lib.catseg_last_error()
    assert lib.catseg_focal_fwd(16, 16, 100, 8, ctypes.c_float(2.0), None, 16, 16, 16, 0, None) != 0
    assert b"workspace too small" in lib.catseg_last_error()
    assert lib.catseg_focal_fwd(16, 16, 0, 8, ctypes.c_float(2.0), None, 16, 16, 16, 1 << 30, None) == 1
    assert lib.catseg_focal_bwd(16, 16, 100, 8, ctypes.c_float(2.0), None, None, None, None) == 1
    assert b"null pointer" in lib.catseg_last_error()


def _cases(golden):
    g = golden("overlap_losses")
    for name in g["names"]:
        c = json.loads(str(g[name + "_cfg"]))
        yield (str(name), c["loss"], c["config"], c["scale"], T(g[name + "_logits"]), T(g[name + "_target"]), float(g[name + "_loss"]),
               T(g[name + "_grad"]))


def test_restatement_reproduces_reference_fixtures(golden):
    import _overlap_ref as R
    n = 0
    for name, loss_name, cfg, scale, logits, target, ref_loss, ref_grad in _cases(golden):
        loss, grad = R.loss_and_grad(loss_name, cfg, logits, target, torch.float64, scale)
        if np.isnan(ref_loss):
            assert torch.isnan(loss), name
        else:
            assert abs(float(loss) - ref_loss) <= 1e-6 * max(1.0, abs(ref_loss)), name
        if torch.isnan(ref_grad).all() and not np.isnan(ref_loss):
            # the reference's non-naive mean excluded a class and its backward divided 0 / 0: the restatement's gradient is finite
            assert name in ("iou_absent_mean", "dice_list_mean") and torch.isfinite(grad).all(), name
            continue
        assert torch.equal(torch.isnan(grad), torch.isnan(ref_grad)), name
        fin = torch.isfinite(ref_grad)
        np.testing.assert_allclose(grad[fin].numpy(), ref_grad[fin].double().numpy(), atol=1e-8, rtol=1e-5, err_msg=name)
        n += 1
    assert n == 25


def test_restatement_invalid_label_rule():
    """invalid pixels add nothing and get a zero gradient row; the focal mean keeps them in its denominator"""
    import _overlap_ref as R
    g = torch.Generator().manual_seed(5)
    x = torch.randn(1, 8, 4, 6, generator=g, dtype=torch.float64)
    y = torch.randint(0, 8, (1, 4, 6), generator=g)
    bad = y.clone()
    bad[0, 1, 2], bad[0, 3, 0] = 9, -3
    keep = torch.ones(1, 4, 6, dtype=torch.bool)
    keep[0, 1, 2] = keep[0, 3, 0] = False
    for name, cfg in (("SoftIoU", {"experiment": 1}), ("GenDiceLoss", {"experiment": 1, "weights": "auto"})):
        l_bad, g_bad = R.loss_and_grad(name, cfg, x, bad, torch.float64)
        rows = x.permute(0, 2, 3, 1)[keep].t().reshape(1, 8, -1, 1)
        l_ref, _ = R.loss_and_grad(name, cfg, rows, y[keep].reshape(1, -1, 1), torch.float64)
        assert abs(float(l_bad) - float(l_ref)) < 1e-12
        assert float(g_bad[0, :, 1, 2].abs().max()) == 0.0 and float(g_bad[0, :, 3, 0].abs().max()) == 0.0
    l_bad, g_bad = R.loss_and_grad("FocalLoss", {"gamma": 2}, x, bad, torch.float64)
    terms = [float(R.focal_loss(x[:, :, i:i + 1, j:j + 1], y[:, i:i + 1, j:j + 1])) for i in range(4) for j in range(6) if keep[0, i, j]]
    assert abs(float(l_bad) - sum(terms) / 24) < 1e-12
    assert float(g_bad[0, :, 1, 2].abs().max()) == 0.0
