"""Frozen BatchNorm without a GPU: the host-side refusals of the `frozen` form of catseg_bn_backward (fake aligned pointers: validation returns
before anything is launched), engine.freeze_bn's selections on CPU-constructed networks, the config key through every constructor, and
dist.sync_bn_stats leaving frozen modules out (the world-2 gloo harness of tests/test_dist_cpu.py)."""
import ctypes
import os
import socket
import sys

import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EINVAL, EWORKSPACE = 1, 3                      # CATSEG_EINVAL, CATSEG_EWORKSPACE of include/catseg.h
ROWS, CH = 64, 64
A = [0x10000 * (i + 1) for i in range(24)]     # fake device pointers, 16-byte aligned


def _frozen_desc(**kw):
    """a catseg_bn_backward_desc that is valid in the frozen form (fp32 dy, no ReLU) but for the fields in kw"""
    from miccai2021_cataract_semantic_segmentation_amd._lib import lib
    f = dict(dz=A[0], lddz=CH, y=A[1], ldy=CH, rows=ROWS, C=CH, dgamma=A[4], dbeta=A[5], workspace=A[6],
             workspace_bytes=lib.catseg_bn_workspace(ROWS, CH), dy=A[7], lddy=CH, frozen=1, running_mean=A[17], running_var=A[18], eps=1e-5,
             scale=A[19])
    f.update(kw)
    return f


def _training_desc(**kw):
    """valid in the training form with an fp32 dy"""
    from miccai2021_cataract_semantic_segmentation_amd._lib import lib
    f = dict(dz=A[0], lddz=CH, y=A[1], ldy=CH, stats=A[2], gamma=A[3], rows=ROWS, C=CH, dgamma=A[4], dbeta=A[5], workspace=A[6],
             workspace_bytes=lib.catseg_bn_workspace(ROWS, CH), dy=A[7], lddy=CH)
    f.update(kw)
    return f


RECORDS = dict(g_record=A[8], y_record=A[9], dy_record=A[10])
FROZEN_DEFECTS = [
    ("frozen with partials", lambda: _frozen_desc(partials=A[13], n_blocks=2), b"frozen takes no partials"),
    ("frozen with dy_planes", lambda: _frozen_desc(dy=None, dy_planes=A[7], **RECORDS), b"not dy_planes"),
    ("frozen with dy_planes beside dy", lambda: _frozen_desc(dy_planes=A[16]), b"not dy_planes"),
    ("frozen with dy_h2_planes", lambda: _frozen_desc(dy=None, dy_h2_planes=A[7], dy_h2_scale=A[11], beta=A[12], **RECORDS), b"not dy_h2_planes"),
    ("frozen with dbias", lambda: _frozen_desc(dbias=A[14]), b"dbias"),
    ("frozen with stats", lambda: _frozen_desc(stats=A[2]), b"stats must be NULL"),
    ("frozen without running_mean", lambda: _frozen_desc(running_mean=None), b"frozen needs running_mean"),
    ("frozen without running_var", lambda: _frozen_desc(running_var=None), b"frozen needs running_mean"),
    ("frozen without scale", lambda: _frozen_desc(scale=None), b"frozen needs running_mean"),
    ("running_mean without frozen", lambda: _training_desc(running_mean=A[17]), b"belong to frozen"),
    ("running_var without frozen", lambda: _training_desc(running_var=A[18]), b"belong to frozen"),
    ("scale without frozen", lambda: _training_desc(scale=A[19]), b"belong to frozen"),
    ("eps without frozen", lambda: _training_desc(eps=1e-5), b"belong to frozen"),
    # the rules of the training form that a frozen call keeps
    ("frozen, relu without z, mask or beta", lambda: _frozen_desc(relu=1), b"relu needs z"),
    ("frozen, relu from beta with a residual branch", lambda: _frozen_desc(relu=1, beta=A[12], dres=A[14], lddres=CH), b"relu needs z"),
    ("frozen, mask together with z", lambda: _frozen_desc(relu=1, mask=A[14], z=A[15], ldz=CH), b"replaces z"),
    ("frozen, mask and C % 8 != 0", lambda: _frozen_desc(relu=1, mask=A[14], C=68, lddz=68, ldy=68, lddy=68), b"multiples of 4"),
    ("frozen, g_record with the fp32 output", lambda: _frozen_desc(g_record=A[8]), b"dy takes dy_record alone"),
    ("frozen, no output", lambda: _frozen_desc(dy=None), b"exactly one"),
    ("frozen, ld of dy % 4 != 0", lambda: _frozen_desc(lddy=66), b"multiples of 4"),
    ("frozen, misaligned running_mean", lambda: _frozen_desc(running_mean=A[17] + 4), b"alignment"),
    ("frozen, misaligned scale", lambda: _frozen_desc(scale=A[19] + 8), b"alignment"),
    ("frozen, no dz", lambda: _frozen_desc(dz=None), b"required"),
]


@pytest.mark.parametrize("what,fields,message", FROZEN_DEFECTS, ids=[c[0] for c in FROZEN_DEFECTS])
def test_bn_backward_frozen_rejects_one_defect(what, fields, message):
    from miccai2021_cataract_semantic_segmentation_amd import _lib
    rc = _lib.lib.catseg_bn_backward(ctypes.byref(_lib.BnBackwardDesc(**fields())), None)
    err = _lib.lib.catseg_last_error()
    assert rc == EINVAL and err.startswith(b"catseg_bn_backward:") and message in err, (what, rc, err)


def test_bn_backward_frozen_workspace_too_small():
    """catseg_bn_workspace(rows, C) suffices (a valid descriptor with it would launch: not tried here); one byte less is EWORKSPACE"""
    from miccai2021_cataract_semantic_segmentation_amd import _lib
    lib = _lib.lib
    need = lib.catseg_bn_workspace(ROWS, CH)
    for fields in (_frozen_desc(workspace_bytes=need - 1), _frozen_desc(workspace=None)):
        rc = lib.catseg_bn_backward(ctypes.byref(_lib.BnBackwardDesc(**fields)), None)
        err = lib.catseg_last_error()
        assert rc == EWORKSPACE and err.startswith(b"catseg_bn_backward:") and b"workspace too small" in err, (rc, err)


def test_descriptor_mirror_ends_with_the_frozen_fields():
    from miccai2021_cataract_semantic_segmentation_amd import _lib
    assert [f[0] for f in _lib.BnBackwardDesc._fields_][-5:] == ["frozen", "running_mean", "running_var", "eps", "scale"]
    assert _lib.lib.catseg_version() == 3                     # appended fields: no new entry point, no version bump


# ---------------------------------------------------------------------------------------------------------------- freeze_bn
OCR_CFG = {"backbone": "resnet50", "out_stride": 8, "pretrained": False}
ENCDEC_CFG = {"encoder": {"model": "ResNet18"}, "decoder": {"model": "UPerNet"}}


def _encdec_cfg(**kw):
    return dict({k: dict(v) for k, v in ENCDEC_CFG.items()}, **kw)


def _bn_names(model):
    from miccai2021_cataract_semantic_segmentation_amd import engine
    return [n for n, m in model.named_modules() if isinstance(m, engine.BatchNorm2d)]


@pytest.fixture(scope="module")
def ocrnet():
    from miccai2021_cataract_semantic_segmentation_amd.models import OCRNet
    return OCRNet(dict(OCR_CFG), 3)


@pytest.fixture(scope="module")
def encdec():
    from miccai2021_cataract_semantic_segmentation_amd.models import EncDec
    return EncDec(_encdec_cfg(), 2)


def _unfreeze(model):
    from miccai2021_cataract_semantic_segmentation_amd import engine
    for m in model.modules():
        if isinstance(m, engine.BatchNorm2d):
            m.__dict__.pop("frozen", None)


def test_frozen_defaults_to_false_and_nothing_is_selected_by_false_or_none(ocrnet):
    from miccai2021_cataract_semantic_segmentation_amd import engine
    assert engine.BatchNorm2d.frozen is False and ocrnet.frozen_bn == []
    for select in (False, None):
        assert engine.freeze_bn(ocrnet, select) == []
    assert engine.frozen_bn_names(ocrnet) == []


def test_selections_on_ocrnet_resnet50(ocrnet):
    from miccai2021_cataract_semantic_segmentation_amd import engine
    names = _bn_names(ocrnet)
    backbone = [n for n in names if n.startswith("backbone.")]
    assert len(names) == 62 and len(backbone) == 53           # ResNet50: 1 + 16 x 3 + 4 downsample; 9 in the OCR head
    try:
        for select in (True, "all"):
            assert engine.freeze_bn(ocrnet, select) == names == engine.frozen_bn_names(ocrnet)
            _unfreeze(ocrnet)
        assert engine.freeze_bn(ocrnet, "backbone") == backbone == engine.frozen_bn_names(ocrnet)
        _unfreeze(ocrnet)
        assert engine.freeze_bn(ocrnet, ["backbone.layer1.0.bn1"]) == ["backbone.layer1.0.bn1"]
        _unfreeze(ocrnet)
        # a prefix names a module, not a string prefix: layer1 does not take a (hypothetical) layer10, "backbone.layer1.0.bn" takes nothing
        got = engine.freeze_bn(ocrnet, ("backbone.layer1", "conv_high_map"))
        assert got == [n for n in names if n.startswith("backbone.layer1.") or n.startswith("conv_high_map.")] and len(got) == 10 + 1
        _unfreeze(ocrnet)
        with pytest.raises(ValueError, match=r"backbone\.layer1\.0\.bn'"):
            engine.freeze_bn(ocrnet, ["backbone.layer1.0.bn"])
        # train() / eval() leave the attribute alone
        engine.freeze_bn(ocrnet, ["backbone.layer1.0.bn2"])
        ocrnet.eval()
        assert engine.frozen_bn_names(ocrnet) == ["backbone.layer1.0.bn2"]
        ocrnet.train()
        assert engine.frozen_bn_names(ocrnet) == ["backbone.layer1.0.bn2"] and ocrnet.backbone["layer1"][0].bn2.training
    finally:
        _unfreeze(ocrnet)


def test_selections_on_encdec_resnet18(encdec):
    from miccai2021_cataract_semantic_segmentation_amd import engine
    names = _bn_names(encdec)
    trunk = [n for n in names if n.startswith("enc_model.")]
    assert len(names) == 32 and len(trunk) == 20              # ResNet18: 1 + 8 x 2 + 3 downsample; 12 in UPerNet
    try:
        assert engine.freeze_bn(encdec, "all") == names
        _unfreeze(encdec)
        assert engine.freeze_bn(encdec, "backbone") == trunk   # (EncDec names its trunk enc_model: backbone_modules)
        _unfreeze(encdec)
        assert engine.freeze_bn(encdec, ["enc_model.layer1.0.bn1"]) == ["enc_model.layer1.0.bn1"]
        _unfreeze(encdec)
        with pytest.raises(ValueError, match="dec_model.nothing"):
            engine.freeze_bn(encdec, ["dec_model.nothing"])
        assert engine.frozen_bn_names(encdec) == []
    finally:
        _unfreeze(encdec)


@pytest.mark.parametrize("select", [1, 0, "trunk", "", 0.5, {"backbone": True}, ["backbone", 3], b"all"], ids=repr)
def test_other_selection_types_are_value_errors(ocrnet, select):
    from miccai2021_cataract_semantic_segmentation_amd import engine
    with pytest.raises(ValueError) as e:
        engine.freeze_bn(ocrnet, select)
    assert repr(select) in str(e.value) and engine.frozen_bn_names(ocrnet) == []


def test_config_key_through_every_constructor():
    from miccai2021_cataract_semantic_segmentation_amd import models
    r50 = {"backbone": "resnet50", "out_stride": 8, "pretrained": False}
    built = [
        (models.OCRNet(dict(r50, freeze_bn="backbone"), 3), 53, "backbone."),
        (models.DeepLabv3Plus(dict(r50, freeze_bn="backbone"), 2), 53, "backbone."),
        (models.DeepLabv3(dict(r50, freeze_bn="backbone"), 2), 53, "backbone."),
        (models.EncDec(_encdec_cfg(freeze_bn="backbone"), 2), 20, "enc_model."),
        (models.HRNetv2({"freeze_bn": ["stage2"]}, 3), None, "stage2."),
    ]
    for m, count, prefix in built:
        assert m.frozen_bn and all(n.startswith(prefix) for n in m.frozen_bn), type(m).__name__
        assert count is None or len(m.frozen_bn) == count, (type(m).__name__, len(m.frozen_bn))
        mods = dict(m.named_modules())
        assert all(mods[n].frozen for n in m.frozen_bn) and sum(getattr(x, "frozen", False) for x in mods.values()) == len(m.frozen_bn)
    every = models.HRNetv2({"freeze_bn": True}, 3)
    assert every.frozen_bn == _bn_names(every)
    assert models.OCRNet(dict(r50), 3).frozen_bn == [] and models.OCRNet(dict(r50, freeze_bn=False), 3).frozen_bn == []
    # the state-dict keys do not know about the attribute
    assert list(models.OCRNet(dict(r50, freeze_bn="all"), 3).state_dict()) == list(models.OCRNet(dict(r50), 3).state_dict())
    # a network without BatchNorm, and a trunk-less one asked for its "backbone", match nothing
    for build in (lambda: models.FCN({"width": 0.25, "freeze_bn": "all"}, 2), lambda: models.UNet({"freeze_bn": True}, 2),
                  lambda: models.HRNetv2({"freeze_bn": "backbone"}, 3)):
        with pytest.raises(ValueError, match="matches no BatchNorm"):
            build()
    with pytest.raises(ValueError, match="'trunk'"):
        models.OCRNet(dict(r50, freeze_bn="trunk"), 3)


# ------------------------------------------------------------------------------------------------------------ sync_bn_stats
def _sync_worker(rank, world, port, out):
    sys.path.insert(0, ROOT)
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    from miccai2021_cataract_semantic_segmentation_amd import dist as D, engine

    class _M(torch.nn.Module):
        def __init__(self):
            super().__init__()
            self.a, self.b, self.c = engine.BatchNorm2d(4), engine.BatchNorm2d(3), engine.BatchNorm2d(2)
    for how in ("mean", "rank0"):
        m = _M()
        for i, bn in enumerate((m.a, m.b, m.c)):
            bn.running_mean.fill_(float(rank) + 0.125 * i)       # (per-rank values even in the frozen module: it must keep them)
            bn.running_var.fill_(1.0 + rank)
            bn.num_batches_tracked.fill_(7 + rank)
        assert engine.freeze_bn(m, ["b"]) == ["b"]
        before = [t.clone() for t in (m.b.running_mean, m.b.running_var, m.b.num_batches_tracked)]
        D.sync_bn_stats(m, how)
        assert all(torch.equal(x, y) for x, y in zip(before, (m.b.running_mean, m.b.running_var, m.b.num_batches_tracked))), "frozen statistics moved"
        if how == "mean":
            assert torch.allclose(m.a.running_mean, torch.full((4,), 0.5)) and torch.allclose(m.a.running_var, torch.full((4,), 1.75))
            assert torch.allclose(m.c.running_mean, torch.full((2,), 0.75)) and torch.allclose(m.c.running_var, torch.full((2,), 1.75))
        else:
            assert torch.equal(m.a.running_mean, torch.zeros(4)) and torch.equal(m.c.running_mean, torch.full((2,), 0.25))
        # every BatchNorm frozen: nothing to exchange (and no collective that the other rank would wait in)
        engine.freeze_bn(m, "all")
        kept = m.a.running_mean.clone()
        D.sync_bn_stats(m, how)
        assert torch.equal(m.a.running_mean, kept)
    open(os.path.join(out, "ok%d" % rank), "w").close()
    dist.destroy_process_group()


def test_sync_bn_stats_skips_frozen_modules_gloo_world2(tmp_path):
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    mp.spawn(_sync_worker, args=(2, port, str(tmp_path)), nprocs=2, join=True)
    assert (tmp_path / "ok0").exists() and (tmp_path / "ok1").exists()
