"""Host side of semi-supervised training: the constructor contract of losses.SemiSupervisedLoss (losses/SemiSupervisedLoss.py:8-43 of the
reference), the batch split and its one-pass gradient join, utils.BalancedConcatDataset and the pseudo_colorjitter arguments against what
the REAL reference produced (tests/golden/semisup.npz, written by tests/golden/make_golden_semisup.py), the RandomApply draw of
sample_color_jitter, the host validation of a per-frame label-table index, and the C ABI of include/catseg_ingest_tables.h."""
import copy
import ctypes

import numpy as np
import pytest
import torch

import _abi


def _cfg(name="LovaszSoftmax", **kw):
    c = {"experiment": 2, "labeled": {"name": name}, "unlabeled": {"name": name}}
    c.update(kw)
    return c


# ---- constructor
def test_constructor_copies_the_experiment_into_both_sub_configs_and_defaults_the_weights():
    from miccai2021_cataract_semantic_segmentation_amd.losses import LovaszSoftmax, SemiSupervisedLoss
    cfg = _cfg()
    crit = SemiSupervisedLoss(cfg)
    assert cfg["labeled"]["experiment"] == 2 and cfg["unlabeled"]["experiment"] == 2          # the reference mutates its config (:25-26)
    assert crit.w_lab == 1.0 and crit.w_ulab == 1.0 and crit.ignore_label == 17
    assert isinstance(crit.loss_lab, LovaszSoftmax) and isinstance(crit.loss_ulab, LovaszSoftmax) and crit.loss_lab is not crit.loss_ulab
    crit = SemiSupervisedLoss({"experiment": 1, "labeled": {"name": "OhemCrossEntropy", "weight": 0.3, "min_kept": 7},
                               "unlabeled": {"name": "OhemCrossEntropy", "weight": 2, "min_kept": 9}})
    assert (crit.w_lab, crit.w_ulab, crit.ignore_label) == (0.3, 2, -100)
    assert (crit.loss_lab.min_kept, crit.loss_ulab.min_kept) == (7, 9)                        # each half's own sub-config


def test_constructor_builds_a_two_scale_pair():
    from miccai2021_cataract_semantic_segmentation_amd.losses import SemiSupervisedLoss, TwoScaleLoss

    def two(final_weight):
        return {"name": "TwoScaleLoss", "interm": {"name": "LovaszSoftmax", "args": [], "weight": 0.4},
                "final": {"name": "LovaszSoftmax", "args": [], "weight": final_weight}}
    cfg = {"experiment": 3, "labeled": two(1.0), "unlabeled": dict(two(0.7), weight=0.5)}
    crit = SemiSupervisedLoss(cfg)
    assert isinstance(crit.loss_lab, TwoScaleLoss) and (crit.loss_lab.w_final, crit.loss_ulab.w_final) == (1.0, 0.7)
    assert cfg["unlabeled"]["final"]["experiment"] == 3 and crit.w_ulab == 0.5


def test_constructor_needs_the_experiment():
    from miccai2021_cataract_semantic_segmentation_amd.losses import SemiSupervisedLoss
    cfg = _cfg()
    del cfg["experiment"]
    with pytest.raises(KeyError, match="experiment"):
        SemiSupervisedLoss(cfg)


def test_constructor_refuses_different_inner_losses_with_the_reference_message():
    from miccai2021_cataract_semantic_segmentation_amd.losses import SemiSupervisedLoss
    cfg = {"experiment": 2, "labeled": {"name": "LovaszSoftmax"}, "unlabeled": {"name": "OhemCrossEntropy"}}
    after = copy.deepcopy(cfg)
    after["labeled"]["experiment"] = after["unlabeled"]["experiment"] = 2
    with pytest.raises(NotImplementedError) as e:
        SemiSupervisedLoss(cfg)
    assert str(e.value) == "different losses for labeled {} and unlabeled {}".format(after["labeled"], after["unlabeled"])


def test_constructor_refuses_cross_entropy_with_a_reason_and_unknown_names_as_the_reference():
    from miccai2021_cataract_semantic_segmentation_amd.losses import SemiSupervisedLoss
    with pytest.raises(NotImplementedError, match="CrossEntropy.*TypeError"):
        SemiSupervisedLoss(_cfg("CrossEntropy"))
    with pytest.raises(KeyError):                                   # globals()[name] of the reference
        SemiSupervisedLoss(_cfg("FocalLoss"))


def test_forward_refuses_other_inputs_before_any_kernel():
    from miccai2021_cataract_semantic_segmentation_amd.losses import SemiSupervisedLoss
    crit = SemiSupervisedLoss(_cfg())
    t = torch.zeros(2, 17, 4, 4)
    lbl = torch.zeros(2, 4, 4, dtype=torch.long)
    with pytest.raises(NotImplementedError, match="only two scales"):
        crit([t, t, t], lbl)
    with pytest.raises(ValueError, match="either torch.tensor or a list"):
        crit((t, t), lbl)
    with pytest.raises(AssertionError, match="batch_size must be great or equal of 2 instead got 1"):
        crit(t[:1], lbl[:1])
    with pytest.raises(AssertionError, match="instead got 1"):
        crit([t[:1], t[:1]], lbl[:1])
    with pytest.raises(RuntimeError, match="no CPU fallback"):     # the halves reach the HIP losses: host tensors are an error, not a fallback
        crit(t, lbl)


# ---- the split and its gradient join (pure torch: runs on the host)
@pytest.mark.parametrize("B", [2, 3, 4, 5])
@pytest.mark.parametrize("channels_last", [False, True])
def test_split_batch_halves_are_views_and_the_joined_gradient_is_torchs(B, channels_last):
    from miccai2021_cataract_semantic_segmentation_amd.losses.semi import split_batch
    g = torch.Generator().manual_seed(B)
    x = torch.randn(B, 5, 3, 7, generator=g)
    if channels_last:
        x = x.permute(0, 2, 3, 1).contiguous().permute(0, 3, 1, 2)      # NCHW view of NHWC storage, as the engine's logits
    a, b = torch.randn(B // 2, 5, 3, 7, generator=g), torch.randn(B - B // 2, 5, 3, 7, generator=g)
    ref = x.clone().requires_grad_()
    ((ref[:B // 2] * a).sum() * 0.5 + (ref[B // 2:] * b).sum() * 2.0).backward()
    x.requires_grad_()
    lab, ulab = split_batch(x)
    assert lab.shape[0] == B // 2 and ulab.shape[0] == B - B // 2                    # odd B: the extra frame is pseudo-labelled
    assert lab.data_ptr() == x.data_ptr() and ulab.data_ptr() == x.data_ptr() + x.stride(0) * (B // 2) * 4      # views, not copies
    if channels_last:
        assert lab.permute(0, 2, 3, 1).is_contiguous() and ulab.permute(0, 2, 3, 1).is_contiguous()            # what as_pixel_rows takes in place
    ((lab * a).sum() * 0.5 + (ulab * b).sum() * 2.0).backward()
    assert torch.equal(x.grad, ref.grad)
    assert x.grad.stride() == x.stride()
    # a half that takes no part in the loss: zeros, not garbage
    y = x.detach().clone().requires_grad_()
    lab, ulab = split_batch(y)
    (ulab * b).sum().backward()
    assert torch.equal(y.grad[:B // 2], torch.zeros_like(y.grad[:B // 2])) and torch.equal(y.grad[B // 2:], b)
    # labels (no gradient): plain slices
    t = torch.arange(B)
    assert [v.tolist() for v in split_batch(t)] == [list(range(B // 2)), list(range(B // 2, B))]


def test_fixture_targets_tell_a_wrong_split(golden):
    """what the cases above rely on: a class only the labelled half holds, one only the pseudo half holds (at B = 4 and B = 3), an empty
    class, ignore-labelled pixels where the experiment has an ignore id; halves of 1728 / 864 pixels (no multiple of 256)"""
    g = golden("semisup")
    for name, K, ignore in (("lovasz_e2", 17, 17), ("lovasz_e1", 8, None), ("ohem_e3", 25, 25), ("two_scale_e2", 17, 17)):
        t = g[name + "_target"]
        assert t.shape == (4, 24, 36) and g[name + "_logits_q"].shape == (4, K, 24, 36)
        for B in (4, 3):
            lab, ulab = set(t[:B // 2].ravel().tolist()), set(t[B // 2:B].ravel().tolist())
            assert 2 in lab and 2 not in ulab and 5 in ulab and 5 not in lab and 6 not in lab | ulab
            assert ignore is None or (ignore in lab and ignore in ulab)
            assert max(lab | ulab) == (ignore if ignore is not None else K - 1)
    assert (2 * 24 * 36) % 256 != 0 and (24 * 36) % 256 != 0


# ---- data side against the reference's records
def test_balanced_concat_dataset_against_the_reference(golden):
    from miccai2021_cataract_semantic_segmentation_amd.utils import BalancedConcatDataset
    g = golden("semisup")
    ds = BalancedConcatDataset(list(range(5)), list(range(100, 107)))
    assert len(ds) == int(g["concat_len"]) == 7 and (ds.max_len, ds.min_len) == (7, 5)
    items = [ds[i] for i in range(len(ds))]
    assert all(isinstance(it, tuple) and len(it) == 2 for it in items)
    assert np.array_equal(np.array(items), g["concat_items"])
    three = BalancedConcatDataset([0, 1], [10, 11, 12], [20])
    assert len(three) == 3 and three[2] == (0, 12, 20)


@pytest.mark.parametrize("strength", [1, 2, 3, None])
def test_pseudo_jitter_ranges_against_the_reference(golden, strength):
    from miccai2021_cataract_semantic_segmentation_amd.utils import augment
    want = golden("semisup")["jitter_s%s" % ("default" if strength is None else strength)]
    got = augment.pseudo_jitter_ranges(strength) if strength is not None else augment.pseudo_jitter_ranges()
    rows = np.array([got["brightness"], got["contrast"], got["saturation"], got["hue"]], dtype=np.float64)
    assert np.array_equal(rows, want[:4])                      # the same float64 values: the same expressions
    assert augment.PSEUDO_JITTER_PROBABILITY == want[4, 0] == 0.7
    if strength is None:
        assert np.array_equal(want, golden("semisup")["jitter_s2"])
    with pytest.raises(AssertionError):
        augment.pseudo_jitter_ranges(4)
    # the keyword scan of utils/utils.py:421-429, with the lists make_golden_semisup.py handed to parse_transform_list
    tl = ["pseudo_colorjitter"] + ([{"strength": strength}] if strength is not None else [])
    assert augment.pseudo_jitter_strength(tl) == (2 if strength is None else strength)
    assert augment.pseudo_jitter_strength(["pad", "flip", {"strength": 3}]) is None
    with pytest.raises(AssertionError):
        augment.pseudo_jitter_strength(["pseudo_colorjitter", {"strength": 0}])


def test_sample_color_jitter_random_apply_draws_first_and_skips_with_order_minus_one():
    from miccai2021_cataract_semantic_segmentation_amd.utils.augment import pseudo_jitter_ranges, sample_color_jitter
    rng = pseudo_jitter_ranges(3)
    orders, factors = sample_color_jitter(24, generator=torch.Generator().manual_seed(7), apply_probability=0.7, **rng)
    gen = torch.Generator().manual_seed(7)                    # the same stream, drawn by hand in RandomApply's / get_params' order
    skipped = 0
    for i in range(24):
        if 0.7 < float(torch.rand(1, generator=gen)):        # RandomApply.forward: `if self.p < torch.rand(1): return img`
            assert orders[i].tolist() == [-1] * 4 and factors[i].tolist() == [0.0] * 4       # nothing else is drawn for a skipped frame
            skipped += 1
            continue
        assert orders[i].tolist() == torch.randperm(4, generator=gen).tolist()
        for k, name in enumerate(("brightness", "contrast", "saturation", "hue")):
            lo, hi = rng[name]
            assert factors[i, k] == float(torch.empty(1).uniform_(lo, hi, generator=gen)) and lo <= factors[i, k] <= hi
    assert 0 < skipped < 24
    # without the probability nothing changes: no extra draw, no skipped frame
    a = sample_color_jitter(6, generator=torch.Generator().manual_seed(3))
    gen = torch.Generator().manual_seed(3)
    assert a[0][0].tolist() == torch.randperm(4, generator=gen).tolist() and (a[0] >= 0).all()
    # the extremes
    assert (sample_color_jitter(5, generator=torch.Generator().manual_seed(1), apply_probability=0.0)[0] == -1).all()
    assert (sample_color_jitter(5, generator=torch.Generator().manual_seed(1), apply_probability=1.0)[0] >= 0).all()


# ---- label tables
def test_label_tables_rows_and_host_validation():
    from miccai2021_cataract_semantic_segmentation_amd.utils import check_label_tables, label_tables_of, remap_lut
    for exp in (1, 2, 3):
        t = label_tables_of(exp)
        assert t.dtype == np.uint8 and t.shape == (2, 256)
        assert np.array_equal(t[0], remap_lut(exp)) and np.array_equal(t[1], np.arange(256))
    got = check_label_tables([0, 0, 1, 1], 4)
    assert got.dtype == np.int32 and got.flags["C_CONTIGUOUS"] and got.tolist() == [0, 0, 1, 1]
    assert check_label_tables(np.array([1, 0, 1], dtype=np.int64), 3).tolist() == [1, 0, 1]
    assert check_label_tables([2, 0], 2, tables=3).tolist() == [2, 0]
    for bad, batch, msg in (([0, 2, 1, 0], 4, r"\[0, 2\)"), ([0, -1], 2, r"\[0, 2\)"), ([0, 1, 1], 4, "one table row per frame"),
                            ([[0, 1]], 2, "one table row per frame"), ([0.0, 1.0], 2, "integers"), ([True, False], 2, "integers")):
        with pytest.raises(ValueError, match=msg):
            check_label_tables(bad, batch)


def test_loader_refuses_paired_datasets_it_cannot_lay_out():
    from miccai2021_cataract_semantic_segmentation_amd.utils import BalancedConcatDataset
    from miccai2021_cataract_semantic_segmentation_amd.utils.loader import PinnedFrameLoader
    pair = BalancedConcatDataset([0] * 5, [0] * 6)
    for ds, kw, msg in ((pair, dict(batch_size=4), "labels_remapped"), (pair, dict(batch_size=4, labels_remapped=(True, False)), "labels_remapped"),
                        (pair, dict(batch_size=3, labels_remapped=(False, True)), "even batch_size"),
                        ([0] * 5, dict(batch_size=4, labels_remapped=(False, True)), "BalancedConcatDataset"),
                        (BalancedConcatDataset([0], [0], [0]), dict(batch_size=4, labels_remapped=(False, True)), "two members")):
        with pytest.raises(ValueError, match=msg):
            PinnedFrameLoader(ds, experiment=2, **kw)


def test_manager_batch_unpacking_and_the_encdec_refusal():
    from miccai2021_cataract_semantic_segmentation_amd.managers.base import unpack_batch
    from miccai2021_cataract_semantic_segmentation_amd.managers import EncDecManager
    img, lbl = torch.zeros(2, 3, 4, 4), torch.zeros(2, 4, 4, dtype=torch.long)
    a, b = unpack_batch([img, lbl, {"index": torch.tensor([0, 1])}])
    assert a is img and b is lbl
    a, b = unpack_batch([[img, lbl, {}], [img + 1, lbl + 1, {}]])        # torch's collation of BalancedConcatDataset items
    assert a.shape[0] == 4 and torch.equal(a[2:], img + 1) and torch.equal(b, torch.cat([lbl, lbl + 1]))
    with pytest.raises(ValueError):
        unpack_batch([img, lbl])
    m = EncDecManager.__new__(EncDecManager)                               # load_loss alone: constructing a manager needs the device
    m.config, m.experiment, m.device = {"loss": {"name": "SemiSupervisedLoss"}}, 2, "cuda:0"
    with pytest.raises(NotImplementedError, match="LossWrapper"):
        m.load_loss()


# ---- the C ABI of include/catseg_ingest_tables.h
EINVAL = 1
A = [0x10000 * (i + 1) for i in range(16)]     # fake device pointers: a refusal returns before anything is launched


def test_tables_signature_table_matches_the_header_and_the_plain_prototypes():
    from miccai2021_cataract_semantic_segmentation_amd import _lib
    tables = _abi.prototypes("catseg_ingest_tables.h")
    assert sorted(tables) == ["catseg_crop_freq_pick_tables", "catseg_ingest_u8_tables", "catseg_ingest_warp_u8_tables"]
    lib = ctypes.CDLL(_lib.LIB_PATH)
    plain = set(_abi.prototypes("catseg.h")) | set(_abi.prototypes("catseg_cropfreq.h"))
    for name, (res, args, names) in tables.items():
        assert hasattr(lib, name), "libcatseg_hip.so does not export %s" % name
        assert _lib._SIGS[name] == (res, args), "%s: header %r, _lib._SIGS %r" % (name, (res, args), _lib._SIGS[name])
        # the plain entry point's arguments with (T, table_of_frame) after the tables, nothing else moved
        i = names.index("luts")
        assert names[i:i + 3] == ["luts", "T", "table_of_frame"] and args[i + 1:i + 3] == [ctypes.c_int, ctypes.c_void_p]
        base = name[:-len("_tables")]
        assert base in plain and (res, args[:i + 1] + args[i + 3:]) == _lib._SIGS[base]
    # the existing entry points kept their signatures
    assert _lib._SIGS["catseg_ingest_u8"][1] == [ctypes.c_void_p] * 2 + [ctypes.c_int] * 3 + [ctypes.c_void_p] * 2 + [ctypes.c_int] * 2 + [ctypes.c_void_p] * 6


def _ingest_args(**kw):
    f = dict(img=A[0], lbl=A[1], B=2, H=20, W=28, luts=A[2], T=2, table_of_frame=A[3], flips=A[4], pad_top=2, pad_bottom=2, mean=None,
             stdv=None, x_nchw=A[5], x_nhwc4=None, labels=A[6], stream=None)
    f.update(kw)
    return tuple(f.values())


def _warp_args(**kw):
    f = dict(img=A[0], lbl=A[1], B=2, H=20, W=28, luts=A[2], T=2, table_of_frame=A[3], flips=A[4], minv=A[5], Hc=40, Wc=56, origin=A[6], Hw=16,
             Ww=16, pad_top=0, pad_bottom=0, mean=None, stdv=None, x_nchw=A[7], x_nhwc4=None, x_u8=None, labels=A[8], stream=None)
    f.update(kw)
    return tuple(f.values())


def _pick_args(**kw):
    f = dict(lbl=A[0], B=2, H=20, W=28, luts=A[1], T=2, table_of_frame=A[2], flips=A[3], minv=A[4], Hc=40, Wc=56, px=16, wq=A[5], m53=A[6],
             origin=A[7], total=A[8], flat=A[9], workspace=A[10], workspace_bytes=2 * 24 * 8, stream=None)
    f.update(kw)
    return tuple(f.values())


TABLE_DEFECTS = [
    ("ingest: no table", "catseg_ingest_u8_tables", _ingest_args(T=0), b"T >= 1"),
    ("ingest: an index without tables", "catseg_ingest_u8_tables", _ingest_args(luts=None), b"T >= 1"),
    ("ingest: a misaligned index", "catseg_ingest_u8_tables", _ingest_args(table_of_frame=A[3] + 2), b"4-byte aligned"),
    ("ingest: the plain entry's rules hold", "catseg_ingest_u8_tables", _ingest_args(pad_top=20), b"reflect padding"),
    ("warp: no table", "catseg_ingest_warp_u8_tables", _warp_args(T=-1), b"T >= 1"),
    ("warp: an index without tables", "catseg_ingest_warp_u8_tables", _warp_args(luts=None), b"T >= 1"),
    ("warp: a misaligned index", "catseg_ingest_warp_u8_tables", _warp_args(table_of_frame=A[3] + 1), b"4-byte aligned"),
    ("warp: the plain entry's rules hold", "catseg_ingest_warp_u8_tables", _warp_args(Hw=41), b"must fit into the canvas"),
    ("pick: no table", "catseg_crop_freq_pick_tables", _pick_args(T=0), b"T >= 1"),
    ("pick: an index without tables", "catseg_crop_freq_pick_tables", _pick_args(luts=None), b"T >= 1"),
    ("pick: a misaligned index", "catseg_crop_freq_pick_tables", _pick_args(table_of_frame=A[2] + 2), b"4-byte aligned"),
    ("pick: the plain entry's rules hold", "catseg_crop_freq_pick_tables", _pick_args(px=41), b"px outside the canvas"),
]


@pytest.mark.parametrize("what,entry,args,message", TABLE_DEFECTS, ids=[c[0] for c in TABLE_DEFECTS])
def test_tables_entry_points_refuse_one_defect_before_a_launch(what, entry, args, message):
    from miccai2021_cataract_semantic_segmentation_amd import _lib
    rc = getattr(_lib.lib, entry)(*args)
    err = _lib.lib.catseg_last_error()
    assert rc == EINVAL and message in err, (what, rc, err)
