"""Semi-supervised training on the device: losses.SemiSupervisedLoss against the REAL reference's losses and gradients (tests/golden/
semisup*.npz, written by tests/golden/make_golden_semisup.py), its composition of the inner losses bit for bit, the captured step, mixed
labelled / pseudo-labelled batches through the three ingest launches, and OCRNetManager's pseudo_label / epoch / validate with such a loss.

Bars of the fixture cases: those tests/test_contract_gpu.py holds the inner losses to against the reference -- loss within
3e-6 max(1, |loss|), gradients atol 3e-7 / rtol 2e-4, OHEM with the identical set of pixels that receive gradient."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

T = torch.from_numpy


def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")


def _dev(t, channels_last=True):
    """NCHW logits on the device; channels_last: an NCHW view of NHWC storage, the engine's layout"""
    t = t.cuda()
    if channels_last:
        t = t.permute(0, 2, 3, 1).contiguous().permute(0, 3, 1, 2)
    return t.requires_grad_()


def _lovasz(exp, w_lab, w_ulab, **extra):
    return {"experiment": exp, "labeled": dict({"name": "LovaszSoftmax", "weight": w_lab}, **extra),
            "unlabeled": dict({"name": "LovaszSoftmax", "weight": w_ulab}, **extra)}


def _two_scale(final_weight, weight):
    return {"name": "TwoScaleLoss", "weight": weight, "interm": {"name": "LovaszSoftmax", "args": [], "weight": 0.4},
            "final": {"name": "LovaszSoftmax", "args": [], "weight": final_weight}}


def _ohem(exp):
    return {"experiment": exp, "labeled": {"name": "OhemCrossEntropy", "weight": 1.0, "min_kept": 200, "thresh": 0.004},
            "unlabeled": {"name": "OhemCrossEntropy", "weight": 0.25, "min_kept": 200, "thresh": 0.004}}


# the configurations tests/golden/make_golden_semisup.py ran the reference with
FIXTURE = {"lovasz_e2": (lambda: _lovasz(2, 1.0, 0.5), False), "lovasz_e1": (lambda: _lovasz(1, 0.75, 1.5), False),
           "ohem_e3": (lambda: _ohem(3), False),
           "two_scale_e2": (lambda: {"experiment": 2, "labeled": _two_scale(1.0, 1.0), "unlabeled": _two_scale(0.7, 0.5)}, True)}
FIXTURE_CASES = [("lovasz_e2", 4), ("lovasz_e2", 3), ("lovasz_e1", 4), ("lovasz_e1", 3), ("ohem_e3", 4), ("two_scale_e2", 4)]


@pytest.mark.parametrize("flag", [False, True], ids=["train", "valid"])
@pytest.mark.parametrize("name,B", FIXTURE_CASES, ids=["%s_b%d" % c for c in FIXTURE_CASES])
def test_loss_and_gradients_against_the_reference(golden, name, B, flag):
    _need_gpu()
    from miccai2021_cataract_semantic_segmentation_amd.losses import SemiSupervisedLoss
    g, gg = golden("semisup"), golden("semisup_" + name)
    cfg, as_list = FIXTURE[name]
    final = _dev(T(g[name + "_logits_q"][:B]).float() / 16)
    interm = _dev(T(g[name + "_interm_q"][:B]).float() / 16) if as_list else None
    target = T(g[name + "_target"][:B]).long().cuda()
    tag = "%s_b%d_%s" % (name, B, "valid" if flag else "train")
    loss = SemiSupervisedLoss(cfg())([interm, final] if as_list else final, target, run_on_labeled_validation=flag)
    loss.backward()
    want = float(g[tag + "_loss"])
    print(tag, "loss", float(loss.detach()), "reference", want, "max |grad diff|", float((final.grad.cpu() - T(gg[tag + "_grad"])).abs().max()))
    assert abs(float(loss.detach()) - want) < 3e-6 * max(1.0, abs(want)), (float(loss.detach()), want)
    if name.startswith("ohem"):
        sel, ref_sel = final.grad.cpu().abs().sum(1) > 0, T(gg[tag + "_grad"]).abs().sum(1) > 0
        assert (sel != ref_sel).sum().item() == 0 and 0 < int(ref_sel.sum()) < ref_sel.numel()      # the same pixels receive gradient
    np.testing.assert_allclose(final.grad.cpu().numpy(), gg[tag + "_grad"], atol=3e-7, rtol=2e-4)
    if as_list:
        np.testing.assert_allclose(interm.grad.cpu().numpy(), gg[tag + "_ginterm"], atol=3e-7, rtol=2e-4)


# ---- composition
def _inner_reference(crit, logits, target, as_list):
    """w_lab inner(labelled half) + w_ulab inner(pseudo half) on contiguous COPIES of the halves; returns (loss, full gradients)"""
    B = target.shape[0]
    h = B // 2
    parts = [[_dev(x.detach()[s].clone()) for x in logits] for s in (slice(0, h), slice(h, B))]
    second = crit.loss_ulab if as_list else crit.loss_lab
    loss = crit.loss_lab(*parts[0], target[:h].clone()) * crit.w_lab + second(*parts[1], target[h:].clone()) * crit.w_ulab
    loss.backward()
    return loss, [torch.cat([parts[0][i].grad, parts[1][i].grad]) for i in range(len(logits))]


COMPOSE = {
    "lovasz": (lambda: _lovasz(2, 1.0, 0.5), False),
    "lovasz_per_image": (lambda: _lovasz(2, 0.8, 1.3, per_image=True), False),
    "ohem": (lambda: _ohem(2), False),
    "two_scale": (lambda: {"experiment": 2, "labeled": _two_scale(1.0, 1.0), "unlabeled": _two_scale(0.7, 0.5)}, True),
}


@pytest.mark.parametrize("channels_last", [True, False], ids=["nhwc", "nchw"])
@pytest.mark.parametrize("B", [2, 3, 4])
@pytest.mark.parametrize("form", sorted(COMPOSE))
def test_composition_is_bit_for_bit_the_inner_losses_on_copies_of_the_halves(form, B, channels_last):
    """the loss and the FULL logits gradient equal w_lab inner(lab) + w_ulab inner(ulab) evaluated on contiguous copies of the halves: the
    views reach the kernels unchanged, the joined gradient holds both halves' rows, and no workspace of the first term is reused by the
    second before backward has read it"""
    _need_gpu()
    from miccai2021_cataract_semantic_segmentation_amd.losses import SemiSupervisedLoss
    cfg, as_list = COMPOSE[form]
    gen = torch.Generator().manual_seed(10 * B + len(form))
    K, H, W = 17, 20, 28                                            # 560 pixels per frame: no multiple of 256; a half is 1, 1 | 2 or 2 frames
    target = torch.randint(0, K + 1, (B, H // 4, W // 4), generator=gen).repeat_interleave(4, 1).repeat_interleave(4, 2).cuda()
    final = _dev(torch.randn(B, K, H, W, generator=gen) * 2, channels_last)
    logits = [_dev(torch.randn(B, K, H // 2, W // 2, generator=gen) * 2, channels_last), final] if as_list else [final]
    crit = SemiSupervisedLoss(cfg())
    loss = crit(logits if as_list else final, target)
    loss.backward()
    want, grads = _inner_reference(crit, logits, target, as_list)
    assert float(loss.detach()) == float(want.detach()) and np.isfinite(float(loss.detach()))
    for x, gref in zip(logits, grads):
        assert torch.equal(x.grad, gref) and float(gref.abs().sum()) > 0
        assert float(x.grad[:B // 2].abs().sum()) > 0 and float(x.grad[B // 2:].abs().sum()) > 0
    # the validation form: the labelled loss on the whole batch, unweighted
    whole = [_dev(x.detach().clone(), channels_last) for x in logits]
    got = crit([w for w in whole] if as_list else whole[0], target, run_on_labeled_validation=True)
    assert float(got) == float(crit.loss_lab(*[w.detach() for w in whole], target))


# ---- the captured step
def test_three_graph_replays_equal_three_eager_steps():
    """OCRNet-ResNet50 at 4 x 3 x 64 x 96 with TwoScaleLoss(LovaszSoftmax) inside: parameters and losses bit for bit (nothing in the loss
    synchronises with the host, so the capture holds it)"""
    _need_gpu()
    import bench
    from miccai2021_cataract_semantic_segmentation_amd.graph import GraphedTrainStep
    from miccai2021_cataract_semantic_segmentation_amd.losses import SemiSupervisedLoss
    from miccai2021_cataract_semantic_segmentation_amd.models import OCRNet
    from miccai2021_cataract_semantic_segmentation_amd.optim import FusedAdam
    dev = torch.device("cuda")
    torch.manual_seed(0)
    model = OCRNet(dict(bench.MODELS["ocrnet_r50"][0]), 3).to(dev).train()
    crit = SemiSupervisedLoss({"experiment": 3, "labeled": _two_scale(1.0, 1.0), "unlabeled": _two_scale(0.7, 0.5)})
    opt = FusedAdam(model, lr=1e-3)
    batches = [bench.synth_batch(4, 64, 96, 25, 700 + i, dev) for i in range(3)]
    fp = model.flat()
    w0 = fp.flat.clone()
    bufs0 = [b.clone() for b in model.buffers()]
    losses_e = []
    for x, y in batches:
        opt.zero_grad()
        loss = crit(list(model(x)), y)
        loss.backward()
        opt.step()
        losses_e.append(float(loss.detach()))
    torch.cuda.synchronize()
    w_e = fp.flat.clone()
    with torch.no_grad():
        fp.flat.copy_(w0)
        opt._m.zero_()
        opt._v.zero_()
        for b, s in zip(model.buffers(), bufs0):
            b.copy_(s)
    opt._steps = 0
    step = GraphedTrainStep(model, lambda o, l: crit(list(o), l), opt, *batches[0])
    losses_g = [float(step(x, y)) for x, y in batches]
    torch.cuda.synchronize()
    step.release()
    assert losses_g == losses_e and all(np.isfinite(v) for v in losses_e)
    assert torch.equal(fp.flat, w_e) and not torch.equal(w_e, w0)


# ---- mixed batches through the ingest
FH, FW = 20, 28


def _frames(B, rows, seed):
    """raw uint8 frames and label maps: frames of table row 0 hold raw CaDIS ids (0 .. 35), frames of row 1 network ids of experiment 2"""
    g = torch.Generator().manual_seed(seed)
    img = torch.randint(0, 256, (B, FH, FW, 3), generator=g).to(torch.uint8)
    raw = torch.randint(0, 36, (B, FH, FW), generator=g)
    net = torch.randint(0, 18, (B, FH, FW), generator=g)
    lbl = torch.where(torch.tensor(rows).view(B, 1, 1) == 1, net, raw).to(torch.uint8)
    flips = torch.tensor([(3 * b + 1) % 4 for b in range(B)], dtype=torch.int32)
    return img.cuda(), lbl.cuda(), flips.cuda()


def _luts():
    from miccai2021_cataract_semantic_segmentation_amd.utils import label_tables_of
    luts = T(label_tables_of(2)).cuda()
    assert not torch.equal(luts[0], luts[1])
    return luts


def _mats(B, seed):
    """canvas -> frame matrices: a small rotation about the frame's centre on the 2H x 2W canvas"""
    rng = np.random.RandomState(seed)
    m = np.zeros((B, 3, 3))
    for b in range(B):
        a = rng.uniform(-0.3, 0.3)
        c, s = np.cos(a), np.sin(a)
        m[b] = [[c, -s, FW / 2 - c * FW + s * FH], [s, c, FH / 2 - s * FW - c * FH], [0, 0, 1]]
    return m


MIXED = [[0, 0, 1, 1], [1, 0, 1]]


@pytest.mark.parametrize("rows", MIXED, ids=["0011", "101"])
def test_mixed_plain_ingest_equals_the_two_launches_it_replaces(rows):
    _need_gpu()
    from miccai2021_cataract_semantic_segmentation_amd import ops
    B = len(rows)
    img, lbl, flips = _frames(B, rows, 11)
    luts = _luts()
    x, labels = ops.ingest_u8(img, lbl, luts, flips, 2, 2, tables=torch.tensor(rows, dtype=torch.int32).cuda())
    assert x.shape == (B, 3, FH + 4, FW) and labels.shape == (B, FH + 4, FW)
    for t in (0, 1):
        idx = torch.tensor([b for b in range(B) if rows[b] == t]).cuda()
        xt, lt = ops.ingest_u8(img[idx].contiguous(), lbl[idx].contiguous(), luts[t].contiguous(), flips[idx].contiguous(), 2, 2)
        assert torch.equal(x[idx], xt) and torch.equal(labels[idx], lt)
    assert int(labels.max()) <= 17
    # a null index: row 0 for every frame = the existing entry point
    x0, l0 = ops.ingest_u8(img, lbl, luts, flips, 2, 2)
    xp, lp = ops.ingest_u8(img, lbl, luts[0].contiguous(), flips, 2, 2)
    assert torch.equal(x0, xp) and torch.equal(l0, lp) and not torch.equal(l0, labels)
    # an index outside [0, T) is clamped by the kernel
    wild = torch.tensor([7 if r else -3 for r in rows], dtype=torch.int32).cuda()
    assert torch.equal(ops.ingest_u8(None, lbl, luts, flips, 2, 2, tables=wild)[1], labels)


@pytest.mark.parametrize("rows", MIXED, ids=["0011", "101"])
def test_mixed_warp_ingest_equals_the_two_launches_it_replaces(rows):
    _need_gpu()
    from miccai2021_cataract_semantic_segmentation_amd import ops
    B = len(rows)
    img, lbl, flips = _frames(B, rows, 12)
    luts, minv = _luts(), _mats(B, 3)
    origin = np.array([[5 + 3 * b, 9 + 2 * b] for b in range(B)])
    kw = dict(canvas=(2 * FH, 2 * FW), window=(16, 16), outputs=("nchw", "u8"))
    out = ops.ingest_warp_u8(img, lbl, luts, flips, minv, origin=origin, tables=torch.tensor(rows, dtype=torch.int32).cuda(), **kw)
    assert out["labels"].shape == (B, 16, 16) and int((out["labels"] > 0).sum()) > 0
    for t in (0, 1):
        sel = [b for b in range(B) if rows[b] == t]
        idx = torch.tensor(sel).cuda()
        part = ops.ingest_warp_u8(img[idx].contiguous(), lbl[idx].contiguous(), luts[t].contiguous(), flips[idx].contiguous(), minv[sel],
                                  origin=origin[sel], **kw)
        for key in ("nchw", "u8", "labels"):
            assert torch.equal(out[key][idx], part[key]), key
    null = ops.ingest_warp_u8(img, lbl, luts, flips, minv, origin=origin, **kw)
    plain = ops.ingest_warp_u8(img, lbl, luts[0].contiguous(), flips, minv, origin=origin, **kw)
    assert all(torch.equal(null[k], plain[k]) for k in ("nchw", "u8", "labels")) and not torch.equal(null["labels"], out["labels"])


@pytest.mark.parametrize("rows", MIXED, ids=["0011", "101"])
def test_mixed_freq_pick_equals_the_two_launches_it_replaces(rows):
    _need_gpu()
    from miccai2021_cataract_semantic_segmentation_amd import ops
    B = len(rows)
    _, lbl, flips = _frames(B, rows, 13)
    luts, minv = _luts(), _mats(B, 4)
    wq = [1 + 37 * c * c for c in range(18)]                      # integer class weights: the pick depends on every remapped label
    m53 = [int(u * 2 ** 53) for u in np.random.RandomState(5).uniform(0.05, 0.95, B)]
    args = dict(canvas=(2 * FH, 2 * FW), px=12, wq=wq, return_debug=True)
    got = ops.crop_freq_pick(lbl, luts, flips, minv, m53=m53, tables=torch.tensor(rows, dtype=torch.int32).cuda(), **args)
    for t in (0, 1):
        sel = [b for b in range(B) if rows[b] == t]
        idx = torch.tensor(sel).cuda()
        part = ops.crop_freq_pick(lbl[idx].contiguous(), luts[t].contiguous(), flips[idx].contiguous(), minv[sel], m53=[m53[b] for b in sel], **args)
        for a, b in zip(got, part):
            assert torch.equal(a[idx], b)
    null = ops.crop_freq_pick(lbl, luts, flips, minv, m53=m53, **args)
    plain = ops.crop_freq_pick(lbl, luts[0].contiguous(), flips, minv, m53=m53, **args)
    assert all(torch.equal(a, b) for a, b in zip(null, plain))
    assert not torch.equal(null[1], got[1])                       # the totals of the pseudo frames differ under the wrong table


def test_gpu_ingest_label_tables_and_the_paired_loader():
    """GpuIngest(label_tables=) validates on the host and reaches the same launch; PinnedFrameLoader lays a BalancedConcatDataset out as
    [labelled | pseudo-labelled] with the tables to match"""
    _need_gpu()
    from miccai2021_cataract_semantic_segmentation_amd.utils import BalancedConcatDataset, GpuIngest, remap_lut
    from miccai2021_cataract_semantic_segmentation_amd.utils.loader import PinnedFrameLoader
    rows = [0, 0, 1, 1]
    img, lbl, flips = _frames(4, rows, 14)
    ing = GpuIngest(2)
    x, labels = ing(img, lbl, flips.cpu().numpy(), label_tables=rows)
    lut = T(remap_lut(2)).cuda()
    both = [ing(img, lbl, flips.cpu().numpy())[1], ing(img, lbl, flips.cpu().numpy(), label_tables=[1, 1, 1, 1])[1]]
    assert torch.equal(labels[:2], both[0][:2]) and torch.equal(labels[2:], both[1][2:]) and not torch.equal(both[0], both[1])
    assert torch.equal(both[0][:, 2:-2][flips == 0], lut[lbl.long()][flips == 0].long())
    with pytest.raises(ValueError, match=r"\[0, 2\)"):
        ing(img, lbl, None, label_tables=[0, 0, 2, 1])

    class Frames:
        def __init__(self, n, net, seed):
            g = torch.Generator().manual_seed(seed)
            self.img = torch.randint(0, 256, (n, FH, FW, 3), generator=g).to(torch.uint8).numpy()
            self.lbl = torch.randint(0, 18 if net else 36, (n, FH, FW), generator=g).to(torch.uint8).numpy()

        def __len__(self):
            return len(self.img)

        def __getitem__(self, i):
            return self.img[i], self.lbl[i]

    lab, pseudo = Frames(5, False, 1), Frames(6, True, 2)
    loader = PinnedFrameLoader(BalancedConcatDataset(lab, pseudo), batch_size=4, experiment=2, shuffle=False, flip_probability=(0.0, 0.0),
                               labels_remapped=(False, True), pseudo_colorjitter=2)
    assert len(loader) == 3
    batches = list(loader)
    loader.close()
    assert len(batches) == 3
    lut_h = remap_lut(2)
    for bi, (x, labels) in enumerate(batches):
        assert x.shape == (4, 3, FH + 4, FW) and labels.shape == (4, FH + 4, FW)
        got = labels[:, 2:-2].cpu().numpy()
        for j in range(2):
            i = 2 * bi + j
            assert np.array_equal(got[j], lut_h[lab.lbl[i % 5]]) and np.array_equal(got[2 + j], pseudo.lbl[i % 6])


# ---- the manager
def _manager_cfg(tmp_path, **train):
    return {"name": "semi", "mode": "training", "manager": "OCRNet", "log_path": str(tmp_path),
            "graph": {"model": "OCRNet", "backbone": "resnet50", "out_stride": 8, "pretrained": False},
            "data": {"experiment": 2, "batch_size": 2},
            "loss": {"name": "SemiSupervisedLoss", "labeled": _two_scale(1.0, 1.0), "unlabeled": _two_scale(0.7, 0.5)},
            "train": dict({"learning_rate": 1e-3, "epochs": 1}, **train), "log_every_n_epochs": 1, "seed": 0}


class _PseudoFrames(torch.utils.data.Dataset):
    def __init__(self, frames, labels):
        self.frames, self.labels = frames, labels

    def __len__(self):
        return len(self.labels)

    def __getitem__(self, i):
        return self.frames[i][0], T(self.labels[i]).long(), {"index": i}


def test_ocrnet_manager_pseudo_labels_trains_and_validates(tmp_path):
    _need_gpu()
    from miccai2021_cataract_semantic_segmentation_amd.losses import SemiSupervisedLoss
    from miccai2021_cataract_semantic_segmentation_amd.managers import OCRNetManager, SyntheticCataractDataset
    from miccai2021_cataract_semantic_segmentation_amd.models import OCRNet
    from miccai2021_cataract_semantic_segmentation_amd.utils import BalancedConcatDataset, clipped_argmax
    labelled = SyntheticCataractDataset(5, 64, 96, 17, seed=1)
    unlabelled = SyntheticCataractDataset(6, 64, 96, 17, seed=3)
    valid = SyntheticCataractDataset(2, 64, 96, 17, seed=2)
    m = OCRNetManager(_manager_cfg(tmp_path / "eager"), None, valid)
    assert isinstance(m.loss, SemiSupervisedLoss)
    initial = {k: v.detach().clone() for k, v in m.model.state_dict().items()}
    # ---- pseudo labels: torch's clipped_argmax of the same logits, outside a 1e-5 band of scores
    m.model.eval()
    with torch.no_grad():
        probs = torch.cat([torch.softmax(m.model(unlabelled[i][0][None].cuda())[1].float(), 1).cpu() for i in range(6)])
    m.model.train()
    top2 = probs.topk(2, dim=1).values
    for threshold in (0.5, round(float(top2[:, 0].median()), 3)):      # the second: a mix of kept and ignored pixels whatever the weights
        got = {}
        assert m.pseudo_label(unlabelled, lambda i, lab: got.__setitem__(i, lab), threshold=threshold) == 6
        assert sorted(got) == list(range(6)) and all(v.dtype == np.uint8 and v.shape == (64, 96) for v in got.values())
        want = clipped_argmax(probs, threshold, 17).numpy()
        band = ((top2[:, 0] - threshold).abs() <= 1e-5) | ((top2[:, 0] - top2[:, 1]) <= 1e-5)
        differ = np.stack([got[i] for i in range(6)]) != want
        print("threshold", threshold, "ignored", int((want == 17).sum()), "of", want.size, "in the band", int(band.sum()), "differ", int(differ.sum()))
        assert int(band.sum()) <= 0.01 * want.size
        assert not (differ & ~band.numpy()).any()
    assert 0 < int((want == 17).sum()) < want.size
    assert m.model.training and m.model.get_intermediate                 # pseudo_label left the training manager as it was
    with pytest.raises(ValueError, match="mark pixels below the threshold"):
        m.experiment = 1
        try:
            m.pseudo_label(unlabelled, lambda i, lab: None, threshold=0.5)
        finally:
            m.experiment = 2
    # ---- one epoch on (5 labelled, 6 pseudo-labelled): eager and as a hipGraph, identical parameters
    pseudo = _PseudoFrames(unlabelled, [got[i] for i in range(6)])
    pair = BalancedConcatDataset(labelled, pseudo)
    assert len(pair) == 6
    assert all(torch.equal(v, initial[k]) for k, v in m.model.state_dict().items())      # labelling trained nothing
    weights = []
    for name, mgr in (("eager", m), ("graph", OCRNetManager(_manager_cfg(tmp_path / "graph", hip_graph=True), None, valid))):
        mgr.model.load_state_dict(initial)                                 # (each manager drew its own initial weights)
        mgr.train_set = pair
        mgr.train_loader, mgr.valid_loader = mgr.loaders()
        torch.manual_seed(5)                                               # the DataLoader's shuffle
        mgr.train_one_epoch()
        assert mgr.global_step == 3 and np.isfinite(mgr.history[-1]["train_loss"])
        weights.append(mgr.model.flat().flat.clone())
    assert torch.equal(weights[0], weights[1])
    # ---- validate(): the labelled loss on every (batch-of-one) validation frame
    m.validate()
    m.model.eval()
    total = torch.zeros((), device="cuda")
    with torch.no_grad():
        for i in range(len(valid)):
            img, lbl, _ = valid[i]
            interm, out = m.model(img[None].cuda())
            total += m.loss.loss_lab(interm, out, lbl[None].cuda())
    assert m.history[-1]["valid_loss"] == float(total) / len(valid)
    # ---- the checkpoint: the loss adds no state, the keys are the plain manager's
    m.save_checkpoint(is_best=True)
    ck = torch.load(str(m.log_dir / "chkpts" / "chkpt_best.pt"), weights_only=False)
    assert set(ck) == {"global_step", "epoch", "model_state_dict", "optimiser_state_dict", "best_loss", "best_miou", "is_best",
                       "scheduler_state_dict"}
    assert list(ck["model_state_dict"]) == list(OCRNet(_manager_cfg(tmp_path)["graph"], 2).state_dict())


def test_single_output_manager_passes_the_tensor(tmp_path):
    """DeepLabv3PlusManager-style managers hand the loss `out`: the tensor form, loss_lab on both halves"""
    _need_gpu()
    from miccai2021_cataract_semantic_segmentation_amd.managers import DeepLabv3PlusManager, SyntheticCataractDataset
    cfg = {"name": "semi1", "mode": "training", "manager": "DeepLabv3Plus", "log_path": str(tmp_path),
           "graph": {"model": "DeepLabv3Plus", "backbone": "resnet50", "out_stride": 8, "pretrained": False},
           "data": {"experiment": 2, "batch_size": 4}, "loss": _lovasz(2, 1.0, 0.5), "train": {"learning_rate": 1e-3, "epochs": 1}}
    cfg["loss"]["name"] = "SemiSupervisedLoss"
    m = DeepLabv3PlusManager(cfg, SyntheticCataractDataset(4, 64, 96, 17, seed=1), SyntheticCataractDataset(1, 64, 96, 17, seed=2))
    img, lbl = (torch.stack(v) for v in zip(*[m.train_set[i][:2] for i in range(4)]))
    m.model.train()
    loss, out = m.forward_loss(img.cuda(), lbl.cuda())
    want = m.loss.loss_lab(out.detach()[:2], lbl[:2].cuda()) * 1.0 + m.loss.loss_lab(out.detach()[2:], lbl[2:].cuda()) * 0.5
    assert float(loss.detach()) == float(want.detach()) and np.isfinite(float(loss.detach()))
