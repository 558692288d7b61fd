"""PointRend's eval-mode forward on the GPU: ops.pointrend_refine against the fp64 restatement (tests/_pointrend_ref.py), the whole network
against the fixture of the real reference, eager against hipGraph replay, and the callers (EncDecManager, Ensemble, TTA)."""
import copy
import json
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _pointrend_ref as PR  # noqa: E402

pytestmark = pytest.mark.gpu
T = torch.from_numpy
FIXTURE = "pointrend_r18_e2_tiny"


def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")


def _nhwc(t):
    return t.permute(0, 2, 3, 1).contiguous().cuda()


def _dev_head(head):
    return {"fc": [(w.cuda(), b.cuda()) for w, b in head["fc"]], "predictor": tuple(t.cuda() for t in head["predictor"]),
            "coarse_in_each_layer": head["coarse_in_each_layer"]}


# ------------------------------------------------------------------------------------------------------------ the seam
@pytest.mark.parametrize("shape,k0,steps", PR.seam_cases())
def test_refine_against_the_fp64_restatement(shape, k0, steps):
    """Selection: exactly fp64's outside the undecided pixels (tests/_pointrend_ref.undecided), none of which lies in a step before the last
    (the seeds are chosen so: _pointrend_ref.seam_search) and at most 1 % of k in the last.  Logits: within 4 x the distance of the fp32
    torch-CPU restatement from fp64 (floor 1e-6 of the logit scale); an undecided pixel may hold the refined or the unrefined fp64 value.
    Measured (MI355X), GPU distance / fp32-CPU distance, per case: see the printed line; the README row quotes the range."""
    _need_gpu()
    from miccai2021_cataract_semantic_segmentation_amd import ops
    (coarse, feats, head), (f64, r64), (f32, _), und, scale = PR.seam_reference(shape, k0, steps, PR.SEAM_SEEDS[(shape, k0, steps)])
    seg = ops.new_act(*coarse.permute(0, 2, 3, 1).shape, "cuda", ld=32, zero=True)
    seg.copy_(coarse.permute(0, 2, 3, 1))
    rec = []
    out = ops.pointrend_refine(seg, [_nhwc(f) for f in feats], _dev_head(head), k0, steps, record=rec)
    got = out.cpu().permute(0, 3, 1, 2).double()
    assert got.shape == f64.shape and len(rec) == steps
    for s, (r, ref, m) in enumerate(zip(rec, r64, und)):
        hw, k = m.shape[1], ref["idx"].shape[1]
        assert r["idx"].shape == (coarse.shape[0], k)
        assert not bool(((PR.selected(r["idx"].cpu(), hw) != PR.selected(ref["idx"], hw)) & ~m).any()), "step %d selects differently from fp64" % s
        assert int(m.sum(1).max()) <= 0.01 * k and (s == steps - 1 or not bool(m.any()))
    last = und[-1].view(f64.shape[0], 1, *f64.shape[2:]).expand_as(f64)
    d_torch = float((f32.double() - f64).abs()[~last].max())
    d_gpu = float((got - f64).abs()[~last].max())
    bar = 4 * d_torch + 1e-6 * scale
    print("refine %s k0=%d steps=%d: GPU %.3g, fp32 CPU %.3g from fp64 (ratio %.2f), scale %.3g, undecided %d"
          % (shape, k0, steps, d_gpu, d_torch, d_gpu / d_torch, scale, int(und[-1].sum())))
    assert d_gpu <= bar
    if bool(last.any()):
        either = torch.minimum((got - f64).abs(), (got - r64[-1]["before"]).abs())
        assert float(either[last].max()) <= bar


# ------------------------------------------------------------------------------------------------------------ the reference's fixture
def _fixture_model(g, cfg):
    from miccai2021_cataract_semantic_segmentation_amd.models import EncDec
    spec = json.loads(str(g["spec"]))
    model = EncDec(PR.model_config(PR.CONFIG[cfg]), 2)
    assert [k for k, _ in spec] == list(model.state_dict().keys())
    model.load_state_dict(PR.fill_state(spec, int(g["seed"])))
    model.cuda().eval()
    model.get_features = False
    return model


def _recorded_forward(model, x):
    """model(x) with the coarse logits and the per-step records of ops.pointrend_refine"""
    from miccai2021_cataract_semantic_segmentation_amd import ops
    seen, refine = {}, ops.pointrend_refine

    def spy(seg, feats, head, k0, steps, record=None):
        seen["coarse"], seen["rec"] = seg.clone(), []
        return refine(seg, feats, head, k0, steps, record=seen["rec"])

    ops.pointrend_refine = spy
    try:
        with torch.no_grad():
            out = model(x)
    finally:
        ops.pointrend_refine = refine
    return out, seen["coarse"].cpu().permute(0, 3, 1, 2), seen["rec"]


@pytest.mark.usefixtures("precision")
def test_encdec_resnet18_pointrend_matches_reference_fixture(golden):
    """The bar of test_encdec_resnet18_upernet_matches_reference_fixture: 1e-3 of max|reference logits|.  A pixel whose recorded uncertainty lies
    within 4e-3 max|logit| of the k-th value (twice the bar on a difference of two logits, doubled) may be selected either way: there the
    logits must match the reference's final or its pre-scatter value.  The generator recorded 37 and 51 such pixels of k = 1024 for A's step 2
    and 20 and 26 of 1024 pixels (k = 96) for B's step 1.  B's assertion here is weak: a band of 20 / 26 pixels around a selection of 96 lets
    about a quarter of it go either way, so it only shows that the bulk of the selection is the reference's.  What pins B is the CPU
    restatement (bit for bit against the reference) and the seam test against that restatement."""
    _need_gpu()
    g = golden(FIXTURE)
    x = T(g["x"]).cuda()
    # A: step 1 refines every pixel, step 2 1024 of 4096
    step1, before2, final = PR.fixture_tensors(g, "A")
    out, coarse, rec = _recorded_forward(_fixture_model(g, "A"), x)
    scale = float(g["A_scale"])
    bar = 1e-3 * scale
    assert abs(scale - float(final.abs().max())) == 0
    assert float((coarse - T(g["coarse"])).abs().max()) <= 1e-3 * float(np.abs(g["coarse"]).max())
    assert np.array_equal(rec[0]["idx"].cpu().numpy(), g["A_idx1"]) and rec[1]["idx"].shape == (2, 1024)
    band = (T(g["A_unc2"]).reshape(2, -1) - T(g["A_kth2"][0])[:, None]).abs() <= 4e-3 * scale
    assert band.sum(1).tolist() == g["A_band2"].tolist() and int(band.sum(1).max()) <= 0.05 * 1024
    sel_ref = PR.selected(T(g["A_idx2"]), 4096)
    assert not bool(((PR.selected(rec[1]["idx"].cpu(), 4096) != sel_ref) & ~band).any())
    err = (out.cpu() - final).abs()
    inband = band.view(2, 1, 64, 64).expand_as(err)
    print("pointrend fixture A: max err outside the band %.3g, bar %.3g" % (float(err[~inband].max()), bar))
    assert float(err[~inband].max()) <= bar
    assert float(torch.minimum(err, (out.cpu() - before2).abs())[inband].max()) <= bar
    # B: pinned through the restatement on the CPU and through the seam test; here only its step-1 selection outside the band
    out, _, rec = _recorded_forward(_fixture_model(g, "B"), x)
    band = (T(g["B_unc1"]).reshape(2, -1) - T(g["B_kth1"][0])[:, None]).abs() <= 4e-3 * float(g["B_scale"])
    assert band.sum(1).tolist() == g["B_band1"].tolist()
    assert not bool(((PR.selected(rec[0]["idx"].cpu(), 1024) != PR.selected(T(g["B_idx1"]), 1024)) & ~band).any())
    assert out.shape == (2, 17, 64, 64) and bool(torch.isfinite(out).all())


# ------------------------------------------------------------------------------------------------------------ hipGraph
def test_eager_forward_equals_graph_replay_bit_for_bit(golden):
    """the eval forward captured once and replayed on three different inputs: the selection has no host dependence"""
    _need_gpu()
    g = golden(FIXTURE)
    model = _fixture_model(g, "B")
    gen = torch.Generator().manual_seed(7)
    xs = [T(g["x"]).cuda()] + [torch.rand(2, 3, 64, 64, generator=gen).cuda() for _ in range(2)]
    with torch.no_grad():
        eager = [model(x).clone() for x in xs]
        static = xs[1].clone()
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            for _ in range(2):
                model(static)
        torch.cuda.current_stream().wait_stream(side)
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=side):
            out = model(static)
        for x, want in zip(xs, eager):
            static.copy_(x)
            graph.replay()
            torch.cuda.synchronize()
            assert torch.equal(out, want)
    assert not torch.equal(eager[0], eager[1])


# ------------------------------------------------------------------------------------------------------------ managers and callers
def _checkpoint(tmp_path, run, seed, k0=96):
    """a run directory holding a 'best' checkpoint with the reference's keys"""
    from miccai2021_cataract_semantic_segmentation_amd.models import EncDec
    spec = [(k, tuple(v.shape)) for k, v in EncDec(PR.model_config(k0), 2).state_dict().items()]
    (tmp_path / run / "chkpts").mkdir(parents=True)
    torch.save({"global_step": 1, "epoch": 0, "model_state_dict": PR.fill_state(spec, seed), "best_loss": 1.0, "best_miou": 1.0, "is_best": True},
               str(tmp_path / run / "chkpts" / "chkpt_best.pt"))


class _Video(torch.utils.data.Dataset):
    """frames as DatasetFromVideo yields them: (float [3, H, W] in [0, 1], frame index, video id)"""

    def __init__(self, n, H, W):
        self.frames = torch.rand(n, 3, H, W, generator=torch.Generator().manual_seed(11))

    def __len__(self):
        return len(self.frames)

    def __getitem__(self, i):
        return self.frames[i], 10 * i, 7


def test_encdec_manager_round_trip_validate_infer_tta_demo(tmp_path):
    _need_gpu()
    from torch.utils.data import DataLoader
    from miccai2021_cataract_semantic_segmentation_amd import managers, models
    from miccai2021_cataract_semantic_segmentation_amd import utils as U
    _checkpoint(tmp_path, "run", 5)          # (best_miou 1.0 in the file: validate() finds no new best and writes no checkpoint)
    va = managers.SyntheticCataractDataset(2, 64, 96, 17, seed=2)
    cfg = dict(PR.model_config(96), name="pr", mode="inference", manager="EncDec", log_path=str(tmp_path), load_checkpoint="run",
               data={"experiment": 2, "batch_size": 2}, loss={"losses": {"LovaszSoftmax": 1}}, train={"learning_rate": 1e-4, "epochs": 5},
               log_every_n_epochs=10)
    m = managers.EncDecManager(copy.deepcopy(cfg), None, va)
    assert isinstance(m.model.dec_model, models.PointRend) and m.loss is None
    m.load_checkpoint("best")
    ck = torch.load(str(tmp_path / "run" / "chkpts" / "chkpt_best.pt"), weights_only=False)["model_state_dict"]
    assert torch.equal(m.model.state_dict()["dec_model.point_head.fc1.weight"].cpu(), ck["dec_model.point_head.fc1.weight"])
    # validate() itself, as the training loop calls it after an epoch: eval mode, (deep features, prediction) into the LossWrapper
    m.load_loss()
    m.valid_loader = DataLoader(va, batch_size=1, shuffle=False)
    miou_valid = m.validate()
    assert np.isfinite(miou_valid) and (m.log_dir / "info.json").exists() and not m.model.training
    miou = m.infer()                                   # loads the checkpoint again, prediction only
    assert len(miou) == 4 and all(np.isfinite(v) for v in miou) and abs(round(miou[0], 4) - miou_valid) < 1e-9
    cm, _ = m._eval_pass(m.valid_loader, with_loss=False)
    assert int(cm.sum()) > 0
    m.config["tta"] = True
    tta = m.infer()
    assert len(tta) == 4 and all(np.isfinite(v) for v in tta) and isinstance(m.model, models.EncDec)
    # demo_infer: three frames, the sink gets frame | coloured prediction of the same model's logits, in order
    video, got = _Video(3, 64, 96), []
    dm = managers.EncDecManager(dict(copy.deepcopy(cfg), mode="demo_video_inference"), video_set=video,
                                frame_sink=lambda vid, idx, arr: got.append((vid, idx, arr)))
    assert dm.demo_infer() == 3 and [(v, i) for v, i, _ in got] == [(7, 0), (7, 10), (7, 20)]
    egress = U.GpuEgress(2, crop=(0, 0), bgr=True, device=dm.device)       # as demo_infer builds it
    for i, (_, _, arr) in enumerate(got):
        frame = video.frames[i:i + 1].cuda().float()
        with torch.no_grad():
            want = egress(dm.model(frame), frame=frame)[0]
        assert arr.shape == (64, 192, 3) and np.array_equal(arr, want.cpu().numpy())


def test_pointrend_as_an_ensemble_member(tmp_path):
    _need_gpu()
    from miccai2021_cataract_semantic_segmentation_amd import managers, models
    _checkpoint(tmp_path, "a", 5)
    _checkpoint(tmp_path, "b", 6)
    member = lambda run: dict(PR.model_config(96), model="UPerNet", ckpt=run)
    cfg = {"name": "ens", "mode": "inference", "manager": "Ensemble", "log_path": str(tmp_path), "data": {"experiment": 2},
           "graph": {"model": "Ensemble", "merge": "mean", "members": {"1": member("a"), "2": member("b")}}, "loss": {"name": "LovaszSoftmax"}}
    va = managers.SyntheticCataractDataset(2, 64, 96, 17, seed=2)
    em = managers.EnsembleManager(cfg, None, va)
    assert all(isinstance(mm.dec_model, models.PointRend) and not mm.training for mm in em.model.members)
    x = torch.rand(1, 3, 64, 96, generator=torch.Generator().manual_seed(1)).cuda()
    with torch.no_grad():
        probs = em.model(x)
        inside = [z.permute(0, 3, 1, 2) for z in em.model._member_logits(x)]
    want = torch.stack([torch.softmax(z, 1) for z in inside]).mean(0)
    assert probs.shape == (1, 17, 64, 96) and float((probs - want).abs().max()) <= 1e-6
    miou = em.infer()
    assert len(miou) == 4 and all(np.isfinite(v) for v in miou)
