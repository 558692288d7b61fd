"""UNet (reference models/UNet.py:6-63) on the GPU: against the fixture the REAL reference wrote (tests/golden/make_golden_unet.py) and the
CPU restatement (tests/_unet_ref.py), on the production routes with the record producers of BatchNorm-free layers on and off, under
hipGraph replay, and through FCNManager."""
import json
import os
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

_CPU = {}


def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")


def _records(on):
    """context: the plan field bnfree_records set to `on`"""
    import contextlib
    from miccai2021_cataract_semantic_segmentation_amd import ops

    @contextlib.contextmanager
    def cm():
        saved, ops.BNFREE_RECORDS = ops.BNFREE_RECORDS, on
        try:
            yield
        finally:
            ops.BNFREE_RECORDS = saved
            ops.release_b3_cache()
    return cm()


def _cpu_reference(spec, seed, x, lbl):
    """the restatement's fp32 train step (logits, loss, gradients) and its fp64 logits, once per input"""
    from _unet_ref import unet_forward
    from oracle import losses as OL
    from oracle.state import fill_state
    key = (seed, tuple(x.shape))
    if key not in _CPU:
        S = fill_state(spec, seed)
        with torch.no_grad():
            y64 = unet_forward({k: v.double() for k, v in S.items()}, x.double())
        for v in S.values():
            v.requires_grad_()
        y32 = unet_forward(S, x)
        loss = OL.lovasz_softmax(y32, lbl)
        loss.backward()
        _CPU.clear()
        _CPU[key] = (y64, y32.detach(), float(loss.detach()), {k: v.grad for k, v in S.items()})
    return _CPU[key]


@pytest.mark.parametrize("records", [False, True], ids=["composed", "records"])
def test_unet_matches_reference_fixture_and_restatement(golden, precision, records):
    _need_gpu()
    from _unet_ref import make_inputs, summarise
    from oracle.state import fill_state
    from miccai2021_cataract_semantic_segmentation_amd.models import UNet
    from miccai2021_cataract_semantic_segmentation_amd.losses import LovaszSoftmax
    from miccai2021_cataract_semantic_segmentation_amd.optim import FusedAdam
    g = golden("unet_e2_tiny")
    spec, seed, shape = json.loads(str(g["spec"])), int(g["seed"]), tuple(int(v) for v in g["shape"])
    x, lbl = make_inputs(seed, shape, int(g["num_classes"]))
    y64, _, _, grads = _cpu_reference(spec, seed, x, lbl)
    scale = float(g["train_scale"])
    with _records(records):
        model = UNet({}, 2)
        assert [k for k, _ in spec] == list(model.state_dict().keys())
        model.load_state_dict(fill_state(spec, seed))
        model.cuda().train()
        xd, ld = x.cuda(), lbl.cuda()
        crit = LovaszSoftmax({"experiment": 2})
        opt = FusedAdam(model, lr=1e-3)
        losses = []
        for step in range(2):
            opt.zero_grad()
            y = model(xd)
            loss = crit(y, ld)
            loss.backward()
            if step == 0:
                yc = y.detach().cpu()
                s = summarise(yc)
                e_sub, e_rows = np.abs(s["sub"] - g["train_sub"]).max(), np.abs(s["rows"] - g["train_rows"]).max()
                e64 = float((yc.double() - y64).abs().max())
                print("UNet logits vs fixture %.3g / %.3g, vs fp64 %.3g (scale %.2f)" % (e_sub, e_rows, e64, scale))
                assert e_sub <= 1e-3 * max(1.0, scale) and e_rows <= 1e-3 * max(1.0, scale)
                assert e64 <= 1e-3
                names = json.loads(str(g["grad_names"]))
                P = dict(model.named_parameters())
                norms = np.array([float(P[k].grad.double().norm()) for k in names])
                np.testing.assert_allclose(norms, g["grad_norms"], rtol=2e-2, atol=1e-9)
                for k in names:          # every parameter's gradient against the restatement's, element by element
                    ref = grads[k]
                    err = float((P[k].grad.cpu() - ref).abs().max())
                    assert err <= 3e-2 * float(ref.abs().max()) + 1e-9, (k, err, float(ref.abs().max()))
                for k in ("conv_last.bias", "dconv_up1.0.bias"):
                    ref = g["g:" + k]
                    assert np.abs(P[k].grad.cpu().numpy() - ref).max() <= 3e-2 * np.abs(ref).max(), k
            opt.step()
            losses.append(float(loss.detach()))
        assert abs(losses[0] - float(g["losses"][0])) < 1e-4
        assert abs(losses[1] - float(g["losses"][1])) < 5e-3 * float(g["losses"][1])
        # inference path (no tape) gives the same logits as the recorded forward of the same weights
        model.eval()
        with torch.no_grad():
            e1 = model(xd)
        model.train()
        y2 = model(xd)
        assert torch.equal(e1, y2.detach())


@pytest.mark.parametrize("records", [True, False], ids=["records", "composed"])
def test_unet_production_routes(records):
    """2 x 3 x 96 x 128 under the production thresholds: 24 576 / 6 144 / 1 536 / 384 pixels per level, the first two above DCONV3_MIN_ROWS and
    g1_min_rows.  With the record producers on, the 64 -> 64 layers run the f16x2 direct kernel and the other level-1 / level-2 layers the
    gather kernel in all three directions; off, no layer does."""
    _need_gpu()
    from _calib import calibrated_grad_check
    from _unet_ref import make_inputs, unet_forward
    from oracle import losses as OL
    from oracle.state import fill_state, spec_of
    from miccai2021_cataract_semantic_segmentation_amd import ops
    from miccai2021_cataract_semantic_segmentation_amd.models import UNet
    from miccai2021_cataract_semantic_segmentation_amd.losses import LovaszSoftmax
    saved = ops.PRECISION
    ops.PRECISION = "bf16x3"
    try:
        with _records(records):
            model = UNet({}, 2)
            spec = spec_of(model.state_dict())
            model.load_state_dict(fill_state(spec, 21))
            model.cuda().train()
            x, lbl = make_inputs(22, (2, 3, 96, 128), model.num_classes)
            y64, y32, loss32, _ = _cpu_reference(spec, 21, x, lbl)
            ops.PROFILE = []
            try:
                y = model(x.cuda())
                n_fwd = len(ops.PROFILE)
                loss = LovaszSoftmax({"experiment": 2})(y, lbl.cuda())
                loss.backward()
                torch.cuda.synchronize()
                kinds_f = {k for k, *_ in ops.PROFILE[:n_fwd]}
                kinds_b = {k for k, *_ in ops.PROFILE[n_fwd:]}
            finally:
                ops.PROFILE = None
            print("forward kinds", sorted(kinds_f), "backward kinds", sorted(kinds_b))
            want = {"fwd_d3h", "fwd_s2p"}, {"dgrad_d3h", "dgrad_s2p", "wgrad_d3h", "wgrad_s2p"}
            if records:
                assert want[0] <= kinds_f and want[1] <= kinds_b
            else:
                assert not [k for k in kinds_f | kinds_b if k.endswith("_d3h") or k.endswith("_s2p")]
            e64 = float((y.detach().cpu().double() - y64).abs().max())
            c64 = float((y32.double() - y64).abs().max())
            print("UNet logits vs fp64: HIP %.3g, CPU fp32 %.3g (scale %.2f)" % (e64, c64, float(y64.abs().max())))
            assert e64 <= max(1e-3, 1.5 * c64)
            assert abs(float(loss.detach()) - loss32) < 1e-4
            calibrated_grad_check(model, spec, 21, unet_forward, OL.lovasz_softmax, x, lbl, label="unet_96x128")
    finally:
        ops.PRECISION = saved


def test_unet_rejects_sizes_the_reference_cannot_concatenate():
    _need_gpu()
    from miccai2021_cataract_semantic_segmentation_amd.models import UNet
    model = UNet({}, 1).cuda().eval()
    with pytest.raises(ValueError, match="36 x 40"):
        with torch.no_grad():
            model(torch.zeros(1, 3, 36, 40, device="cuda"))


def test_unet_graphed_step_is_bit_identical_to_the_eager_step(precision):
    _need_gpu()
    from _unet_ref import make_inputs
    from miccai2021_cataract_semantic_segmentation_amd.graph import GraphedTrainStep
    from miccai2021_cataract_semantic_segmentation_amd.models import UNet
    from miccai2021_cataract_semantic_segmentation_amd.losses import LovaszSoftmax
    from miccai2021_cataract_semantic_segmentation_amd.optim import FusedAdam
    with _records(True):
        torch.manual_seed(5)
        model = UNet({}, 2).cuda().train()
        crit = LovaszSoftmax({"experiment": 2})
        opt = FusedAdam(model, lr=1e-3)
        batches = [tuple(t.cuda() for t in make_inputs(30 + i, (2, 3, 40, 56), model.num_classes)) for i in range(3)]
        fp = model.flat()
        w0 = fp.flat.clone()
        losses_e = []
        for xb, lb in batches:
            opt.zero_grad()
            out = model(xb)
            loss = crit(out, lb)
            loss.backward()
            opt.step()
            losses_e.append(float(loss.detach()))
        torch.cuda.synchronize()
        w_e, m_e, v_e, logits_e = fp.flat.clone(), opt._m.clone(), opt._v.clone(), out.detach().clone()
        with torch.no_grad():
            fp.flat.copy_(w0)
            opt._m.zero_()
            opt._v.zero_()
        opt._steps = 0
        step = GraphedTrainStep(model, crit, opt, *batches[0])
        losses_g = [float(step(xb, lb)) for xb, lb in batches]
        torch.cuda.synchronize()
        assert losses_g == losses_e and step.replays == 3
        assert torch.equal(fp.flat, w_e) and torch.equal(opt._m, m_e) and torch.equal(opt._v, v_e)
        out_g = step.outputs[0] if isinstance(step.outputs, (tuple, list)) else step.outputs
        assert torch.equal(out_g.detach(), logits_e)


def test_unet_through_the_fcn_manager(tmp_path, golden):
    """managers/FCN_Manager.py of the reference drives UNet too (graph.model = "UNet"): one epoch trains, the checkpoint holds the reference's
    keys, inference from it runs"""
    _need_gpu()
    from miccai2021_cataract_semantic_segmentation_amd import managers
    cfg = {"name": "unet", "mode": "training", "manager": "FCN", "log_path": str(tmp_path), "graph": {"model": "UNet"},
           "data": {"experiment": 2, "batch_size": 2}, "loss": {"name": "LovaszSoftmax"},
           "train": {"learning_rate": 1e-3, "epochs": 1}, "log_every_n_epochs": 1, "seed": 0}
    tr = managers.SyntheticCataractDataset(4, 48, 64, 17, seed=1)
    va = managers.SyntheticCataractDataset(2, 48, 64, 17, seed=2)
    m = managers.FCNManager(cfg, tr, va)
    m.train()
    assert len(m.history) == 1 and np.isfinite(m.history[0]["train_loss"]) and "valid_miou" in m.history[0]
    ck = torch.load(str(m.log_dir / "chkpts" / "chkpt_best.pt"), weights_only=False)
    spec = json.loads(str(golden("unet_e2_tiny")["spec"]))
    assert list(ck["model_state_dict"].keys()) == [k for k, _ in spec]
    assert [tuple(v.shape) for v in ck["model_state_dict"].values()] == [tuple(s) for _, s in spec]
    inf = managers.FCNManager(dict(cfg, mode="inference", load_checkpoint=m.run_id), None, va)
    assert np.isfinite(inf.infer()[0])
