"""Fixture for EncDec(ResNet18 + PointRend) in TRAIN mode, generated with the REAL reference (EncDec / PointRend / UPerNet,
utils/pointrend_utils.py and losses/LossWrapper.py from the reference, torchvision trunk from the oracle's restatement), experiment 2
(K = 17), input 2 x 3 x 64 x 64, pr_train_num_pts 48, oversample ratio 3, importance ratio 0.75; labels with ignore pixels.
    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_pointrend_train.py
torch.rand inside the reference's sampler is recorded (the device path draws from its own generator: the tests feed the recorded points).
Three forwards: step 0 (everything below), then two torch.optim.Adam steps (lr 1e-4) with their own recorded points and losses.
Stored: state-dict spec and seed, x, lbl; per step both draws and the final point_coords; for step 0 the uncertainties of the candidates
with the k-th and (k+1)-th value per image and the size of the band around the k-th, point_logits, pred AT THE SCATTERED PIXELS only
(every other pixel is F.interpolate of the coarse logits: asserted here against the reference's tensor), coarse logits, the point labels,
loss_coarse and loss_points as the manager's lines compute them, every parameter's gradient norm.
Asserted: seg_logits and pred are one memory; no tie at the k-th uncertainty; at most 5 % of k candidates per image lie within
4e-3 max|logit| of the k-th uncertainty; at least one pixel is hit by two points; the fp32 restatement (tests/_pointrend_train_ref.py)
reproduces the reference's point set, point_logits, pred and both losses bit for bit.
The band counts the candidates OTHER than the k-th one: it is the set another evaluation may select differently, and the k-th candidate's
distance from its own value says nothing about that.  With k = int(0.75 * 48) = 36 the bound, 1.8, admits one such candidate per image.
WEIGHT_SEED and INPUT_SEED (of the input, the labels and the sampler's torch.rand) are pinned to a pair that meets every condition; the
environment variables POINTREND_TRAIN_FIXTURE_WEIGHTS / POINTREND_TRAIN_FIXTURE_SEED try another pair, which fails an assertion if unsuitable."""
import json
import os
import sys

import numpy as np
import torch
from torch import nn

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
import ref_harness  # noqa: E402
import _pointrend_ref as PR  # noqa: E402
import _pointrend_train_ref as TR  # noqa: E402
from oracle.state import spec_of  # noqa: E402

R = ref_harness.load()
ref_utils = sys.modules["utils.pointrend_utils"]
ref_pointrend = sys.modules["models.PointRend"]
K, P = 17, TR.FIXTURE_P
M, KB, REST = TR.counts(P, TR.FIXTURE_RATIO, TR.FIXTURE_BETA)


class _RecordingTorch:
    """the torch module as utils/pointrend_utils.py sees it, with rand recorded"""

    def __init__(self):
        self.draws = []

    def __getattr__(self, name):
        return getattr(torch, name)

    def rand(self, *a, **k):
        t = torch.rand(*a, **k)
        self.draws.append(t.clone())
        return t


WEIGHT_SEED = int(os.environ.get("POINTREND_TRAIN_FIXTURE_WEIGHTS", "891"))
INPUT_SEED = int(os.environ.get("POINTREND_TRAIN_FIXTURE_SEED", "9476"))
torch.manual_seed(9)
MODEL = R.models.EncDec(TR.model_config(on_device=False), 2)
SPEC = spec_of(MODEL.state_dict())
FILLED = PR.fill_state(SPEC, WEIGHT_SEED)


def generate(seed):
    """seed: of the input, the labels and the sampler's torch.rand; the weights are fill_state(WEIGHT_SEED)"""
    g = torch.Generator().manual_seed(seed + 1)
    x = torch.rand(2, 3, 64, 64, generator=g)
    lbl = torch.randint(0, K, (2, 8, 8), generator=g).repeat_interleave(8, 1).repeat_interleave(8, 2)
    lbl[torch.rand(2, 64, 64, generator=g) < 0.1] = K                        # ignore pixels
    model, spec = MODEL, SPEC
    model.load_state_dict(FILLED)
    torch.manual_seed(seed)
    S0 = {k: v.clone() for k, v in model.state_dict().items()}
    model.train()
    model.get_features = True
    rec = _RecordingTorch()
    unc_seen, grabbed = [], {}
    calc = ref_pointrend.calculate_uncertainty
    ref_utils.torch = rec
    ref_pointrend.calculate_uncertainty = lambda logits: (unc_seen.append(calc(logits).clone()), calc(logits))[1]
    hook = model.dec_model.partial_upernet.register_forward_hook(lambda m, i, o: grabbed.__setitem__("coarse", o.detach().clone()))
    loss_fct = R.losses.LossWrapper({"losses": {"CrossEntropyLoss": 1}, "experiment": 2, "device": "cpu"})
    opt = torch.optim.Adam(model.parameters(), lr=1e-4)
    out = {"x": PR.as_np(x), "lbl": PR.as_np(lbl), "seed": np.array(WEIGHT_SEED), "input_seed": np.array(seed), "spec": np.array(json.dumps(spec))}
    losses = []
    try:
        for step in range(3):
            del rec.draws[:], unc_seen[:]
            opt.zero_grad()
            # (models/EncDec.py:50 returns the decoder's 4-tuple nested behind the features; the manager's line unpacks five values)
            deep_features, (point_coords, point_logits, seg_logits, prediction) = model(x)
            assert seg_logits.data_ptr() == prediction.data_ptr()            # the reshape is a view: the scatter ran in place
            # managers/EncDec_Manager.py:163-171
            loss_coarse = loss_fct(deep_features, seg_logits, lbl.long(), epoch=0)
            lbl_logits = ref_utils.point_sample(lbl.unsqueeze(1).float(), point_coords, mode='nearest').squeeze(1)
            ce_loss = nn.CrossEntropyLoss(ignore_index=K)
            loss_points = ce_loss(point_logits.unsqueeze(3), lbl_logits.unsqueeze(2).long())
            loss = loss_coarse + loss_points
            loss.backward()
            cand, rest = rec.draws
            assert cand.shape == (2, M, 2) and rest.shape == (2, REST, 2) and len(unc_seen) == 1
            out["cand%d" % step], out["rest%d" % step], out["coords%d" % step] = PR.as_np(cand), PR.as_np(rest), PR.as_np(point_coords)
            losses.append([float(loss_coarse), float(loss_points)])
            if step == 0:
                unc = unc_seen[0][:, 0]
                kth, nxt = PR.kth_values(unc.unsqueeze(1), KB)
                assert bool((kth > nxt).all()), "a tie at the k-th uncertainty"
                coarse = grabbed["coarse"]
                scale = float(prediction.detach().abs().max())
                band = ((unc - kth[:, None]).abs() <= 4e-3 * scale).sum(1) - 1          # (without the k-th candidate itself)
                assert int(band.max()) <= 0.05 * KB, "band %s of k = %d" % (band.tolist(), KB)
                pix = TR.pixel_index(point_coords, 64, 64)
                dup = max(int(torch.bincount(r).max()) for r in pix)
                assert dup >= 2, "no pixel is hit by two points"
                # the restatement, fp32: the reference's point set (its order: descending uncertainty), logits, pred, losses, bit for bit
                mine_unc = TR.point_uncertainty(coarse, cand)
                assert torch.equal(mine_unc, unc)
                mine_pts, _ = TR.select_points(mine_unc, cand, rest, KB, ascending=False)
                assert torch.equal(mine_pts, point_coords)
                _, c2, pl2, pred2, pix2 = TR.network_forward(S0, x, point_coords)
                assert torch.equal(c2, coarse) and torch.equal(pl2, point_logits) and torch.equal(pred2, prediction) and torch.equal(pix2, pix)
                lc2, lp2 = TR.manager_losses(pl2, pred2, lbl, point_coords, K)
                assert float(lc2) == float(loss_coarse) and float(lp2) == float(loss_points)
                assert torch.equal(TR.point_labels(lbl, point_coords), lbl_logits.long())
                # pred = interpolate(coarse) with the point logits scattered in: only the scattered pixels are stored
                rebuilt = TR.scatter_last(torch.nn.functional.interpolate(coarse, scale_factor=4, mode="bilinear", align_corners=False), pix,
                                          point_logits.detach())
                assert torch.equal(rebuilt, prediction.detach())
                out.update(unc=PR.as_np(unc), kth=np.stack([PR.as_np(kth), PR.as_np(nxt)]), band=PR.as_np(band), scale=np.array(scale),
                           coarse=PR.as_np(coarse), point_logits=PR.as_np(point_logits), pix=PR.as_np(pix),
                           pred_at_points=PR.as_np(prediction.detach().reshape(2, K, -1).gather(2, pix.unsqueeze(1).expand(-1, K, -1))),
                           point_labels=PR.as_np(lbl_logits.long()), max_points_per_pixel=np.array(dup))
                names = [k for k, _ in model.named_parameters()]
                out["grad_names"] = np.array(json.dumps(names))
                out["grad_norms"] = np.array([float(p.grad.double().norm()) for _, p in model.named_parameters()])
            opt.step()
    finally:
        hook.remove()
        ref_utils.torch = torch
        ref_pointrend.calculate_uncertainty = calc
    out["losses"] = np.array(losses)
    return out


out = generate(INPUT_SEED)
path = os.path.join(HERE, TR.FIXTURE + ".npz")
np.savez_compressed(path, **out)
print("wrote", path, os.path.getsize(path), "bytes; losses", out["losses"].tolist(), "band", out["band"].tolist(), "max points per pixel",
      int(out["max_points_per_pixel"]))
