"""SoftIoU / GenDiceLoss / FocalLoss fixtures from the REAL reference (losses/SoftIoU.py, losses/GenDiceLoss.py, losses/FocalLoss.py),
see make_golden.py.  Each case: NCHW logits, labels, the config (JSON), the loss and the logits gradient of loss * scale.

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_overlap.py
"""
import json
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
import ref_harness  # noqa: E402

R = ref_harness.load()
K_OF = {1: 8, 2: 17, 3: 25}
SHAPE = {1: (1, 8, 12), 2: (1, 8, 8), 3: (1, 6, 8)}
W17 = [1.0, 0.5, 2.0, 0.0, 1.5, 1.0, 0.25, 3.0, 1.0, 0.75, 1.25, 2.5, 1.0, 0.5, 1.0, 2.0, 1.0]
A8 = [0.25, 1.0, 0.5, 2.0, 0.75, 1.5, 1.0, 0.3]
CASES = []   # name, loss, config (experiment included), extra: absent / saturated, scale
for exp in (1, 2, 3):
    for naive in (False, True):
        CASES.append(("iou_e%d_%s" % (exp, "naive" if naive else "mean"), "SoftIoU", {"experiment": exp, "naive": naive}, None, 1.0))
for naive in (False, True):      # class 7 absent, its probability exactly 0 everywhere: union 0 -> excluded (non-naive) / nan (naive)
    CASES.append(("iou_absent_%s" % ("naive" if naive else "mean"), "SoftIoU", {"experiment": 1, "naive": naive}, "absent", 1.0))
for wname, w in (("none", None), ("auto", "auto"), ("list", W17)):
    for naive in (False, True):
        cfg = {"experiment": 2, "naive": naive}
        if w is not None:
            cfg["weights"] = w
        CASES.append(("dice_%s_%s" % (wname, "naive" if naive else "mean"), "GenDiceLoss", cfg, None, 1.0))
for gamma in (0, 0.5, 2, 3.5):
    for alpha in (None, A8):
        cfg = {"experiment": 1, "gamma": gamma}
        if alpha is not None:
            cfg["alpha"] = alpha
        CASES.append(("focal_g%s_%s" % (str(gamma).replace(".", "p"), "alpha" if alpha else "plain"), "FocalLoss", cfg, None, 1.0))
CASES.append(("focal_saturated_g1", "FocalLoss", {"experiment": 1, "gamma": 1}, "saturated", 1.0))
CASES.append(("focal_saturated_g2_alpha", "FocalLoss", {"experiment": 1, "gamma": 2, "alpha": A8}, "saturated", 1.0))
CASES.append(("focal_scaled", "FocalLoss", {"experiment": 1, "gamma": 2, "alpha": A8}, None, 0.3))
CASES.append(("iou_scaled", "SoftIoU", {"experiment": 3}, None, 0.3))
CASES.append(("dice_auto_scaled", "GenDiceLoss", {"experiment": 3, "weights": "auto"}, None, 0.3))

out = {"names": np.array([c[0] for c in CASES])}
for i, (name, loss_name, cfg, extra, scale) in enumerate(CASES):
    g = torch.Generator().manual_seed(700 + i)
    exp = cfg["experiment"]
    K = K_OF[exp]
    B, H, W = SHAPE[exp]
    logits = torch.randn(B, K, H, W, generator=g) * 2.0
    hi = K + 1 if exp in (2, 3) and loss_name != "FocalLoss" else K       # the ignore label is a valid input of the overlap losses only
    target = torch.randint(0, hi, (B, H, W), generator=g)
    if extra == "absent":
        target[target == 7] = 0
        logits[:, 7] = -1000.0
    if extra == "saturated":                                            # p_y == 1 in fp32 on a third of the pixels
        sat = torch.rand(B, H, W, generator=g) < 0.33
        onehot = torch.nn.functional.one_hot(target, K).permute(0, 3, 1, 2).bool()
        logits = torch.where(onehot & sat.unsqueeze(1), torch.full_like(logits, 60.0), logits)
    logits.requires_grad_()
    crit = getattr(R.losses, loss_name)(dict(cfg))
    loss = crit(logits, target)
    (loss * scale).backward()
    out[name + "_logits"] = logits.detach().numpy().copy()
    out[name + "_target"] = target.numpy().copy()
    out[name + "_cfg"] = np.array(json.dumps({"loss": loss_name, "config": cfg, "scale": scale}))
    out[name + "_loss"] = np.float64(loss.item())
    out[name + "_grad"] = logits.grad.numpy().copy()
    print("%-26s loss %+.7f  grad nan %d of %d" % (name, loss.item(), int(torch.isnan(logits.grad).sum()), logits.grad.numel()))
np.savez_compressed(os.path.join(HERE, "overlap_losses.npz"), **out)
print("wrote overlap_losses.npz %.1f KB" % (os.path.getsize(os.path.join(HERE, "overlap_losses.npz")) / 1024))
