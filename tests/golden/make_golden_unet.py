"""Fixture for the reference's UNet (models/UNet.py:6-63: double_conv levels, MaxPool2d(2), bilinear Upsample with align_corners=True,
torch.cat skip junctions, a 1x1 class layer), generated with the REAL reference:

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_unet.py

task 2 (18 logit channels: the reference's UNet keeps the 'ignore' entry), input 2 x 3 x 40 x 56 (bottleneck 5 x 7: the resize scales
(h - 1) / (2 h - 1) are non-trivial and H != W).  Inputs / labels / weights are regenerated from seeds; the fixture stores the state-dict
spec, the logits of the first step (every 4th row and column, three full rows, sums), the loss of two Adam steps, per-parameter gradient
norms / sums and the full gradients of conv_last.bias and dconv_up1.0.bias.
"""
import json
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
import ref_harness  # noqa: E402
from _unet_ref import make_inputs, summarise  # noqa: E402
from oracle.state import fill_state, spec_of  # noqa: E402

SEED, SHAPE, EXP = 910, (2, 3, 40, 56), 2


if __name__ == "__main__":
    torch.set_num_threads(8)
    R = ref_harness.load()
    torch.manual_seed(SEED)
    model = R.models.UNet({}, EXP)
    spec = spec_of(model.state_dict())
    model.load_state_dict(fill_state(spec, SEED))
    x, lbl = make_inputs(SEED, SHAPE, model.num_classes)
    out = {"seed": np.array(SEED), "shape": np.array(SHAPE), "spec": np.array(json.dumps(spec)), "num_classes": np.array(model.num_classes)}
    model.train()
    L = R.losses.LovaszSoftmax({"experiment": EXP})
    opt = torch.optim.Adam(model.parameters(), lr=1e-3)
    losses = []
    for s in range(2):
        opt.zero_grad()
        y = model(x)
        loss = L(y, lbl)
        loss.backward()
        if s == 0:
            for k, v in summarise(y).items():
                out["train_" + k] = v
            out["train_scale"] = np.array(float(y.abs().max()))
            names = [k for k, _ in model.named_parameters()]
            out["grad_names"] = np.array(json.dumps(names))
            out["grad_norms"] = np.array([float(p.grad.double().norm()) for _, p in model.named_parameters()])
            out["grad_sums"] = np.array([float(p.grad.double().sum()) for _, p in model.named_parameters()])
            for k in ("conv_last.bias", "dconv_up1.0.bias"):
                out["g:" + k] = dict(model.named_parameters())[k].grad.numpy().copy()
        opt.step()
        losses.append(float(loss))
    out["losses"] = np.array(losses)
    path = os.path.join(HERE, "unet_e2_tiny.npz")
    np.savez_compressed(path, **out)
    print("wrote %s %.1f KB; losses %s; scale %.4f" % (path, os.path.getsize(path) / 1024, losses, float(out["train_scale"])))
