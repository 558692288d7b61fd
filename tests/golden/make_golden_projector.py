"""Fixture for the contrastive projector, every value recorded from the REAL reference (models/Projector.py, the model constructors with
the 'projector' key, utils/torch_utils.t_normalise_confusion_matrix).
    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_projector.py"""
import contextlib
import io
import json
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
import ref_harness  # noqa: E402
from oracle.state import fill_state, spec_of  # noqa: E402

R = ref_harness.load()
# models/EncDec.py takes its names from `from models import *`, and models/__init__.py reaches it (through Ensemble) before it has bound
# the Projector class: the name is then the SUBMODULE and EncDec(config with 'projector') raises "'module' object is not callable".
# The class is put in its place here, in the imported module's namespace (nothing is written into the reference tree).
if not isinstance(sys.modules["models.EncDec"].Projector, type):
    sys.modules["models.EncDec"].Projector = R.models.Projector
out = {}

# ---- the Projector alone: state-dict spec, outputs and parameter gradients of sum(out * r) on two inputs
CONFIGS = [{}, {"mlp": [[1, 256, 1]]}, {"mlp": [[3, 8, 2], [1, 6, 1]], "d": 4}]
SHAPES = [(2, 5, 9, 11), (2, 5, 8, 12)]
out["configs"] = np.array(json.dumps(CONFIGS))
out["shapes"] = np.array(SHAPES)
for ci, cfg in enumerate(CONFIGS):
    with contextlib.redirect_stdout(io.StringIO()):
        proj = R.models.Projector(dict(cfg, c_in=5))
    spec = spec_of(proj.state_dict())
    proj.load_state_dict(fill_state(spec, 700 + ci))
    out["p%d_spec" % ci] = np.array(json.dumps(spec))
    out["p%d_seed" % ci] = np.array(700 + ci)
    for si, shape in enumerate(SHAPES):
        g = torch.Generator().manual_seed(710 + 10 * ci + si)
        x = torch.randn(shape, generator=g)
        proj.zero_grad()
        y = proj(x)
        r = torch.randn(y.shape, generator=g)
        (y * r).sum().backward()
        tag = "p%d_s%d_" % (ci, si)
        # (x and r are the two draws of torch.Generator().manual_seed(710 + 10 * ci + si), randn(shape) then randn(y.shape): not stored)
        out[tag + "y"] = y.detach().numpy().copy()
        for name, p in proj.named_parameters():
            out[tag + "grad_" + name] = p.grad.numpy().copy()

# ---- the output tuples of the models with the key, on the tiny fixture input
PROJ = {"mlp": [[1, 16, 1]], "d": 8}
x = torch.rand(2, 3, 64, 64, generator=torch.Generator().manual_seed(730))
tuples = {}
with contextlib.redirect_stdout(io.StringIO()):
    nets = {
        "ocrnet_r50": R.models.OCRNet({"backbone": "resnet50", "out_stride": 8, "pretrained": False, "projector": dict(PROJ)}, 3),
        "deeplabv3plus_r50": R.models.DeepLabv3Plus({"backbone": "resnet50", "out_stride": 16, "pretrained": False, "projector": dict(PROJ)}, 2),
        "encdec_r18": R.models.EncDec({"encoder": {"model": "ResNet18", "pretrained": False}, "decoder": {"model": "UPerNet"},
                                       "projector": dict(PROJ)}, 1),
    }
for name, net in nets.items():
    rec = {"projector_keys": [k for k in net.state_dict() if k.startswith("projector_model.")], "c_in": net.projector_model.c_in}
    for mode in ("train", "eval"):
        net.train() if mode == "train" else net.eval()
        with torch.no_grad():
            res = net(x)
        rec[mode] = [list(t.shape) for t in res]
    tuples[name] = rec
out["tuples"] = np.array(json.dumps(tuples))
out["tuples_x_seed"] = np.array(730)

# ---- t_normalise_confusion_matrix, both modes, on a matrix with an all-zero row and an all-zero column
cm = torch.randint(0, 50, (6, 6), generator=torch.Generator().manual_seed(740), dtype=torch.int32)
cm[2, :] = 0
cm[:, 4] = 0
out["cm"] = cm.numpy().copy()
out["cm_row"] = R.utils.t_normalise_confusion_matrix(cm, "row").numpy().copy()
out["cm_col"] = R.utils.t_normalise_confusion_matrix(cm, "col").numpy().copy()
np.savez_compressed(os.path.join(HERE, "projector.npz"), **out)
print("wrote projector fixture", {k: v["train"] for k, v in tuples.items()})
