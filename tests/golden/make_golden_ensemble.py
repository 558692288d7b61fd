"""Fixtures for models.Ensemble and the merge kernel, generated with the REAL reference's models/Ensemble.py (members: the reference's
OCRNet, DeepLabv3Plus and EncDec(ResNet18 + UPerNet), experiment 3).
    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_ensemble.py
Writes ensemble.npz (frame, specs + seeds of the members, merged 'mean' output, its argmax), ensemble_member{1,2,3}.npz (each member's
logits; one file each to stay within the size limit of a committed file) and ensemble_merge.npz (merge-only cases on random logits,
stored as seeds + the reference's output)."""
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
from oracle.state import fill_state, spec_of  # noqa: E402
import _ensemble_ref as ER  # noqa: E402  (member configurations and the merge-case generator shared with the tests; no arithmetic is taken from it)

torch.set_num_threads(8)
R = ref_harness.load()
ref_mod = sys.modules[R.models.Ensemble.__module__]


class Normalize:
    """what torchvision's Normalize computes (the harness stubs torchvision.transforms with identities)"""

    def __init__(self, mean, std):
        self.mean, self.std = torch.tensor(mean).view(3, 1, 1), torch.tensor(std).view(3, 1, 1)

    def __call__(self, t):
        return (t - self.mean) / self.std


ref_mod.Normalize = Normalize
SEEDS = (500, 501, 502)


def save(name, **arrs):
    path = os.path.join(HERE, name + ".npz")
    np.savez_compressed(path, **arrs)
    size = os.path.getsize(path)
    print("wrote %s  %.1f KB" % (name, size / 1024))
    assert size <= 1 << 20, "fixture %s is larger than 1 MiB" % name


def whole_ensemble():
    torch.manual_seed(5)
    ens = R.models.Ensemble({"merge": "mean", "members": ER.member_configs()}, 3)
    assert ens.members_names == ["OCRNet", "DeepLabv3Plus", "EncDec"], ens.members_names
    specs, seen, logits = [], [], []
    for model, seed in zip(ens.members, SEEDS):
        spec = spec_of(model.state_dict())
        model.load_state_dict(fill_state(spec, seed))
        model.eval()
        specs.append(spec)
        model.register_forward_pre_hook(lambda mod, args: seen.append(args[0].clone()))
        model.register_forward_hook(lambda mod, args, out: logits.append(out.clone()))
    x = torch.rand(1, 3, 64, 96, generator=torch.Generator().manual_seed(510))
    with torch.no_grad():
        merged = ens(x)
    assert len(seen) == 3 and torch.equal(seen[0], x) and torch.equal(seen[1], x)
    assert not torch.equal(seen[2], x) and torch.equal(seen[2][0], Normalize(ER.IMAGENET_MEAN, ER.IMAGENET_STD)(x[0])), \
        "the UPerNet member must see the normalised frame"
    assert merged.shape == (1, 25, 64, 96) and all(z.shape == merged.shape for z in logits)
    save("ensemble", x=x.numpy().copy(), seeds=np.array(SEEDS), specs=np.array(json.dumps(specs)), merged=merged.numpy().copy(),
         argmax=merged.argmax(1).numpy().astype(np.uint8))
    for i, z in enumerate(logits):
        save("ensemble_member%d" % (i + 1), logits=z.numpy().copy())


def merge_only():
    """M = 3 random logit tensors of P = 4096 pixels (1 x K x 64 x 64, randn * 4) per K: the reference's own merge lines on them"""
    out = {}
    for K in (8, 17, 25):
        zs = ER.merge_case_logits(K)
        stacked = torch.stack([torch.nn.Softmax2d()(z) for z in zs])        # models/Ensemble.py:66,69,71
        out["mean_K%d" % K] = torch.mean(stacked, dim=0).numpy().copy()
    save("ensemble_merge", **out)


if __name__ == "__main__":
    merge_only()
    whole_ensemble()
