"""Semi-supervised fixtures from the REAL reference (losses/SemiSupervisedLoss.py, utils/semi_utis.py, utils/utils.py:419-436), see
make_golden.py.

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_semisup.py

Writes semisup.npz (inputs of every case, every loss, the BalancedConcatDataset indices, the pseudo_colorjitter arguments) and one
semisup_<case>.npz per loss case with its logits gradients (dense float32: they do not compress, and one file would pass 1 MiB).

Inputs: logits are multiples of 1/16 in [-4, 4) kept as int8; the B = 3 form of a case is its first three frames (split 1 + 2).  Frame 0
(labelled at B = 4 and B = 3) alone holds class ONLY_LAB, frame 2 (pseudo-labelled at both) alone holds class ONLY_ULAB, class EMPTY is
nowhere: a wrong split changes Lovasz's set of present classes.  Experiments 2 / 3 also carry ignore-labelled pixels (experiment 1 has no
ignore label)."""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
import ref_harness  # noqa: E402

R = ref_harness.load()
from losses.SemiSupervisedLoss import SemiSupervisedLoss  # noqa: E402  (the reference's own module: ref_harness put its tree on sys.path)
from utils.semi_utis import BalancedConcatDataset  # noqa: E402

H, W = 24, 36
ONLY_LAB, ONLY_ULAB, EMPTY = 2, 5, 6
CHANNELS = {1: 8, 2: 17, 3: 25}        # (the label values count one more in experiments 2 / 3: the ignore id)


def lovasz(exp, w_lab, w_ulab):
    return {"experiment": exp, "labeled": {"name": "LovaszSoftmax", "weight": w_lab}, "unlabeled": {"name": "LovaszSoftmax", "weight": w_ulab}}


def two_scale(final_weight, weight):
    return {"name": "TwoScaleLoss", "weight": weight, "interm": {"name": "LovaszSoftmax", "args": [], "weight": 0.4},
            "final": {"name": "LovaszSoftmax", "args": [], "weight": final_weight}}


CASES = [
    # name, experiment, config, list form, batch sizes
    ("lovasz_e2", 2, lambda: lovasz(2, 1.0, 0.5), False, (4, 3)),
    ("lovasz_e1", 1, lambda: lovasz(1, 0.75, 1.5), False, (4, 3)),
    ("ohem_e3", 3, lambda: {"experiment": 3, "labeled": {"name": "OhemCrossEntropy", "weight": 1.0, "min_kept": 200, "thresh": 0.004},
                            "unlabeled": {"name": "OhemCrossEntropy", "weight": 0.25, "min_kept": 200, "thresh": 0.004}}, False, (4,)),
    ("two_scale_e2", 2, lambda: {"experiment": 2, "labeled": two_scale(1.0, 1.0), "unlabeled": two_scale(0.7, 0.5)}, True, (4,)),
]


def make_target(exp, g):
    K = CHANNELS[exp]
    common = [c for c in range(K) if c not in (ONLY_LAB, ONLY_ULAB, EMPTY)]
    if exp in (2, 3):
        common.append(K)                 # the ignore id
    pick = torch.randint(0, len(common), (4, H // 4, W // 4), generator=g)
    t = torch.tensor(common)[pick].repeat_interleave(4, 1).repeat_interleave(4, 2).contiguous()
    t[0, 3:9, 5:17] = ONLY_LAB
    t[2, 10:19, 20:31] = ONLY_ULAB
    if exp in (2, 3):                    # ignore-labelled pixels in both halves, at B = 4 and at B = 3
        t[0, 12:16, 0:8] = K
        t[2, 0:4, 0:8] = K
    return t


main, grads = {}, {}
for ci, (name, exp, cfg, as_list, batches) in enumerate(CASES):
    g = torch.Generator().manual_seed(500 + ci)
    K = CHANNELS[exp]
    q = torch.randint(-64, 64, (4, K, H, W), generator=g).to(torch.int8)
    target = make_target(exp, g)
    main[name + "_logits_q"] = q.numpy()
    main[name + "_target"] = target.numpy().astype(np.uint8)
    if as_list:
        qi = torch.randint(-64, 64, (4, K, H // 2, W // 2), generator=g).to(torch.int8)
        main[name + "_interm_q"] = qi.numpy()
    grads[name] = {}
    for B in batches:
        for flag in (False, True):
            final = (q[:B].float() / 16).requires_grad_()
            interm = (qi[:B].float() / 16).requires_grad_() if as_list else None
            crit = SemiSupervisedLoss(cfg())
            loss = crit([interm, final] if as_list else final, target[:B], run_on_labeled_validation=flag)
            loss.backward()
            tag = "%s_b%d_%s" % (name, B, "valid" if flag else "train")
            main[tag + "_loss"] = np.float64(loss.item())
            grads[name][tag + "_grad"] = final.grad.numpy().copy()
            if as_list:
                grads[name][tag + "_ginterm"] = interm.grad.numpy().copy()
            print(tag, float(loss), "present:", sorted(set(target[:B].reshape(-1).tolist())))

# utils/semi_utis.py:6-23: which item of each member item i holds, for member lengths 5 and 7
members = [list(range(5)), list(range(100, 107))]
ds = BalancedConcatDataset(*members)
main["concat_len"] = np.int64(len(ds))
main["concat_items"] = np.array([ds[i] for i in range(len(ds))], dtype=np.int64)

# utils/utils.py:419-436: the arguments parse_transform_list hands to ColorJitter / RandomApply, captured by recording stand-ins
import utils.utils as ref_utils_module  # noqa: E402
seen = []


class _ColorJitter:
    def __init__(self, **kw):
        self.kw = kw


class _RandomApply:
    def __init__(self, transforms, p):
        seen.append((transforms[0].kw, p, len(transforms)))


ref_utils_module.ColorJitter, ref_utils_module.RandomApply = _ColorJitter, _RandomApply
for s in (1, 2, 3, None):
    tl = ["pseudo_colorjitter"] + ([{"strength": s}] if s is not None else [])
    ref_utils_module.parse_transform_list(tl, {}, 18)
    kw, p, n = seen[-1]
    assert n == 1 and sorted(kw) == ["brightness", "contrast", "hue", "saturation"]
    main["jitter_s%s" % ("default" if s is None else s)] = np.array(
        [kw["brightness"], kw["contrast"], kw["saturation"], kw["hue"], (p, p)], dtype=np.float64)

np.savez_compressed(os.path.join(HERE, "semisup.npz"), **main)
print("wrote semisup.npz %.1f KB" % (os.path.getsize(os.path.join(HERE, "semisup.npz")) / 1024))
for name, arrays in grads.items():
    path = os.path.join(HERE, "semisup_%s.npz" % name)
    np.savez_compressed(path, **arrays)
    print("wrote %s %.1f KB" % (os.path.basename(path), os.path.getsize(path) / 1024))
