"""Times ops.egress_u8 (argmax / clipped argmax + colouring + frame bytes + canvas, one launch) against the same result composed from torch
operations -- argmax (softmax + max + where with a threshold), table indexing, round(img * 255), cat -- on the same GPU in the same run.
HIP events after warm-up; the inputs rotate through sets that together exceed the last-level cache; the two contenders alternate within
every round and the medians over the rounds are reported.  Bytes = P * ld * 4 + the output bytes (the algorithmic count of the kernel);
the fraction is of the 8 TB/s HBM peak.
    python tools/time_egress.py [--rounds 30] [--out profiles/egress_time.json]"""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from miccai2021_cataract_semantic_segmentation_amd import ops  # noqa: E402
from miccai2021_cataract_semantic_segmentation_amd.utils.classes import CLASS_REMAP  # noqa: E402
from miccai2021_cataract_semantic_segmentation_amd.utils.egress import get_remapped_colormap, network_lut, palette_table  # noqa: E402

HBM_PEAK = 8.0e12
K, LD, IGNORE = 25, 28, 25


def torch_composition(rows, lut_l, pal, frame, target, threshold):
    """the same outputs from torch operations: canvas [B, H, n W, 3] uint8, BGR"""
    if threshold > 0:
        score, idx = torch.softmax(rows, -1).max(-1)
        idx = torch.where(score < threshold, torch.full_like(idx, IGNORE), idx)
    else:
        idx = rows.argmax(-1)
    panels = []
    if frame is not None:
        panels.append(torch.round(frame.permute(0, 2, 3, 1).flip(-1) * 255).clamp(0, 255).to(torch.uint8))
    if target is not None:
        panels.append(pal[lut_l[target]])
    panels.append(pal[lut_l[idx]])
    return torch.cat(panels, dim=2) if len(panels) > 1 else panels[0]


def time_case(B, H, W, panels, threshold, rounds, rotate):
    dev = torch.device("cuda")
    g = torch.Generator(device="cuda").manual_seed(0)
    lut = torch.from_numpy(network_lut(3)).to(dev)
    pal = torch.from_numpy(palette_table(get_remapped_colormap(CLASS_REMAP[3]), bgr=True)).to(dev)
    lut_l = lut.long()
    sets = []
    for _ in range(rotate):
        rows = ops.new_act(B, H, W, K, dev, ld=LD, zero=True)
        rows.copy_(torch.randn(B, H, W, K, device=dev, generator=g) * 4)
        frame = torch.rand(B, 3, H, W, device=dev, generator=g) if panels >= 2 else None
        target = torch.randint(0, K + 1, (B, H, W), device=dev, generator=g) if panels >= 3 else None
        sets.append((rows, frame, target))

    def hip(i):
        rows, frame, target = sets[i % rotate]
        return ops.egress_u8(rows, threshold=threshold, ignore_value=IGNORE, lut=lut, palette=pal, frame=frame, bgr=True, target=target)[2]

    def composed(i):
        rows, frame, target = sets[i % rotate]
        return torch_composition(rows, lut_l, pal, frame, target, threshold)

    a, b = hip(0), composed(0)
    same = float((a == b).float().mean())                          # (softmax scores a few ulps apart may clip differently at a threshold)
    for i in range(3):
        hip(i), composed(i)
    torch.cuda.synchronize()
    e0, e1, e2 = (torch.cuda.Event(enable_timing=True) for _ in range(3))
    t_hip, t_torch = [], []
    for i in range(rounds):                                         # interleaved: both see the same machine state
        e0.record()
        hip(i)
        e1.record()
        composed(i)
        e2.record()
        e2.synchronize()
        t_hip.append(e0.elapsed_time(e1) * 1e3)
        t_torch.append(e1.elapsed_time(e2) * 1e3)
    P = B * H * W
    nbytes = P * LD * 4.0 + P * 3.0 * panels
    med_hip, med_torch = float(np.median(t_hip)), float(np.median(t_torch))
    return {"B": B, "H": H, "W": W, "K": K, "ld": LD, "panels": panels, "threshold": threshold, "hip_us": round(med_hip, 2),
            "hip_min_us": round(min(t_hip), 2), "torch_us": round(med_torch, 2), "torch_min_us": round(min(t_torch), 2),
            "speedup": round(med_torch / med_hip, 2), "bytes": nbytes, "GB_per_s": round(nbytes / med_hip * 1e-3, 1),
            "fraction_of_8TBps": round(nbytes / (med_hip * 1e-6) / HBM_PEAK, 3), "bytes_equal_to_torch": same, "rounds": rounds,
            "rotate": rotate}


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=30)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("time_egress: needs the GPU (no number comes from a CPU run)")
    results = []
    for B, H, W in ((1, 544, 960), (4, 1088, 1920)):
        rotate = min(12, max(2, int(1.0e9 / (B * H * W * LD * 4)) + 1))      # sets that together exceed the 256 MB last-level cache
        for panels in (1, 2, 3):
            for threshold in (0.0, 0.9):
                r = time_case(B, H, W, panels, threshold, a.rounds, rotate)
                results.append(r)
                print(json.dumps(r), flush=True)
    if a.out:
        with open(a.out, "w") as f:
            json.dump({"tool": "tools/time_egress.py", "device": torch.cuda.get_device_name(0), "cases": results}, f, indent=1)
