"""Times ops.ensemble_merge (softmax per member + merge + argmax, one launch) with HIP events after warm-up and prints the achieved
HBM rate from the algorithmic byte count (M + 1) * P * K * 4 (+ 8 P for the label map).
    python tools/time_ensemble_merge.py [--members 3] [--classes 25] [--iters 50]"""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from miccai2021_cataract_semantic_segmentation_amd import ops  # noqa: E402


def time_case(M, K, H, W, iters, want_probs, want_labels, rotate):
    dev = torch.device("cuda")
    g = torch.Generator(device="cuda").manual_seed(0)
    # `rotate` input sets, cycled: together far larger than the 256 MB last-level cache, so that no launch finds its input there
    sets = []
    for _ in range(rotate):
        ms = []
        for _ in range(M):
            t = ops.new_act(1, H, W, K, dev, zero=True)
            t.copy_(torch.randn(1, H, W, K, device=dev, generator=g) * 4)
            ms.append(t)
        sets.append(ms)
    for i in range(5):
        ops.ensemble_merge(sets[i % rotate], "mean", want_probs, want_labels)
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    times = []
    for i in range(iters):
        e0.record()
        ops.ensemble_merge(sets[i % rotate], "mean", want_probs, want_labels)
        e1.record()
        e1.synchronize()
        times.append(e0.elapsed_time(e1) * 1e-3)
    times.sort()
    med = times[len(times) // 2]
    P = H * W
    nbytes = 4.0 * (M + (1 if want_probs else 0)) * P * K + (8.0 * P if want_labels else 0.0)
    return {"M": M, "K": K, "H": H, "W": W, "probs": want_probs, "labels": want_labels, "ld": ops.ld_of(sets[0][0]), "median_us": med * 1e6,
            "min_us": times[0] * 1e6, "GB_per_s": nbytes / med * 1e-9, "bytes": nbytes}


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--members", type=int, default=3)
    ap.add_argument("--classes", type=int, default=25)
    ap.add_argument("--iters", type=int, default=50)
    a = ap.parse_args()
    for H, W in ((544, 960), (1088, 1920)):
        rotate = max(2, int(1.5e9 / (a.members * H * W * a.classes * 4)))
        for want_probs, want_labels in ((True, False), (True, True), (False, True)):
            print(json.dumps(time_case(a.members, a.classes, H, W, a.iters, want_probs, want_labels, min(rotate, 12))), flush=True)
