"""Times RandAugment's photometric operations (csrc/augment.hip behind catseg_aug_color_op, op codes 4 ... 8) beside the legacy contrast
operation (code 1, the yardstick: a reduction pre-pass, then a read-modify-write pass) with HIP events, on 8 x 544 x 960 x 3 uint8 frames, in
one run.  Every operation is timed on frames of natural statistics (smooth structure + noise, a skewed histogram) and on constant frames
(all histogram counts in one bin).  The C ABI is called directly (no allocator, no host -> device copy inside the timed region); the frames
rotate through >= 1.5 GB per kind, so that no launch finds its frames in the 256 MB last-level cache; the operations work in place, so
each frame set is restored from its master after its timed call, outside the events.  The cases are interleaved in rounds and the medians
over all calls are reported with the algorithmic bytes from the shapes (pre-pass read + apply read and write; sharpness: the source copy's
write and read as well).
    python tools/time_randaugment.py [--rounds 7] [--iters 10] [--out profiles/randaugment_time.json]"""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from miccai2021_cataract_semantic_segmentation_amd import _lib, ops  # noqa: E402

B, H, W = 8, 544, 960
OPS = {"contrast": (1, 1.31), "autocontrast": (4, 0.0), "equalize": (5, 0.0), "posterize": (6, 4.0), "solarize": (7, 178.5), "sharpness": (8, 1.45)}


def natural_frames(seed):
    """smooth low-frequency structure plus sensor-like noise, gamma-skewed (most pixels dark, as a surgical video frame): uint8 [B, H, W, 3]"""
    rng = np.random.default_rng(seed)
    coarse = torch.from_numpy(rng.random((B, 3, H // 32, W // 32), dtype=np.float32))
    smooth = torch.nn.functional.interpolate(coarse, size=(H, W), mode="bicubic", align_corners=False).clamp_(0, 1)
    img = smooth ** 2.2 * 235 + torch.from_numpy(rng.normal(0, 4, (B, 3, H, W)).astype(np.float32)) + 8
    return img.clamp_(0, 255).permute(0, 2, 3, 1).contiguous().to(torch.uint8)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "randaugment_time.json"))
    a = ap.parse_args()
    dev = torch.device("cuda")
    lib, st = _lib.lib, _lib.stream
    set_bytes = B * H * W * 3
    nsets = int(1.5e9 / set_bytes) + 1
    masters = {"natural": natural_frames(0).to(dev), "constant": torch.full((B, H, W, 3), 93, dtype=torch.uint8, device=dev)}
    sets = {kind: [m.clone() for _ in range(nsets)] for kind, m in masters.items()}
    ws_bytes = {None: ops.aug_color_workspace_bytes(B, H, W), "lut": ops.aug_color_workspace_bytes(B, H, W, "lut"),
                "full": ops.aug_color_workspace_bytes(B, H, W, "full")}
    ws = torch.empty(ws_bytes["full"], dtype=torch.uint8, device=dev)
    frame_b = float(set_bytes)
    cases = {}
    for name, (code, value) in OPS.items():
        op = torch.full((B,), code, dtype=torch.int32, device=dev)
        fac = torch.full((B,), value, dtype=torch.float32, device=dev)
        size = ws_bytes[None if code < 4 else ("full" if code == 8 else "lut")]
        nbytes = 5.0 * frame_b if code == 8 else 3.0 * frame_b          # reads + writes of whole frames, from the shapes
        if code in (6, 7):
            nbytes = 2.0 * frame_b                                       # (their blocks return from the pre-pass at once)
        for kind in masters:
            def call(k, kind=kind, op=op, fac=fac, size=size):
                _lib.check(lib.catseg_aug_color_op(sets[kind][k].data_ptr(), B, H, W, op.data_ptr(), fac.data_ptr(), ws.data_ptr(), size, st()))
            cases["%s/%s" % (name, kind)] = (call, kind, nbytes)
    times = {name: [] for name in cases}
    k = 0
    for name, (fn, kind, _) in cases.items():          # warm-up
        for _ in range(3):
            fn(k % nsets)
            sets[kind][k % nsets].copy_(masters[kind])
            k += 1
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    for _ in range(a.rounds):
        for name, (fn, kind, _) in cases.items():
            for _ in range(a.iters):
                e0.record()
                fn(k % nsets)
                e1.record()
                e1.synchronize()
                times[name].append(e0.elapsed_time(e1) * 1e3)
                sets[kind][k % nsets].copy_(masters[kind])     # in-place operations: the set gets its statistics back, untimed
                k += 1
    res = {"frames": [B, H, W, 3], "input_sets_per_kind": nsets, "input_bytes_rotated_per_kind": nsets * set_bytes, "rounds": a.rounds,
           "iters_per_round": a.iters, "device": torch.cuda.get_device_name(0), "workspace_bytes": {str(k_): v for k_, v in ws_bytes.items()},
           "yardstick": "contrast", "cases": {}}
    med = {}
    for name, (_, kind, nbytes) in cases.items():
        t = sorted(times[name])
        med[name] = t[len(t) // 2]
        res["cases"][name] = {"median_us": round(med[name], 2), "min_us": round(t[0], 2), "max_us": round(t[-1], 2), "bytes": nbytes,
                              "GB_per_s": round(nbytes / med[name] * 1e-3, 1), "ratio_to_contrast": round(med[name] / med["contrast/" + kind], 3)}
        print(json.dumps({name: res["cases"][name]}), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
