"""Times the geometric-augmentation ingest (csrc/warp.hip) beside the plain ingest kernel it extends, with HIP events, on 8 x 540 x 960 frames of
experiment 3, in one run:
    ingest_u8_pad        catseg_ingest_u8, reflect pad (2, 2): the yardstick
    warp_identity_pad    catseg_ingest_warp_u8 without a matrix, the same window and padding
    warp_affine_crop416  'affine' draws + a 416 x 416 crop window of the 1080 x 1920 canvas
    warp_affine_canvas   'affine' draws on the full 1080 x 1920 canvas, reflect pad (2, 2)
The C ABI is called directly on preallocated outputs (no allocator, no host -> device copy of the parameters inside the timed region); the
inputs rotate through >= 1.5 GB of frame sets, so that no launch finds its frames in the 256 MB last-level cache; the cases are interleaved
in rounds and the medians over all launches are reported with the algorithmic bytes (frames read once + outputs written; for a crop only the
window's share of the frames).
    python tools/time_ingest_warp.py [--rounds 7] [--iters 10] [--out profiles/ingest_warp_time.json]"""
import argparse
import json
import os
import random
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from miccai2021_cataract_semantic_segmentation_amd import _lib  # noqa: E402
from miccai2021_cataract_semantic_segmentation_amd.utils import remap_lut  # noqa: E402
from miccai2021_cataract_semantic_segmentation_amd.utils import geometry as G  # noqa: E402

B, H, W, EXP = 8, 540, 960, 3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ingest_warp_time.json"))
    a = ap.parse_args()
    dev = torch.device("cuda")
    lib, P = _lib.lib, (lambda t: 0 if t is None else t.data_ptr())
    set_bytes = B * H * W * 4
    nsets = int(1.5e9 / set_bytes) + 1
    gen = torch.Generator(device="cuda").manual_seed(0)
    sets = [(torch.randint(0, 256, (B, H, W, 3), dtype=torch.uint8, device=dev, generator=gen),
             torch.randint(0, 36, (B, H, W), dtype=torch.uint8, device=dev, generator=gen)) for _ in range(nsets)]
    lut = torch.from_numpy(remap_lut(EXP)).to(dev)
    rng, pyrng = np.random.RandomState(0), random.Random(0)
    params = G.geometry_from_transforms(["affine"], {})["affine"]
    px = G.crop_px(0.4, 2 * H, 2 * W)
    geo = []                              # per input set: flips, inverse matrices, crop origins (device)
    for _ in range(nsets):
        flips = torch.from_numpy(rng.randint(0, 2, B).astype(np.int32)).to(dev)
        minv = G.affine_inverse(G.sample_affine(B, (H, W), params, rng)[1])[:, :2].reshape(B, 6)
        geo.append((flips, torch.from_numpy(np.ascontiguousarray(minv)).to(dev), torch.from_numpy(G.sample_crops(B, (2 * H, 2 * W), px, pyrng)).to(dev)))

    def outputs(ho, wo):
        return (torch.empty((B, 3, ho, wo), dtype=torch.float32, device=dev), torch.empty((B, ho, wo), dtype=torch.int64, device=dev))

    o_pad, o_crop, o_canvas = outputs(H + 4, W), outputs(px, px), outputs(2 * H + 4, 2 * W)
    st = _lib.stream

    def ingest(k):
        (img, lbl), (fl, _, _) = sets[k], geo[k]
        _lib.check(lib.catseg_ingest_u8(P(img), P(lbl), B, H, W, P(lut), P(fl), 2, 2, None, None, P(o_pad[0]), None, P(o_pad[1]), st()))

    def warp(k, minv, canvas, origin, window, pad, out):
        (img, lbl), fl = sets[k], geo[k][0]
        _lib.check(lib.catseg_ingest_warp_u8(P(img), P(lbl), B, H, W, P(lut), P(fl), P(minv), canvas[0], canvas[1], P(origin), window[0], window[1],
                                             pad, pad, None, None, P(out[0]), None, None, P(out[1]), st()))

    frame_px, out_b = B * H * W, 12 + 8
    cases = {
        "ingest_u8_pad": (ingest, 4.0 * frame_px + out_b * B * (H + 4) * W),
        "warp_identity_pad": (lambda k: warp(k, None, (H, W), None, (H, W), 2, o_pad), 4.0 * frame_px + out_b * B * (H + 4) * W),
        "warp_affine_crop416": (lambda k: warp(k, geo[k][1], (2 * H, 2 * W), geo[k][2], (px, px), 0, o_crop), (4.0 + out_b) * B * px * px),
        "warp_affine_canvas": (lambda k: warp(k, geo[k][1], (2 * H, 2 * W), None, (2 * H, 2 * W), 2, o_canvas),
                               4.0 * frame_px + out_b * B * (2 * H + 4) * 2 * W),
    }
    times = {name: [] for name in cases}
    k = 0
    for name, (fn, _) in cases.items():          # warm-up
        for _ in range(3):
            fn(k % nsets)
            k += 1
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    for _ in range(a.rounds):
        for name, (fn, _) in cases.items():
            for _ in range(a.iters):
                e0.record()
                fn(k % nsets)
                e1.record()
                e1.synchronize()
                times[name].append(e0.elapsed_time(e1) * 1e3)
                k += 1
    res = {"frames": [B, H, W], "experiment": EXP, "crop_px": px, "input_sets": nsets, "input_bytes_rotated": nsets * set_bytes,
           "rounds": a.rounds, "iters_per_round": a.iters, "device": torch.cuda.get_device_name(0), "cases": {}}
    for name, (_, nbytes) in cases.items():
        t = sorted(times[name])
        med = t[len(t) // 2]
        res["cases"][name] = {"median_us": round(med, 2), "min_us": round(t[0], 2), "max_us": round(t[-1], 2), "bytes": nbytes,
                              "GB_per_s": round(nbytes / med * 1e-3, 1)}
        print(json.dumps({name: res["cases"][name]}), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
