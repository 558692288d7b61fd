"""Times the frequency-weighted crop pick (csrc/cropfreq.hip: two launches, row sums + pick) beside the ingest launch of the same batch
(catseg_ingest_warp_u8 reading the picked origins from device memory), with HIP events, on 8 x 540 x 960 frames of experiment 2, in one run:
    pick_frame_px192      the pick on the frames themselves (no affine): px 192, region 348 x 348
    warp_frame_crop192    the ingest of the 192 x 192 windows at the picked origins
    pick_canvas_px416     the pick on the 1080 x 1920 canvas of the 'affine' draws: px 416, region 664 x 664
    warp_canvas_crop416   the ingest of the 416 x 416 windows at the picked origins
The C ABI is called directly on preallocated outputs and workspace (no allocator, no host -> device copy inside the timed region); the inputs
rotate through >= 1.5 GB of frame sets, so that no launch finds its frames in the 256 MB last-level cache; the cases are interleaved in rounds
and the medians over all launches are reported with the algorithmic bytes: for the pick the region's label bytes read once plus the row sums
written and read; for the ingest the window's share of the frames plus the outputs.  The class table is synthetic (a geometric spread of
frequencies over the 18 classes): the time does not depend on its values.
    python tools/time_cropfreq.py [--rounds 7] [--iters 10] [--out profiles/cropfreq_time.json]"""
import argparse
import json
import os
import random
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from miccai2021_cataract_semantic_segmentation_amd import _lib, ops  # noqa: E402
from miccai2021_cataract_semantic_segmentation_amd.utils import remap_lut  # noqa: E402
from miccai2021_cataract_semantic_segmentation_amd.utils import geometry as G  # noqa: E402

B, H, W, EXP = 8, 540, 960, 2


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "cropfreq_time.json"))
    a = ap.parse_args()
    dev = torch.device("cuda")
    lib, P = _lib.lib, (lambda t: 0 if t is None else t.data_ptr())
    set_bytes = B * H * W * 4
    nsets = int(1.5e9 / set_bytes) + 1
    gen = torch.Generator(device="cuda").manual_seed(0)
    sets = [(torch.randint(0, 256, (B, H, W, 3), dtype=torch.uint8, device=dev, generator=gen),
             torch.randint(0, 36, (B, H, W), dtype=torch.uint8, device=dev, generator=gen)) for _ in range(nsets)]
    lut = torch.from_numpy(remap_lut(EXP)).to(dev)
    freqs = np.float32(0.5) ** np.arange(1, 19, dtype=np.float32)
    freqs[-1] *= 2
    wq = G.freq_weight_table(freqs / freqs.sum())[0]
    table = ops.crop_freq_table(wq, dev)
    rng, pyrng = np.random.RandomState(0), random.Random(0)
    params = G.geometry_from_transforms(["affine"], {})["affine"]
    shapes = {"frame": ((H, W), G.crop_px(0.4, H, W)), "canvas": ((2 * H, 2 * W), G.crop_px(0.4, 2 * H, 2 * W))}
    regions = {k: G.crop_freq_region(c[0], c[1], px) for k, (c, px) in shapes.items()}
    for k, (c, px) in shapes.items():
        G.check_freq_weights(wq, regions[k][1] * regions[k][2])
    geo = []                              # per input set: flips, inverse matrices, m53 (device)
    for _ in range(nsets):
        flips = torch.from_numpy(rng.randint(0, 2, B).astype(np.int32)).to(dev)
        minv = G.affine_inverse(G.sample_affine(B, (H, W), params, rng)[1])[:, :2].reshape(B, 6)
        m53 = torch.tensor(G.freq_m53(G.sample_freq_u(B, pyrng)), dtype=torch.int64, device=dev)
        geo.append((flips, torch.from_numpy(np.ascontiguousarray(minv)).to(dev), m53))
    origins = {k: [torch.zeros((B, 2), dtype=torch.int32, device=dev) for _ in range(nsets)] for k in shapes}
    ws_bytes = {k: lib.catseg_crop_freq_workspace(B, c[0], c[1], px) for k, (c, px) in shapes.items()}
    ws = {k: torch.empty(n // 8, dtype=torch.int64, device=dev) for k, n in ws_bytes.items()}
    outs = {k: (torch.empty((B, 3, px, px), dtype=torch.float32, device=dev), torch.empty((B, px, px), dtype=torch.int64, device=dev))
            for k, (_, px) in shapes.items()}
    st = _lib.stream

    def pick(which, k):
        (_, lbl), (fl, minv, m53), (c, px) = sets[k], geo[k], shapes[which]
        _lib.check(lib.catseg_crop_freq_pick(P(lbl), B, H, W, P(lut), P(fl), P(minv) if which == "canvas" else None, c[0], c[1], px, P(table), P(m53),
                                             P(origins[which][k]), None, None, P(ws[which]), ws_bytes[which], st()))

    def warp(which, k):
        (img, lbl), (fl, minv, _), (c, px), out = sets[k], geo[k], shapes[which], outs[which]
        _lib.check(lib.catseg_ingest_warp_u8(P(img), P(lbl), B, H, W, P(lut), P(fl), P(minv) if which == "canvas" else None, c[0], c[1],
                                             P(origins[which][k]), px, px, 0, 0, None, None, P(out[0]), None, None, P(out[1]), st()))

    for which in shapes:                  # the origins the timed ingest launches read: picked once per input set
        for k in range(nsets):
            pick(which, k)
    torch.cuda.synchronize()

    def pick_bytes(which):
        _, rh, rw = regions[which]
        return float(B * rh * rw + 2 * 8 * B * rh + B * rw)

    cases = {
        "pick_frame_px192": (lambda k: pick("frame", k), pick_bytes("frame")),
        "warp_frame_crop192": (lambda k: warp("frame", k), (4.0 + 12 + 8) * B * shapes["frame"][1] ** 2),
        "pick_canvas_px416": (lambda k: pick("canvas", k), pick_bytes("canvas")),
        "warp_canvas_crop416": (lambda k: warp("canvas", k), (4.0 + 12 + 8) * B * shapes["canvas"][1] ** 2),
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
    res = {"frames": [B, H, W], "experiment": EXP, "crop_px": {k: px for k, (_, px) in shapes.items()},
           "regions": {k: [r[1], r[2]] for k, r in regions.items()}, "input_sets": nsets, "input_bytes_rotated": nsets * set_bytes,
           "rounds": a.rounds, "iters_per_round": a.iters, "device": torch.cuda.get_device_name(0),
           "note": "pick_* = both launches of catseg_crop_freq_pick between one pair of events; bytes of a pick = region label bytes once + "
                   "row sums written and read + one region row per frame again",
           "cases": {}}
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
