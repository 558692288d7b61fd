"""Times PointRend's eval-mode forward (csrc/pointrend.hip, ops.pointrend_refine) at configuration 5's shape:

    python3 tools/time_pointrend.py [--batch 4] [--height 1088] [--width 1920] [--rounds 5] [--reps 3] [--out profiles/pointrend_infer_time.json]

Per encoder (ResNet50, ResNeXt101) and k0 (8192, 32768), experiment 3 (K = 25):
  * every new kernel of the last refinement step in microseconds (50 back-to-back calls of the C entry point per timed window, arguments
    built beforehand) and as a fraction of 8 TB/s for the bytes its shapes imply;
  * the refinement stage (ops.pointrend_refine) against the same stage composed from torch device operations (F.interpolate, torch.topk,
    F.grid_sample, F.conv1d, scatter_), interleaved in every round;
  * the whole eval forward against the same encoder with the UPerNet decoder.
Device events around every timed window, three inputs rotate in every comparison, medians over the rounds."""
import argparse
import json
import os
import statistics
import sys

import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from miccai2021_cataract_semantic_segmentation_amd import ops  # noqa: E402
from miccai2021_cataract_semantic_segmentation_amd.models import EncDec  # noqa: E402

HBM = 8e12


def timed(fn, n):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for i in range(n):
        fn(i)
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / n


def interleaved(fns, rounds, reps):
    """{name: median ms}; the candidates alternate inside every round"""
    for fn in fns.values():
        fn(0)
    ts = {k: [] for k in fns}
    for _ in range(rounds):
        for k, fn in fns.items():
            ts[k].append(timed(fn, reps))
    return {k: round(statistics.median(v), 4) for k, v in ts.items()}


def torch_refine(seg, feats, head, k0, steps):
    """the refinement stage as the reference writes it, on the device (NCHW)"""
    for _ in range(steps):
        seg = F.interpolate(seg, scale_factor=2, mode="bilinear", align_corners=False)
        top2 = torch.topk(seg, 2, dim=1)[0]
        n, c, h, w = seg.shape
        idx = torch.topk((top2[:, 1] - top2[:, 0]).view(n, h * w), min(h * w, k0), dim=1)[1]
        pts = torch.stack([(0.5 / w) + (idx % w).float() / w, (0.5 / h) + (idx // w).float() / h], 2)
        grid = (2.0 * pts - 1.0).unsqueeze(2)
        coarse = F.grid_sample(seg, grid, align_corners=False).squeeze(3)
        x = torch.cat([F.grid_sample(f, grid, align_corners=False).squeeze(3) for f in feats[::-1]] + [coarse], 1)
        for wt, b in head["fc"]:
            x = torch.cat([F.relu(F.conv1d(x, wt, b)), coarse], 1)
        seg = seg.reshape(n, c, h * w).scatter_(2, idx.unsqueeze(1).expand(-1, c, -1), F.conv1d(x, *head["predictor"])).view(n, c, h, w)
    return seg


def kernel_times(segs, feats, k0, rounds, launches=50):
    """the new kernels of the LAST refinement step, each timed as `launches` back-to-back calls of its C entry point between two device
    events (arguments built beforehand: no allocation, no wrapper in the window), three input sets in rotation, candidates interleaved per
    round; segs: three coarse logit tensors of the stage"""
    import ctypes
    from miccai2021_cataract_semantic_segmentation_amd import _lib
    lib, st = _lib.lib, _lib.stream()
    N, _, _, K = segs[0].shape
    Kq, Cf = (K + 3) // 4 * 4, sum(f.shape[-1] for f in feats)
    sets = []
    for seg in segs:
        mid = ops.bilinear_fwd(seg, 2 * seg.shape[1], 2 * seg.shape[2], False)
        up, unc = ops.pointrend_upsample2x(mid)
        idx = ops.pointrend_topk(unc, k0)
        _, h, w, _ = up.shape
        k = idx.shape[1]
        x = torch.empty((N * k, Cf + Kq), device="cuda")
        extra = [torch.empty((N * k, 256 + Kq), device="cuda") for _ in range(2)]
        rows = torch.randn(N * k, Kq, device="cuda")
        ws = torch.empty(lib.catseg_pointrend_topk_workspace(N, h * w), dtype=torch.uint8, device="cuda")
        d = _lib.PointrendGatherDesc()
        for i, s in enumerate(list(feats[::-1]) + [up]):
            d.src[i], d.ld[i], d.H[i], d.W[i], d.C[i] = s.data_ptr(), ops.ld_of(s), s.shape[1], s.shape[2], s.shape[3]
        d.n_sources, d.idx, d.N, d.k, d.h, d.w, d.out, d.ld_out, d.n_extra = 5, idx.data_ptr(), N, k, h, w, x.data_ptr(), x.stride(0), 2
        for i, e in enumerate(extra):
            d.extra[i], d.extra_ld[i], d.extra_off[i] = e.data_ptr(), e.stride(0), 256
        sets.append(dict(up=up, unc=unc, idx=idx, x=x, extra=extra, rows=rows, ws=ws, d=d, h=h, w=w, k=k))
    calls = {
        "uncertainty": lambda z: lib.catseg_pointrend_uncertainty(z["up"].data_ptr(), ops.ld_of(z["up"]), z["unc"].data_ptr(), z["unc"].numel(), K, st),
        "topk": lambda z: lib.catseg_pointrend_topk(z["unc"].data_ptr(), N, z["h"] * z["w"], z["k"], z["idx"].data_ptr(), z["ws"].data_ptr(), z["ws"].numel(), st),
        "gather": lambda z: lib.catseg_pointrend_gather(ctypes.byref(z["d"]), st),
        "scatter": lambda z: lib.catseg_pointrend_scatter(z["rows"].data_ptr(), Kq, z["idx"].data_ptr(), N, z["k"], z["h"] * z["w"], z["up"].data_ptr(),
                                                          ops.ld_of(z["up"]), K, st),
    }
    ms = interleaved({n: (lambda i, f=f: _lib.check(f(sets[i % 3]))) for n, f in calls.items()}, rounds, launches)
    h, w, k = sets[0]["h"], sets[0]["w"], sets[0]["k"]
    # gather: what it writes, plus what it reads -- four taps per point and source, but no more than the sources hold (taps of neighbouring
    # points fall on the same pixels of the coarse stages and come from cache)
    srcs = list(feats) + [sets[0]["up"]]
    taps = sum(min(4.0 * N * k * s.shape[-1], float(s.numel())) for s in srcs)
    bytes_ = {"uncertainty": 4.0 * N * h * w * (K + 1), "topk": 4.0 * (6 * N * h * w + N * k),
              "gather": 4.0 * (N * k * (Cf + 3 * Kq) + taps), "scatter": 8.0 * N * k * K}
    return {n: {"us": round(1e3 * ms[n], 2), "fraction_of_8TBs": round(bytes_[n] / (ms[n] * 1e-3) / HBM, 4)} for n in bytes_}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=4)
    ap.add_argument("--height", type=int, default=1088)
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--encoders", default="ResNet50,ResNeXt101")
    ap.add_argument("--out", default="profiles/pointrend_infer_time.json")
    a = ap.parse_args()
    gen = torch.Generator().manual_seed(0)
    xs = [torch.rand(a.batch, 3, a.height, a.width, generator=gen).cuda() for _ in range(3)]
    res = {"shape": [a.batch, 3, a.height, a.width], "experiment": 3, "rounds": a.rounds, "reps": a.reps, "device": torch.cuda.get_device_name(0), "runs": []}
    for enc in a.encoders.split(","):
        for k0 in (8192, 32768):
            torch.manual_seed(0)
            cfg = {"encoder": {"model": enc, "pretrained": False}}
            pr = EncDec(dict(cfg, decoder={"model": "PointRend", "pr_train_num_pts": 196, "pr_subdivision_num_pts": k0}), 3).cuda().eval()
            up = EncDec(dict(cfg, decoder={"model": "UPerNet"}), 3).cuda().eval()
            torch.nn.init.normal_(pr.dec_model.point_head.predictor.weight, std=0.05)      # (the point logits matter: the second step selects other pixels)
            pr.get_features = up.get_features = False
            with torch.no_grad():
                whole = interleaved({"pointrend": lambda i: pr(xs[i % 3]), "upernet": lambda i: up(xs[i % 3])}, a.rounds, a.reps)
                # the stage's inputs, from one forward of the network per rotating input
                seen, refine = [], ops.pointrend_refine
                ops.pointrend_refine = lambda seg, feats, head, k, steps, record=None: seen.append((seg, feats, head)) or refine(seg, feats, head, k, steps)
                try:
                    for x in xs:
                        pr(x)
                finally:
                    ops.pointrend_refine = refine
                tin = [(sg.permute(0, 3, 1, 2).contiguous(), [f.permute(0, 3, 1, 2).contiguous() for f in ft]) for sg, ft, _ in seen]
                head = seen[0][2]
                stage = interleaved({"hip": lambda i: ops.pointrend_refine(seen[i % 3][0], seen[i % 3][1], head, k0, 2),
                                     "torch": lambda i: torch_refine(tin[i % 3][0], tin[i % 3][1], head, k0, 2)}, a.rounds, a.reps)
                kern = kernel_times([sg for sg, _, _ in seen], seen[0][1], k0, a.rounds)
            res["runs"].append({"encoder": enc, "k0": k0, "forward_ms": whole, "refine_stage_ms": stage, "last_step_kernels": kern})
            print(json.dumps(res["runs"][-1]), flush=True)
            del pr, up
            ops.release_workspaces()
            torch.cuda.empty_cache()
    os.makedirs(os.path.dirname(a.out) or ".", exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
    print("wrote", a.out)


if __name__ == "__main__":
    main()
