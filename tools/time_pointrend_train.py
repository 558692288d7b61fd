"""Times PointRend's training step (csrc/pointrend_train.hip, engine.pointrend_train) at the flagship shape:

    python3 tools/time_pointrend_train.py [--batch 8] [--height 544] [--width 960] [--points 2048] [--rounds 5] [--reps 2]
                                          [--out profiles/pointrend_train_time.json]

Experiment 3 (K = 25), EncDec-ResNet50:
  * the train step (zero_grad, forward, LossWrapper(CrossEntropyLoss) + point cross-entropy, backward, FusedAdam) with the PointRend decoder
    against the same network with the UPerNet decoder, interleaved in every round, three inputs in rotation, medians over the rounds;
  * every new kernel in microseconds (20 back-to-back calls of its C entry point per timed window, arguments built beforehand) and as a
    fraction of 8 TB/s for the bytes its shapes imply; the gather backward beside the gather forward.
Device events around every timed window."""
import argparse
import ctypes
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from miccai2021_cataract_semantic_segmentation_amd import _lib, losses, ops  # noqa: E402
from miccai2021_cataract_semantic_segmentation_amd.models import EncDec  # noqa: E402
from miccai2021_cataract_semantic_segmentation_amd.optim import FusedAdam  # noqa: E402

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


def make_step(decoder, a, xs, lbls):
    torch.manual_seed(0)
    model = EncDec({"encoder": {"model": "ResNet50", "pretrained": False}, "decoder": decoder}, 3).cuda().train()
    crit = losses.LossWrapper({"losses": {"CrossEntropyLoss": 1}, "experiment": 3, "device": "cuda"})
    ce = losses.CrossEntropyLoss(ignore_index=25)
    opt = FusedAdam(model, lr=1e-4)

    def step(i):
        x, lbl = xs[i % 3], lbls[i % 3]
        opt.zero_grad()
        out = model(x)
        if len(out) == 5:
            deep, coords, pl, seg, _ = out
            loss = crit(deep, seg, lbl) + ce(pl.unsqueeze(3), ops.pointrend_point_labels(coords, lbl).unsqueeze(2))
        else:
            loss = crit(out[0], out[1], lbl)
        loss.backward()
        opt.step()
    return model, step


def kernel_times(a, rounds, launches=20):
    """the new kernels at the step's shapes (ResNet50 stages at 1/4 .. 1/32, coarse logits at 1/4), three input sets in rotation.
    Two windows differ from what the step launches: the scatter and its backward run here on a dense pred / dpred (rows of K = 25 floats)
    where the step hands them whatever pitch the resize and the loss produce, and the scatter backward accumulates (accumulate = 1) from a
    dpred that its own first launch of the window has already zeroed at the scattered pixels -- same traffic, other values."""
    lib, st = _lib.lib, _lib.stream()
    N, P, K, Kq = a.batch, a.points, 25, 28
    M, kb = 3 * P, int(0.75 * P)
    h, w = a.height, a.width
    chans = (256, 512, 1024, 2048)
    sizes = [((h + s - 1) // s, (w + s - 1) // s) for s in (4, 8, 16, 32)]
    gen = torch.Generator().manual_seed(1)
    sets = []
    for _ in range(3):
        feats = [torch.randn(N, hh, ww, c, device="cuda") for c, (hh, ww) in zip(chans, sizes)]
        coarse = ops.new_act(N, sizes[0][0], sizes[0][1], K, "cuda", ld=32, zero=True)
        coarse.copy_(torch.randn(N, sizes[0][0], sizes[0][1], K, device="cuda"))
        state = torch.tensor([1, 2, 0, 0], dtype=torch.int32, device="cuda")
        cand = ops.pointrend_draw(state, N, M)
        rest = ops.pointrend_draw(state, N, P - kb)
        unc = ops.pointrend_point_uncertainty(coarse, cand)
        sel = ops.pointrend_topk(unc, kb)
        lbl = torch.randint(0, 26, (N, h, w), generator=gen).cuda()
        coords, pix, labels = ops.pointrend_compose(cand, sel, rest, h, w, lbl)
        srcs = feats[::-1] + [coarse]
        cols = sum(chans) + Kq
        x = torch.empty((N * P, cols), device="cuda")
        dx = torch.randn(N * P, cols, device="cuda")
        grads = [torch.empty_like(f) for f in feats[::-1]] + [ops.new_act(N, sizes[0][0], sizes[0][1], K, "cuda", ld=32, zero=True)]
        d = _lib.PointrendGatherDesc()
        b = _lib.PointrendGatherBwdDesc()
        for i, (s, g) in enumerate(zip(srcs, grads)):
            d.src[i], d.ld[i], d.H[i], d.W[i], d.C[i] = s.data_ptr(), ops.ld_of(s), s.shape[1], s.shape[2], s.shape[3]
            b.dst[i], b.ld[i], b.H[i], b.W[i], b.C[i], b.accumulate[i] = g.data_ptr(), ops.ld_of(g), g.shape[1], g.shape[2], g.shape[3], 0
        d.n_sources, d.N, d.k, d.out, d.ld_out = 5, N, P, x.data_ptr(), cols
        b.n_sources, b.coords, b.N, b.P, b.dx, b.ld_dx = 5, coords.data_ptr(), N, P, dx.data_ptr(), cols
        pred = torch.randn(N, h, w, K, device="cuda")
        rows = torch.randn(N * P, Kq, device="cuda")
        sets.append(dict(state=state, cand=cand, rest=rest, unc=unc, sel=sel, lbl=lbl, coords=coords, pix=pix, labels=labels, coarse=coarse, d=d, b=b,
                         pred=pred, rows=rows, keep=(feats, grads, x, dx)))
    hc, wc = sizes[0]
    calls = {
        "draw": lambda z: lib.catseg_pointrend_draw(z["state"].data_ptr(), None, N, M, z["cand"].data_ptr(), st),
        "point_uncertainty": lambda z: lib.catseg_pointrend_point_uncertainty(z["coarse"].data_ptr(), 32, N, hc, wc, K, z["cand"].data_ptr(), M, z["unc"].data_ptr(), st),
        "compose": lambda z: lib.catseg_pointrend_compose(z["cand"].data_ptr(), M, z["sel"].data_ptr(), kb, z["rest"].data_ptr(), N, P, h, w, z["lbl"].data_ptr(), h, w,
                                                          z["coords"].data_ptr(), z["pix"].data_ptr(), z["labels"].data_ptr(), st),
        "gather_at": lambda z: lib.catseg_pointrend_gather_at(ctypes.byref(z["d"]), z["coords"].data_ptr(), st),
        "gather_bwd": lambda z: lib.catseg_pointrend_gather_bwd(ctypes.byref(z["b"]), st),
        "scatter_last": lambda z: lib.catseg_pointrend_scatter_last(z["rows"].data_ptr(), Kq, z["pix"].data_ptr(), N, P, h * w, z["pred"].data_ptr(), K, K, st),
        "scatter_bwd": lambda z: lib.catseg_pointrend_scatter_bwd(z["pred"].data_ptr(), K, z["pix"].data_ptr(), N, P, h * w, z["rows"].data_ptr(), Kq, K, 1, st),
    }
    ms = interleaved({n: (lambda i, f=f: _lib.check(f(sets[i % 3]))) for n, f in calls.items()}, rounds, launches)
    Cf = sum(chans)
    maps = sum(N * hh * ww * c for c, (hh, ww) in zip(chans, sizes)) + N * hc * wc * 32
    taps = sum(min(4.0 * N * P * c, float(N * hh * ww * c)) for c, (hh, ww) in zip(chans + (K,), sizes + [sizes[0]]))
    bytes_ = {"draw": 4.0 * N * M * 2, "point_uncertainty": 4.0 * (N * M * (2 + 1) + min(4.0 * N * M * K, N * hc * wc * K)),
              "compose": 4.0 * N * P * (2 + 2 + 1 + 2 + 1), "gather_at": 4.0 * (N * P * (Cf + Kq) + taps),
              # gather backward: the zero fill of every destination, dX once, one read-modify-write per tap pixel
              "gather_bwd": 4.0 * (maps + N * P * (Cf + Kq) + taps), "scatter_last": 8.0 * N * P * K, "scatter_bwd": 4.0 * N * P * K * 4}
    out = {n: {"us": round(1e3 * ms[n], 2), "fraction_of_8TBs": round(bytes_[n] / (ms[n] * 1e-3) / HBM, 4)} for n in bytes_}
    out["gather_bwd_over_gather_at"] = round(ms["gather_bwd"] / ms["gather_at"], 2)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--height", type=int, default=544)
    ap.add_argument("--width", type=int, default=960)
    ap.add_argument("--points", type=int, default=2048)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--reps", type=int, default=2)
    ap.add_argument("--out", default="profiles/pointrend_train_time.json")
    a = ap.parse_args()
    gen = torch.Generator().manual_seed(0)
    xs = [torch.rand(a.batch, 3, a.height, a.width, generator=gen).cuda() for _ in range(3)]
    lbls = [torch.randint(0, 26, (a.batch, a.height // 16, a.width // 16), generator=gen).repeat_interleave(16, 1).repeat_interleave(16, 2).cuda() for _ in range(3)]
    res = {"shape": [a.batch, 3, a.height, a.width], "experiment": 3, "encoder": "ResNet50", "points": a.points, "rounds": a.rounds, "reps": a.reps,
           "device": torch.cuda.get_device_name(0)}
    res["kernels"] = kernel_times(a, a.rounds)
    print(json.dumps(res["kernels"]), flush=True)
    pr_model, pr_step = make_step({"model": "PointRend", "pr_train_num_pts": a.points, "pr_subdivision_num_pts": 8192, "pr_train_on_device": True}, a, xs, lbls)
    up_model, up_step = make_step({"model": "UPerNet"}, a, xs, lbls)
    for i in range(2):                      # (workspaces, weight images and allocator pools reach their steady state)
        pr_step(i)
        up_step(i)
    res["train_step_ms"] = interleaved({"pointrend": pr_step, "upernet": up_step}, a.rounds, a.reps)
    res["not_measured"] = ["the step replayed as a hipGraph", "data-parallel runs", "ResNeXt101", "the point head's GEMMs one by one"]
    print(json.dumps(res["train_step_ms"]), flush=True)
    os.makedirs(os.path.dirname(a.out) or ".", exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
    print("wrote", a.out)


if __name__ == "__main__":
    main()
