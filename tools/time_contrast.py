"""Times the launches of the dense contrastive loss (include/ext/catseg_contrast.h and the three catseg_gemm_batched products around them) at
the shape of OCRNet-ResNet50 on the bench input: features 8 x 68 x 120, d = 128, K = 25, M = 160 (A = 4000 slots), labels 8 x 544 x 960.
HIP events around single launches through ops.py's wrappers (the buffers a wrapper allocates come from torch's caching allocator: no
device allocation after the warm-up), inputs rotated over two sets, the cases interleaved in --rounds rounds of --iters launches, medians
reported beside the bytes that follow from the shapes and the fraction of 8 TB/s those bytes reach.  pick is three launches and
scatter_bwd two behind one entry point; a launch of a few microseconds is latency-bound and says so instead of a fraction.

Then the train step of OCRNetManager (OCRNet-ResNet50, --batch x 3 x --height x --width) with and without the two keys ('projector' in
the graph section, 'DenseContrastiveLoss' in the LossWrapper), eager, in alternating rounds of --step-iters steps between one pair of events.
    python tools/time_contrast.py [--rounds 7] [--iters 10] [--no-steps] [--out profiles/contrast_time.json]"""
import argparse
import json
import os
import sys
import tempfile

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from miccai2021_cataract_semantic_segmentation_amd import ops  # noqa: E402

LATENCY_BOUND_US = 10.0


def summary(t, nbytes=None):
    t = sorted(t)
    med = t[len(t) // 2]
    rec = {"median_us": round(med, 2), "min_us": round(t[0], 2), "max_us": round(t[-1], 2), "iqr_us": round(t[(3 * len(t)) // 4] - t[len(t) // 4], 2)}
    if nbytes:
        rec["bytes"] = nbytes
        if med < LATENCY_BOUND_US:
            rec["note"] = "latency-bound: a launch of a few microseconds, the bytes do not set its time"
        else:
            rec.update({"GB_per_s": round(nbytes / med * 1e-3, 1), "fraction_of_8TBps": round(nbytes / med * 1e-3 / 8000.0, 4)})
    return rec


def kernel_times(a, dev):
    B, H, W, h, w, d, K, M = 8, 544, 960, 68, 120, 128, 25, 160
    A, n_pix = K * M, B * h * w
    gen = torch.Generator(device="cuda").manual_seed(0)
    sets = []
    for s in range(2):
        lbl = torch.randint(0, K + 1, (B, H // 16, W // 16), device=dev, generator=gen).repeat_interleave(16, 1).repeat_interleave(16, 2).contiguous()
        feat = torch.randn((B, h, w, d), device=dev, generator=gen)
        state = torch.tensor([1 + s, 0, 0, 0], dtype=torch.int32, device=dev)
        idx, lab, n_pos = ops.contrast_pick(lbl, h, w, K, M, state=state)
        Z, inv = ops.contrast_gather(feat, idx, 1e-12)
        S = torch.empty((A, ops.r4(A)), dtype=torch.float32, device=dev)
        sets.append(dict(lbl=lbl, feat=feat, state=state, idx=idx, lab=lab, n_pos=n_pos, Z=Z, inv=inv, S=S, dZ=torch.empty_like(Z),
                         ell=torch.empty(A, device=dev), g=torch.ones(1, device=dev)))
    Wt = torch.ones((K, K), device=dev)
    turn = {"i": 0}

    def cur():
        turn["i"] += 1
        return sets[turn["i"] % 2]

    def s_product(z):
        ops.gemm(ops.NT, 1, A, A, d, z["Z"], d, 0, z["Z"], d, 0, z["S"], z["S"].stride(0), 0)

    def rows(z):
        s_product(z)                                     # (rows overwrites S: every timed launch needs a fresh S; timed apart below)
        ops.contrast_rows(z["S"], A, z["lab"], Wt, 10.0, z["n_pos"], ell=z["ell"])
    lds = ops.r4(A)
    cases = {
        "pick": (lambda z: ops.contrast_pick(z["lbl"], h, w, K, M, state=z["state"]), 2 * 8.0 * n_pix + 8.0 * A + 8.0 * K * ((n_pix + 255) // 256)),
        "gather": (lambda z: ops.contrast_gather(z["feat"], z["idx"], 1e-12, Z=z["Z"], inv_norm=z["inv"]), 4.0 * A * (2 * d + 2)),
        "gemm_S": (s_product, 4.0 * A * (2 * d + lds)),
        "gemm_S_then_rows": (rows, 4.0 * A * (2 * d + lds) + 8.0 * A * lds),
        "finalize": (lambda z: ops.contrast_finalize(z["ell"], z["n_pos"]), 4.0 * A),
        "gemm_dZ_nn": (lambda z: ops.gemm(ops.NN, 1, A, d, A, z["S"], lds, 0, z["Z"], d, 0, z["dZ"], d, 0), 4.0 * A * (lds + 2 * d)),
        "gemm_dZ_tn": (lambda z: ops.gemm(ops.TN, 1, A, d, A, z["S"], lds, 0, z["Z"], d, 0, z["dZ"], d, 0, accumulate=True), 4.0 * A * (lds + 3 * d)),
        "scatter_bwd": (lambda z: ops.contrast_scatter_bwd(z["dZ"], z["Z"], z["inv"], z["idx"], d, z["g"], 10.0, (B, h, w, d)),
                        4.0 * n_pix * d + 12.0 * A * d),
    }
    times = {name: [] for name in cases}
    for fn, _ in cases.values():
        for _ in range(4):
            fn(cur())
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    for _ in range(a.rounds):
        for name, (fn, _) in cases.items():
            for _ in range(a.iters):
                z = cur()
                e0.record()
                fn(z)
                e1.record()
                e1.synchronize()
                times[name].append(e0.elapsed_time(e1) * 1e3)
    out = {"shape": {"B": B, "H": H, "W": W, "h": h, "w": w, "d": d, "K": K, "M": M, "A": A}, "cases": {}}
    for name, (_, nbytes) in cases.items():
        out["cases"][name] = summary(times[name], nbytes)
        print(json.dumps({name: out["cases"][name]}), flush=True)
    c = out["cases"]
    out["rows_alone_us"] = round(c["gemm_S_then_rows"]["median_us"] - c["gemm_S"]["median_us"], 2)
    out["rows_alone_fraction_of_8TBps"] = round(8.0 * A * lds / max(out["rows_alone_us"], 1e-3) * 1e-3 / 8000.0, 4)
    out["loss_forward_backward_us"] = round(sum(c[k]["median_us"] for k in ("pick", "gather", "gemm_S_then_rows", "finalize", "gemm_dZ_nn", "gemm_dZ_tn",
                                                                            "scatter_bwd")), 1)
    return out


def step_times(a, dev):
    from miccai2021_cataract_semantic_segmentation_amd.managers import OCRNetManager, SyntheticCataractDataset
    log = tempfile.mkdtemp(prefix="time_contrast_")
    ds = SyntheticCataractDataset(a.batch, a.height, a.width, 25, seed=1)
    img = torch.stack([ds[i][0] for i in range(a.batch)]).to(dev).float().contiguous()
    lbl = torch.stack([ds[i][1] for i in range(a.batch)]).to(dev).long().contiguous()
    runs = {}
    for key in ("plain", "contrast"):
        graph = {"model": "OCRNet", "backbone": "resnet50", "out_stride": 8, "pretrained": False}
        losses = {"CrossEntropyLoss": 1}
        if key == "contrast":
            graph["projector"] = {"mlp": [[1, 256, 1]], "d": 128}
            losses["DenseContrastiveLoss"] = 0.1
        cfg = {"name": key, "mode": "training", "manager": "OCRNet", "log_path": log, "graph": graph, "data": {"experiment": 3, "batch_size": a.batch},
               "loss": {"name": "LossWrapper", "losses": losses, "max_anchors_per_class": 160}, "train": {"learning_rate": 1e-4, "epochs": 1}, "seed": 0}
        m = OCRNetManager(cfg, ds, None)
        m.model.train()
        runs[key] = m

    def step(m):
        m.optimiser.zero_grad()
        loss, _ = m.forward_loss(img, lbl)
        loss.backward()
        m.optimiser.step()
    for m in runs.values():
        for _ in range(3):
            step(m)
    torch.cuda.synchronize()
    times = {k: [] for k in runs}
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    for _ in range(a.rounds):
        for key, m in runs.items():
            e0.record()
            for _ in range(a.step_iters):
                step(m)
            e1.record()
            e1.synchronize()
            times[key].append(e0.elapsed_time(e1) / a.step_iters)
    out = {"batch": a.batch, "height": a.height, "width": a.width, "ms_per_step": {}}
    for key, t in times.items():
        t = sorted(t)
        out["ms_per_step"][key] = {"median": round(t[len(t) // 2], 3), "min": round(t[0], 3), "max": round(t[-1], 3)}
    out["contrast_minus_plain_ms"] = round(out["ms_per_step"]["contrast"]["median"] - out["ms_per_step"]["plain"]["median"], 3)
    print(json.dumps(out), flush=True)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--step-iters", type=int, default=5)
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--height", type=int, default=544)
    ap.add_argument("--width", type=int, default=960)
    ap.add_argument("--no-steps", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "contrast_time.json"))
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    rec = {"device": torch.cuda.get_device_name(0), "rounds": a.rounds, "iters": a.iters, "kernels": kernel_times(a, dev)}
    if not a.no_steps:
        rec["train_step"] = step_times(a, dev)
    with open(a.out, "w") as f:
        json.dump(rec, f, indent=1)
        f.write("\n")
    print("wrote", a.out)


if __name__ == "__main__":
    main()
