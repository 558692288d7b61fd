"""Times the label census (csrc/census.hip) against the same counts from torch device operations, the per-batch IoU average, and a training
step of a tiny manager run with the IoU tracker on and off, with HIP events, in one run:
    census_8 / census_64          catseg_label_census_u8 over 8 / 64 frames of 540 x 960 (blob-structured label maps, 36 classes)
    torch_bincount_8 / _64        torch.bincount(frame * 256 + label, minlength=B * 256) on the device: the counts without the kernel
    census_8_noise                the census over uniformly random labels (no runs to aggregate: every lane walks its 16 bytes)
    iou_ema_17                    catseg_iou_ema on a 17 x 17 matrix
    step_tracker_off / _on        one eager training step of UNet (FCN manager's step: 2 x 40 x 56, LovaszSoftmax, Adam, confusion matrix)
                                  without / with IoUTracker.step + publish behind it
The C ABI is called directly on preallocated outputs (no allocator inside the timed region); the census inputs rotate through >= 1.5 GB of
frame sets, so that no launch finds its frames in the 256 MB last-level cache; the cases are interleaved in rounds and the medians over all
launches are reported, the census beside its algorithmic bytes (every label byte once) and the time those take at 8 TB/s.
    python tools/time_census.py [--rounds 7] [--iters 10] [--out profiles/census_time.json]"""
import argparse
import json
import os
import sys
import tempfile

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from miccai2021_cataract_semantic_segmentation_amd import _lib, ops  # noqa: E402

H, W, NBINS = 540, 960, 36


def blob_maps(B, gen, dev):
    small = torch.randint(0, NBINS, (B, (H + 11) // 12, (W + 15) // 16), dtype=torch.uint8, device=dev, generator=gen)
    return small.repeat_interleave(12, 1).repeat_interleave(16, 2)[:, :H, :W].contiguous()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "census_time.json"))
    a = ap.parse_args()
    dev = torch.device("cuda")
    lib, P, st = _lib.lib, (lambda t: 0 if t is None else t.data_ptr()), _lib.stream
    gen = torch.Generator(device="cuda").manual_seed(0)
    nsets64 = int(1.5e9 / (64 * H * W)) + 1
    sets64 = [blob_maps(64, gen, dev) for _ in range(nsets64)]
    sets8 = [s[8 * j:8 * j + 8] for s in sets64 for j in range(8)]             # (views: every set of 8 lies in another 4 MB of the 1.5 GB)
    noise = torch.randint(0, NBINS, (nsets64 * 64, H, W), dtype=torch.uint8, device=dev, generator=gen)
    noise8 = [noise[8 * j:8 * j + 8] for j in range(nsets64 * 8)]
    counts = {8: torch.empty((8, NBINS + 1), dtype=torch.int64, device=dev), 64: torch.empty((64, NBINS + 1), dtype=torch.int64, device=dev)}
    offsets = {B: (torch.arange(B, device=dev, dtype=torch.int64) * 256).view(B, 1, 1) for B in (8, 64)}

    def census(sets, B):
        return lambda k: _lib.check(lib.catseg_label_census_u8(P(sets[k % len(sets)]), B, H, W, None, NBINS, P(counts[B]), 0, st()))

    def bincount(sets, B):
        return lambda k: torch.bincount((sets[k % len(sets)].to(torch.int64) + offsets[B]).view(-1), minlength=B * 256)

    # the two ways agree (once, outside the timing)
    got = ops.label_census(sets8[0], NBINS)[:, :NBINS]
    assert torch.equal(got, bincount(sets8, 8)(0).view(8, 256)[:, :NBINS])

    K = 17
    cm, prev = torch.randint(0, 5000, (K, K), dtype=torch.int32, device=dev), torch.zeros((K, K), dtype=torch.int32, device=dev)
    vals = torch.full((K,), 0.5, device=dev)

    # the tiny manager step (eager), tracker off / on
    from miccai2021_cataract_semantic_segmentation_amd import managers
    from miccai2021_cataract_semantic_segmentation_amd.utils import IoUTracker
    from miccai2021_cataract_semantic_segmentation_amd.utils.metrics import t_get_confusion_matrix
    cfg = {"name": "t", "mode": "training", "manager": "FCN", "log_path": tempfile.mkdtemp(), "graph": {"model": "UNet"},
           "data": {"experiment": 2, "batch_size": 2}, "loss": {"name": "LovaszSoftmax"}, "train": {"learning_rate": 1e-3, "epochs": 1}, "seed": 0}
    ds = managers.SyntheticCataractDataset(8, 40, 56, 17, seed=3, patch=8)
    m = managers.FCNManager(cfg, ds, None)
    m.model.train()
    batches = [(torch.stack([ds[i][0], ds[i + 1][0]]).to(dev), torch.stack([ds[i][1], ds[i + 1][1]]).to(dev)) for i in range(0, 8, 2)]
    running = torch.zeros((m.model.num_classes,) * 2, dtype=torch.int32, device=dev)
    tracker = IoUTracker(m.model.num_classes, 0.3, dev)

    def step(with_tracker):
        def run(k):
            img, lbl = batches[k % len(batches)]
            m.optimiser.zero_grad()
            loss, out = m.forward_loss(img, lbl)
            loss.backward()
            m.optimiser.step()
            t_get_confusion_matrix(out.detach(), lbl, running)
            if with_tracker:
                tracker.step(running)
                tracker.publish()
        return run

    cases = {
        "census_8": (census(sets8, 8), 8.0 * H * W),
        "torch_bincount_8": (bincount(sets8, 8), 8.0 * H * W),
        "census_64": (census(sets64, 64), 64.0 * H * W),
        "torch_bincount_64": (bincount(sets64, 64), 64.0 * H * W),
        "census_8_noise": (census(noise8, 8), 8.0 * H * W),
        "iou_ema_17": (lambda k: _lib.check(lib.catseg_iou_ema(P(cm), P(prev), K, 0.7, 0.3, P(vals), None, st())), None),
        "step_tracker_off": (step(False), None),
        "step_tracker_on": (step(True), None),
    }
    times = {name: [] for name in cases}
    k = 0
    for name, (fn, _) in cases.items():          # warm-up
        for _ in range(3):
            fn(k)
            k += 1
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    for _ in range(a.rounds):
        for name, (fn, _) in cases.items():
            for _ in range(a.iters):
                e0.record()
                fn(k)
                e1.record()
                e1.synchronize()
                times[name].append(e0.elapsed_time(e1) * 1e3)
                k += 1
    res = {"frames": [H, W], "nbins": NBINS, "input_sets_of_64": nsets64, "input_bytes_rotated": nsets64 * 64 * H * W, "rounds": a.rounds,
           "iters_per_round": a.iters, "device": torch.cuda.get_device_name(0),
           "note": "census_* = the memset node and the kernel of catseg_label_census_u8 between one pair of events; bytes = every label byte "
                   "once; us_at_8TBps = those bytes at 8 TB/s; step_* = the enqueue and run of one eager training step (host-bound at this size)",
           "cases": {}}
    for name, (_, nbytes) in cases.items():
        t = sorted(times[name])
        med = t[len(t) // 2]
        rec = {"median_us": round(med, 2), "min_us": round(t[0], 2), "max_us": round(t[-1], 2)}
        if nbytes:
            rec.update({"bytes": nbytes, "GB_per_s": round(nbytes / med * 1e-3, 1), "us_at_8TBps": round(nbytes / 8e12 * 1e6, 2)})
        res["cases"][name] = rec
        print(json.dumps({name: rec}), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
