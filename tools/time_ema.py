"""Times the launches of include/catseg_ema.h on flat buffers of the size and layout of the bench model's (OCRNet-HRNetV2-W48: the
model is built on the host for its FlatParams layout and its BatchNorm set, the buffers are random), with HIP events around single
launches, in one run:
    adam_step       catseg_adam_step, the yardstick (profiles/optim_time.json records it at 0.73 of 8 TB/s), measured again here
    ema_update      catseg_ema_update, 12 B per element
    ema_update_dev  ... with the weight read from device memory
    ema_swap        catseg_ema_swap, 16 B per element
    ema_table       catseg_ema_table, mode 0, over the running means and variances of that network's BatchNorm modules
    ema_table_swap  ... mode 1
The C ABI is called directly on preallocated buffers; the cases are interleaved in rounds, every case rotates over two sets of buffers
(one set of ema_update is 585 MB, past the 256 MB last-level cache; two sets keep a launch from finding the tail of its own last run
there), and the medians over all launches are reported beside the algorithmic bytes and the fraction of 8 TB/s those bytes reach.

Then a training step of a manager-built network (OCRNetManager, --backbone, --batch x 3 x --height x --width) with and without
config['train']['ema'], eager and as a hipGraph, in alternating rounds of --step-iters steps between one pair of events.
    python tools/time_ema.py [--rounds 7] [--iters 10] [--no-steps] [--out profiles/ema_time.json]"""
import argparse
import json
import os
import sys
import tempfile

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from miccai2021_cataract_semantic_segmentation_amd import _lib, ops  # noqa: E402
from miccai2021_cataract_semantic_segmentation_amd.engine import FlatParams  # noqa: E402


def summary(t, nbytes=None):
    t = sorted(t)
    med = t[len(t) // 2]
    rec = {"median_us": round(med, 2), "min_us": round(t[0], 2), "max_us": round(t[-1], 2), "iqr_us": round(t[(3 * len(t)) // 4] - t[len(t) // 4], 2)}
    if nbytes:
        rec.update({"bytes": nbytes, "GB_per_s": round(nbytes / med * 1e-3, 1), "fraction_of_8TBps": round(nbytes / med * 1e-3 / 8000.0, 3)})
    return rec


def kernel_times(a, dev):
    from miccai2021_cataract_semantic_segmentation_amd.models import OCRNet
    model = OCRNet({"backbone": "hrnet48", "pretrained": False}, 3)
    fp = FlatParams(model).ensure()                       # (host buffers: the layout is what is wanted)
    n = fp.flat.numel()
    bn_sizes = [t.numel() for m in model.modules() if isinstance(m, torch.nn.modules.batchnorm._BatchNorm) and m.running_mean is not None
                for t in (m.running_mean, m.running_var)]
    gen = torch.Generator(device="cuda").manual_seed(0)
    sets = [{k: torch.randn(n, device=dev, generator=gen) * (1e-2 if k == "g" else 1.0) for k in ("p", "avg", "g")} for _ in range(2)]
    for s in sets:
        s["m"], s["v"] = torch.zeros(n, device=dev), torch.zeros(n, device=dev)
    w_dev = torch.tensor([1e-3], dtype=torch.float32, device=dev)
    lives = [torch.randn(k, device=dev, generator=gen) for k in bn_sizes]
    rec, off = [], 0
    for t in lives:
        rec.append((t.data_ptr(), off, t.numel(), 0))
        off += t.numel()
    table = torch.from_numpy(np.array(rec, dtype=ops.EMA_ENTRY).view(np.uint8).copy()).to(dev)
    shadow = torch.zeros(off, device=dev)
    lib, P, st, ck = _lib.lib, (lambda t: t.data_ptr()), _lib.stream, _lib.check
    turn = {"i": 0}

    def cur():
        turn["i"] += 1
        return sets[turn["i"] % 2]

    def adam():
        s = cur()
        ck(lib.catseg_adam_step(P(s["p"]), P(s["g"]), P(s["m"]), P(s["v"]), n, 1e-6, 0.9, 0.999, 1e-8, 10, 1.0, st()))

    def update(wd=None):
        s = cur()
        ck(lib.catseg_ema_update(P(s["p"]), P(s["avg"]), n, 1e-3, wd, st()))

    def swap():
        s = cur()
        ck(lib.catseg_ema_swap(P(s["p"]), P(s["avg"]), n, st()))
    cases = {
        "adam_step": (adam, 28.0 * n),
        "ema_update": (update, 12.0 * n),
        "ema_update_dev": (lambda: update(P(w_dev)), 12.0 * n),
        "ema_swap": (swap, 16.0 * n),
        "ema_table": (lambda: ck(lib.catseg_ema_table(P(table), len(rec), P(shadow), ops.EMA_LERP, 1e-3, None, st())), 12.0 * off),
        "ema_table_swap": (lambda: ck(lib.catseg_ema_table(P(table), len(rec), P(shadow), ops.EMA_SWAP, 0.0, None, st())), 16.0 * off),
    }
    times = {name: [] for name in cases}
    for fn, _ in cases.values():                 # warm-up
        for _ in range(4):
            fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    for _ in range(a.rounds):
        for name, (fn, _) in cases.items():
            for _ in range(a.iters):
                e0.record()
                fn()
                e1.record()
                e1.synchronize()
                times[name].append(e0.elapsed_time(e1) * 1e3)
    assert all(bool(torch.isfinite(s[k]).all()) for s in sets for k in ("p", "avg"))
    out = {"flat_floats": n, "bn_buffers": len(rec), "bn_floats": off, "cases": {}}
    for name, (_, nbytes) in cases.items():
        out["cases"][name] = summary(times[name], nbytes)
        print(json.dumps({name: out["cases"][name]}), flush=True)
    c = out["cases"]
    # what fusing the average into the update kernel could save at most: one launch and the re-read of p (4 of 12 bytes per element)
    out["fused_form_saves_at_most_us"] = round(c["ema_update"]["median_us"] / 3.0, 2)
    out["fused_form_note"] = ("a third of ema_update's median (4 of its 12 bytes per element), at the rate this kernel streams; the launch itself "
                              "overlaps the kernel in front of it on the stream")
    return out


def step_times(a, dev):
    from miccai2021_cataract_semantic_segmentation_amd.graph import GraphedTrainStep
    from miccai2021_cataract_semantic_segmentation_amd.managers import OCRNetManager, SyntheticCataractDataset
    log = tempfile.mkdtemp(prefix="time_ema_")
    ds = SyntheticCataractDataset(a.batch, a.height, a.width, 17, seed=1)
    img = torch.stack([ds[i][0] for i in range(a.batch)]).to(dev).float().contiguous()
    lbl = torch.stack([ds[i][1] for i in range(a.batch)]).to(dev).long().contiguous()
    runs = {}
    for key in ("plain", "ema"):
        train = {"learning_rate": 1e-4, "epochs": 1}
        if key == "ema":
            train["ema"] = {"decay": 0.999}
        cfg = {"name": key, "mode": "training", "manager": "OCRNet", "log_path": log,
               "graph": {"model": "OCRNet", "backbone": a.backbone, "pretrained": False}, "data": {"experiment": 2, "batch_size": a.batch},
               "loss": {"name": "TwoScaleLoss", "interm": {"name": "LovaszSoftmax", "args": [], "weight": 0.4},
                        "final": {"name": "LovaszSoftmax", "args": [], "weight": 1.0}}, "train": train, "seed": 0}
        m = OCRNetManager(cfg, ds, None)
        m.model.train()
        runs[key] = (m, GraphedTrainStep(m.model, None, m.optimiser, img, lbl, forward_loss=m.forward_loss))

    def eager(m):
        m.optimiser.zero_grad()
        loss, _ = m.forward_loss(img, lbl)
        loss.backward()
        m.optimiser.step()
    cases = {}
    for key, (m, g) in runs.items():
        cases["eager_" + key] = (lambda m=m: eager(m))
        cases["graph_" + key] = (lambda g=g: g(img, lbl))
    for fn in cases.values():
        for _ in range(2):
            fn()
    torch.cuda.synchronize()
    times = {name: [] for name in cases}
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    for _ in range(a.step_rounds):
        for name, fn in cases.items():
            e0.record()
            for _ in range(a.step_iters):
                fn()
            e1.record()
            e1.synchronize()
            times[name].append(e0.elapsed_time(e1) * 1e3 / a.step_iters)
    out = {"network": "OCRNet-%s via OCRNetManager" % a.backbone, "input": [a.batch, 3, a.height, a.width], "rounds": a.step_rounds,
           "steps_per_round": a.step_iters, "flat_floats": runs["ema"][0].model.flat().flat.numel(),
           "note": "per-step time = one pair of events around steps_per_round steps; the four cases alternate inside a round", "cases": {}}
    for name in cases:
        out["cases"][name] = summary(times[name])
        print(json.dumps({name: out["cases"][name]}), flush=True)
    for form in ("eager", "graph"):
        out[form + "_ema_minus_plain_us"] = round(out["cases"][form + "_ema"]["median_us"] - out["cases"][form + "_plain"]["median_us"], 1)
    for _, g in runs.values():
        g.release()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--no-steps", action="store_true")
    ap.add_argument("--backbone", default="hrnet48")
    ap.add_argument("--batch", type=int, default=2)
    ap.add_argument("--height", type=int, default=256)
    ap.add_argument("--width", type=int, default=480)
    ap.add_argument("--step-rounds", type=int, default=5)
    ap.add_argument("--step-iters", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ema_time.json"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("time_ema.py measures on the GPU: none found")
    dev = torch.device("cuda")
    res = {"model": "OCRNet-HRNetV2-W48", "rounds": a.rounds, "iters_per_round": a.iters, "device": torch.cuda.get_device_name(0),
           "note": "one launch between one pair of events; fraction_of_8TBps = bytes / median / 8 TB/s; iqr = the interquartile range of the "
                   "case's own launches"}
    res.update(kernel_times(a, dev))
    torch.cuda.empty_cache()
    if not a.no_steps:
        res["training_step"] = step_times(a, dev)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
