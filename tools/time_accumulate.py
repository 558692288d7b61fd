"""Times the fold of a gradient-accumulation window (optim.FusedOptimizer.fold: acc += g, one catseg_axpy2d launch over the flat
buffer viewed as [numel / 64, 64]) on flat buffers of the size and layout of the bench model's (OCRNet-HRNetV2-W48: the model is built
on the host for its FlatParams layout, the buffers are random), with HIP events around single launches, beside catseg_ema_update in the
same run -- both read 8 and write 4 bytes per element:
    ema_update   catseg_ema_update, the yardstick (profiles/ema_time.json), measured again here
    fold         catseg_axpy2d(g, acc, alpha = 1, accumulate), rows = numel / 64, C = 64
    window_clear the memset of the window behind the optimiser step (acc.zero_(), 4 B per element)
The C ABI is called directly on preallocated buffers; the cases are interleaved in rounds, every case rotates over two sets of buffers
(one set of a case is 585 MB, past the 256 MB last-level cache; two sets keep a launch from finding the tail of its own last run
there), and the medians over all launches are reported beside the algorithmic bytes and the fraction of 8 TB/s those bytes reach.
    python tools/time_accumulate.py [--rounds 7] [--iters 10] [--out profiles/accumulate_time.json]"""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from miccai2021_cataract_semantic_segmentation_amd import _lib  # noqa: E402
from miccai2021_cataract_semantic_segmentation_amd.engine import FlatParams  # noqa: E402


def summary(t, nbytes):
    t = sorted(t)
    med = t[len(t) // 2]
    return {"median_us": round(med, 2), "min_us": round(t[0], 2), "max_us": round(t[-1], 2), "iqr_us": round(t[(3 * len(t)) // 4] - t[len(t) // 4], 2),
            "bytes": nbytes, "GB_per_s": round(nbytes / med * 1e-3, 1), "fraction_of_8TBps": round(nbytes / med * 1e-3 / 8000.0, 3)}


def kernel_times(a, dev):
    from miccai2021_cataract_semantic_segmentation_amd.models import OCRNet
    model = OCRNet({"backbone": "hrnet48", "pretrained": False}, 3)
    n = FlatParams(model).ensure().flat.numel()           # (host buffers: the layout is what is wanted)
    align = FlatParams.ALIGN
    assert n % align == 0
    gen = torch.Generator(device="cuda").manual_seed(0)
    sets = [{k: torch.randn(n, device=dev, generator=gen) * (1e-2 if k == "g" else 1.0) for k in ("p", "avg", "g", "acc")} for _ in range(2)]
    lib, P, st, ck = _lib.lib, (lambda t: t.data_ptr()), _lib.stream, _lib.check
    turn = {"i": 0}

    def cur():
        turn["i"] += 1
        return sets[turn["i"] % 2]

    def update():
        s = cur()
        ck(lib.catseg_ema_update(P(s["p"]), P(s["avg"]), n, 1e-3, None, st()))

    def fold():
        s = cur()
        ck(lib.catseg_axpy2d(P(s["g"]), align, P(s["acc"]), align, n // align, align, 1.0, 1, st()))

    def clear():
        cur()["acc"].zero_()
    cases = {"ema_update": (update, 12.0 * n), "fold": (fold, 12.0 * n), "window_clear": (clear, 4.0 * n)}
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
    assert all(bool(torch.isfinite(s[k]).all()) for s in sets for k in ("avg", "acc"))
    out = {"flat_floats": n, "cases": {}}
    for name, (_, nbytes) in cases.items():
        out["cases"][name] = summary(times[name], nbytes)
        print(json.dumps({name: out["cases"][name]}), flush=True)
    out["fold_over_ema_update"] = round(out["cases"]["fold"]["median_us"] / out["cases"]["ema_update"]["median_us"], 3)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "accumulate_time.json"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("time_accumulate.py measures on the GPU: none found")
    dev = torch.device("cuda")
    res = {"model": "OCRNet-HRNetV2-W48", "rounds": a.rounds, "iters_per_round": a.iters, "device": torch.cuda.get_device_name(0),
           "note": "one launch between one pair of events; fraction_of_8TBps = bytes / median / 8 TB/s; iqr = the interquartile range of the "
                   "case's own launches; fold_over_ema_update = the ratio of the two medians of this run",
           "not_measured": "a training step of the bench shape under accumulation; data parallel (refused)"}
    res.update(kernel_times(a, dev))
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
