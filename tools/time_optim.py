"""Times the optimiser launches of include/catseg_optim.h beside the existing catseg_adam_step, on flat buffers of the size and
layout of the bench model's (OCRNet-HRNetV2-W48: the model is built on the host for its FlatParams layout, the buffers are random), with
HIP events around single launches, in one run:
    adam_step             catseg_adam_step (what FusedAdam launches with its arguments of old)
    adam_ex_plain         catseg_adam_step_ex, one group, no option (the same bits as adam_step)
    adam_ex_wd_2groups    ... decoupled weight decay, two groups (optim.param_groups: weights / norms and biases) through the chunk map
    adam_ex_amsgrad       ... amsgrad (a fourth state buffer read and written)
    sgd_momentum          catseg_sgd_step with a momentum buffer
    grad_norm_pair        catseg_grad_norm: the partial-sum launch and the one-block launch behind it
    grad_norm_pair_n1     the same pair on one element: what two launches cost when there is nothing to read
The C ABI is called directly on preallocated buffers; the cases are interleaved in rounds and the medians over all launches are reported
beside the algorithmic bytes (28 B per parameter for Adam, 36 B with amsgrad, 20 B for momentum SGD, 4 B for the norm, 1/64 B for the map)
and the fraction of 8 TB/s those bytes reach.  The buffers of one launch (1.2 GB for Adam) exceed the 256 MB last-level cache.
    python tools/time_optim.py [--rounds 7] [--iters 10] [--out profiles/optim_time.json]"""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from miccai2021_cataract_semantic_segmentation_amd import _lib, ops, optim  # noqa: E402
from miccai2021_cataract_semantic_segmentation_amd.engine import FlatParams  # noqa: E402

B1, B2, EPS, LR = 0.9, 0.999, 1e-8, 1e-6


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "optim_time.json"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("time_optim.py measures on the GPU: none found")
    dev = torch.device("cuda")
    from miccai2021_cataract_semantic_segmentation_amd.models import OCRNet
    model = OCRNet({"backbone": "hrnet48", "pretrained": False}, 3)
    fp = FlatParams(model).ensure()                       # (host buffers: the layout is what is wanted)
    n = fp.flat.numel()
    groups = optim.param_groups(model, 1e-2)
    group_of = {id(p): gi for gi, g in enumerate(groups) for p in g["params"]}
    cmap = torch.from_numpy(optim.chunk_group_map([fp.offsets[id(p)] for p in fp.params], [p.numel() for p in fp.params],
                                                  [group_of[id(p)] for p in fp.params], n)).to(dev)
    n_real = sum(p.numel() for p in fp.params)
    gen = torch.Generator(device="cuda").manual_seed(0)
    p = torch.randn(n, device=dev, generator=gen)
    g = torch.randn(n, device=dev, generator=gen) * 1e-2
    m, v, vmax, buf = (torch.zeros(n, device=dev) for _ in range(4))
    out = torch.zeros(2, device=dev)
    ws = torch.zeros(ops.grad_norm_workspace(n), dtype=torch.uint8, device=dev)
    row1 = ops.optim_hyper(torch.zeros(20), 10, B1, B2, 1.0, 0.0, [LR], [0.0])
    row2 = ops.optim_hyper(torch.zeros(20), 10, B1, B2, 1.0, 0.0, [LR, LR], [1e-2, 0.0])
    lib, P, st = _lib.lib, (lambda t: 0 if t is None else t.data_ptr()), _lib.stream
    ck = _lib.check

    cases = {
        "adam_step": (lambda: ck(lib.catseg_adam_step(P(p), P(g), P(m), P(v), n, LR, B1, B2, EPS, 10, 1.0, st())), 28.0),
        "adam_ex_plain": (lambda: ck(lib.catseg_adam_step_ex(P(p), P(g), P(m), P(v), None, n, None, 1, P(row1), None, B1, B2, EPS, ops.WD_NONE, None,
                                                             st())), 28.0),
        "adam_ex_wd_2groups": (lambda: ck(lib.catseg_adam_step_ex(P(p), P(g), P(m), P(v), None, n, P(cmap), 2, P(row2), None, B1, B2, EPS,
                                                                  ops.WD_DECOUPLED, None, st())), 28.0 + 1.0 / 64),
        "adam_ex_amsgrad": (lambda: ck(lib.catseg_adam_step_ex(P(p), P(g), P(m), P(v), P(vmax), n, None, 1, P(row1), None, B1, B2, EPS, ops.WD_NONE, None,
                                                               st())), 36.0),
        "sgd_momentum": (lambda: ck(lib.catseg_sgd_step(P(p), P(g), P(buf), n, None, 1, P(row1), None, 0.9, 0, 0, None, st())), 20.0),
        "grad_norm_pair": (lambda: ck(lib.catseg_grad_norm(P(g), n, 1.0, None, 1.0, P(ws), ws.numel(), P(out), st())), 4.0),
        "grad_norm_pair_n1": (lambda: ck(lib.catseg_grad_norm(P(g), 1, 1.0, None, 1.0, P(ws), ws.numel(), P(out), st())), None),
    }
    times = {name: [] for name in cases}
    for name, (fn, _) in cases.items():          # warm-up
        for _ in range(3):
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
    assert bool(torch.isfinite(p).all()) and bool(torch.isfinite(out).all())
    res = {"model": "OCRNet-HRNetV2-W48", "flat_floats": n, "parameters": n_real, "chunks": int(cmap.numel()), "rounds": a.rounds,
           "iters_per_round": a.iters, "device": torch.cuda.get_device_name(0),
           "note": "one launch (grad_norm_pair: two) between one pair of events; bytes = bytes_per_param x flat_floats; fraction_of_8TBps = "
                   "bytes / median / 8 TB/s; spread = the interquartile range of the case's own launches",
           "cases": {}}
    for name, (_, per) in cases.items():
        t = sorted(times[name])
        med = t[len(t) // 2]
        rec = {"median_us": round(med, 2), "min_us": round(t[0], 2), "max_us": round(t[-1], 2),
               "iqr_us": round(t[(3 * len(t)) // 4] - t[len(t) // 4], 2)}
        if per:
            rec.update({"bytes_per_param": per, "bytes": per * n, "GB_per_s": round(per * n / med * 1e-3, 1),
                        "fraction_of_8TBps": round(per * n / med * 1e-3 / 8000.0, 3)})
        res["cases"][name] = rec
        print(json.dumps({name: rec}), flush=True)
    c = res["cases"]
    diff = c["adam_ex_plain"]["median_us"] - c["adam_step"]["median_us"]
    spread = max(c["adam_step"]["iqr_us"], c["adam_ex_plain"]["iqr_us"])
    res["adam_ex_plain_minus_adam_step_us"] = round(diff, 2)
    res["adam_ex_plain_slower_beyond_spread"] = bool(diff > spread)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
