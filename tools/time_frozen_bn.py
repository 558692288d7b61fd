"""Times the frozen-statistics BatchNorm backward (the `frozen` form of catseg_bn_backward: one streaming pass + a small merge) against the
training form (partial sums, merge, apply: two passes over dz and y) on the same tensors in the same run, with HIP events around single
calls, at the head and trunk shapes of the bench step (rows = 8 x 136 x 240):
    relu_c512 / relu_c48      ReLU, no residual branch: the mask recomputed from y (training 5 tensor transfers, frozen 3)
    res_bits_c512 / _c48      residual branch, the ReLU mask read as bits, dres written (training 6 + 2/32, frozen 4 + 1/32)
    bn_apply_c512 / _c48      catseg_bn_apply (y -> z), the project's own streaming yardstick, measured again here
The cases alternate inside a round, every case rotates over three sets of buffers (a 512-channel tensor is 535 MB, past the 256 MB
last-level cache), medians over all calls are reported beside the algorithmic bytes from shapes and the fraction of 8 TB/s they reach.

Then the training step of OCRNet-ResNet50 at the bench shape (--batch x 3 x --height x --width) with config['freeze_bn'] absent, "backbone"
and "all", eager and as a hipGraph, in alternating rounds of --step-iters steps between one pair of events.  One run is one run: the spread
columns are those of this run's own calls.
    python tools/time_frozen_bn.py [--rounds 7] [--iters 10] [--no-steps] [--out profiles/frozen_bn_time.json]"""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402
from miccai2021_cataract_semantic_segmentation_amd import ops  # noqa: E402

EPS = 1e-5


def summary(t, nbytes=None):
    t = sorted(t)
    med = t[len(t) // 2]
    rec = {"median_us": round(med, 2), "min_us": round(t[0], 2), "max_us": round(t[-1], 2), "iqr_us": round(t[(3 * len(t)) // 4] - t[len(t) // 4], 2)}
    if nbytes:
        rec.update({"bytes": nbytes, "GB_per_s": round(nbytes / med * 1e-3, 1), "fraction_of_8TBps": round(nbytes / med * 1e-3 / 8000.0, 3)})
    return rec


def kernel_cases(rows, C, dev, gen, nsets=3):
    """{name: (callable, algorithmic bytes)} on `nsets` rotating sets of tensors of one width"""
    n = rows * C
    rm, rv = torch.randn(C, device=dev, generator=gen), 0.5 + torch.rand(C, device=dev, generator=gen)
    gamma, beta = 1 + 0.3 * torch.randn(C, device=dev, generator=gen), 0.3 * torch.randn(C, device=dev, generator=gen)
    scale = ops.bn_eval_scale(gamma, rv, EPS)
    stats = torch.cat([rm, 1 / torch.sqrt(rv + EPS)])             # the training form handed the same mean and invstd
    dg, db = torch.empty(C, device=dev), torch.empty(C, device=dev)
    sets = []
    for _ in range(nsets):
        s = {"y": torch.randn(rows, C, device=dev, generator=gen) * torch.sqrt(rv) + rm, "dz": torch.randn(rows, C, device=dev, generator=gen),
             "res": torch.randn(rows, C, device=dev, generator=gen), "dy": torch.empty(rows, C, device=dev), "dres": torch.empty(rows, C, device=dev)}
        s["z"] = ops.bn_apply(s["y"], rm, scale, beta, s["res"], True, want_mask=True)        # z = relu(bn(y) + res) with its mask as bits
        assert getattr(s["z"], "_relu_mask", None) is not None
        sets.append(s)
    turn = {"i": 0}

    def cur():
        turn["i"] += 1
        return sets[turn["i"] % nsets]

    def train_relu():
        s = cur()
        ops.bn_backward(s["dz"], None, s["y"], stats, gamma, True, dg, db, dy_out=s["dy"], beta=beta)

    def frozen_relu():
        s = cur()
        ops.bn_backward_frozen(s["dz"], None, s["y"], rm, rv, EPS, scale, True, dg, db, dy_out=s["dy"], beta=beta)

    def train_res():
        s = cur()
        ops.bn_backward(s["dz"], s["z"], s["y"], stats, gamma, True, dg, db, s["dres"], False, dy_out=s["dy"], beta=beta)

    def frozen_res():
        s = cur()
        ops.bn_backward_frozen(s["dz"], s["z"], s["y"], rm, rv, EPS, scale, True, dg, db, s["dres"], False, dy_out=s["dy"], beta=beta)

    def apply():
        s = cur()
        ops.bn_apply(s["y"], rm, scale, beta, None, True, out=s["dy"])
    t = 4.0 * n
    return {"relu_c%d_training" % C: (train_relu, 5 * t), "relu_c%d_frozen" % C: (frozen_relu, 3 * t),
            "res_bits_c%d_training" % C: (train_res, 6 * t + 2 * n / 8.0), "res_bits_c%d_frozen" % C: (frozen_res, 4 * t + n / 8.0),
            "bn_apply_c%d" % C: (apply, 2 * t)}


def kernel_times(a, dev):
    rows = 8 * 136 * 240
    gen = torch.Generator(device="cuda").manual_seed(0)
    out = {"rows": rows, "cases": {}}
    for C in (512, 48):
        cases = kernel_cases(rows, C, dev, gen)
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
        for name, (_, nbytes) in cases.items():
            out["cases"][name] = summary(times[name], nbytes)
            print(json.dumps({name: out["cases"][name]}), flush=True)
        for form in ("relu", "res_bits"):
            tr, fr = out["cases"]["%s_c%d_training" % (form, C)], out["cases"]["%s_c%d_frozen" % (form, C)]
            out["%s_c%d_frozen_over_training" % (form, C)] = {"time": round(fr["median_us"] / tr["median_us"], 3),
                                                              "bytes": round(fr["bytes"] / tr["bytes"], 3),
                                                              "rate_per_byte": round(fr["GB_per_s"] / tr["GB_per_s"], 3)}
        del cases
        torch.cuda.empty_cache()
    return out


def step_times(a, dev):
    from miccai2021_cataract_semantic_segmentation_amd.graph import GraphedTrainStep
    from miccai2021_cataract_semantic_segmentation_amd.losses import TwoScaleLoss
    from miccai2021_cataract_semantic_segmentation_amd.models import OCRNet
    from miccai2021_cataract_semantic_segmentation_amd.optim import FusedAdam
    crit = TwoScaleLoss({"experiment": 3, "interm": {"name": "LovaszSoftmax", "args": [], "weight": 0.4},
                         "final": {"name": "LovaszSoftmax", "args": [], "weight": 1.0}})
    img, lbl = bench.synth_batch(a.batch, a.height, a.width, 25, 1000, dev)
    runs, frozen = {}, {}
    for key, select in (("none", None), ("backbone", "backbone"), ("all", "all")):
        torch.manual_seed(0)
        cfg = dict(bench.MODELS["ocrnet_r50"][0])
        if select is not None:
            cfg["freeze_bn"] = select
        model = OCRNet(cfg, 3).to(dev).train()
        opt = FusedAdam(model, lr=1e-4)
        frozen[key] = len(model.frozen_bn)
        runs[key] = (model, opt, GraphedTrainStep(model, lambda o, l: crit(o[0], o[1], l), opt, img, lbl))

    def eager(model, opt):
        opt.zero_grad()
        crit(*model(img), lbl).backward()
        opt.step()
    cases = {}
    for key, (model, opt, g) in runs.items():
        cases["eager_" + key] = (lambda model=model, opt=opt: eager(model, opt))
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
    out = {"network": "OCRNet-ResNet50 OS8 (bench.MODELS['ocrnet_r50'])", "input": [a.batch, 3, a.height, a.width], "rounds": a.step_rounds,
           "steps_per_round": a.step_iters, "frozen_modules": frozen, "not_measured": ["OCRNet-HRNetV2-W48", "data parallel"],
           "note": "per-step time = one pair of events around steps_per_round steps; the six cases alternate inside a round", "cases": {}}
    for name in cases:
        out["cases"][name] = summary(times[name])
        print(json.dumps({name: out["cases"][name]}), flush=True)
    for form in ("eager", "graph"):
        for key in ("backbone", "all"):
            out["%s_%s_minus_none_us" % (form, key)] = round(out["cases"]["%s_%s" % (form, key)]["median_us"] - out["cases"][form + "_none"]["median_us"], 1)
    for _, _, g in runs.values():
        g.release()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--no-steps", action="store_true")
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--height", type=int, default=544)
    ap.add_argument("--width", type=int, default=960)
    ap.add_argument("--step-rounds", type=int, default=5)
    ap.add_argument("--step-iters", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "frozen_bn_time.json"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("time_frozen_bn.py measures on the GPU: none found")
    dev = torch.device("cuda")
    res = {"rounds": a.rounds, "iters_per_round": a.iters, "device": torch.cuda.get_device_name(0),
           "note": "one call (training form: three launches; frozen form: two) between one pair of events; fraction_of_8TBps = bytes / median / "
                   "8 TB/s; iqr = the interquartile range of the case's own calls; one run"}
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
