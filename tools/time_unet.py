"""Times the UNet training step (models/UNet.py of the reference, task 2; Lovasz + FusedAdam) with the record producers of BatchNorm-free
layers (plan field bnfree_records, csrc/unet.hip) on and off, and the four record kernels against the composed launches they replace:

    python3 tools/time_unet.py [--batch 8] [--rounds 5] [--steps 4] [--out profiles/unet_step_time.json]

Device events around every timed window; the two settings alternate inside every round (launch loop, then hipGraph replay); medians over
the rounds; three input batches rotate.  Per-kind kernel time comes from ops.PROFILE in one extra step per setting."""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from miccai2021_cataract_semantic_segmentation_amd import ops  # noqa: E402
from miccai2021_cataract_semantic_segmentation_amd.graph import GraphedTrainStep  # noqa: E402
from miccai2021_cataract_semantic_segmentation_amd.losses import LovaszSoftmax  # noqa: E402
from miccai2021_cataract_semantic_segmentation_amd.models import UNet  # noqa: E402
from miccai2021_cataract_semantic_segmentation_amd.optim import FusedAdam  # noqa: E402


def timed(fn, n):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for i in range(n):
        fn(i)
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / n


class Setting:
    """one model + optimiser per setting of the field (same seed: same weights); the field is switched around every call"""

    def __init__(self, on, batches):
        self.on, self.batches = on, batches
        torch.manual_seed(0)
        self.model = UNet({}, 2).cuda().train()
        self.opt = FusedAdam(self.model, lr=1e-4)
        self.crit = LovaszSoftmax({"experiment": 2})
        self.graph = None

    def eager(self, i):
        ops.BNFREE_RECORDS = self.on
        x, lbl = self.batches[i % len(self.batches)]
        self.opt.zero_grad()
        loss = self.crit(self.model(x), lbl)
        loss.backward()
        self.opt.step()
        return loss

    def capture(self):
        ops.BNFREE_RECORDS = self.on
        self.graph = GraphedTrainStep(self.model, self.crit, self.opt, *self.batches[0])

    def replay(self, i):
        return self.graph(*self.batches[i % len(self.batches)])

    def kinds(self):
        ops.PROFILE = []
        self.eager(0)
        torch.cuda.synchronize()
        agg = {}
        for k, fl, e0, e1 in ops.PROFILE:
            a = agg.setdefault(k, [0.0, 0.0, 0])
            a[0] += e0.elapsed_time(e1); a[1] += fl; a[2] += 1
        ops.PROFILE = None
        return {k: {"ms": round(ms, 4), "launches": n, "tflops_or_gbs": round(fl / ms / 1e9, 2) if ms > 0 and fl > 0 else None}
                for k, (ms, fl, n) in sorted(agg.items(), key=lambda kv: -kv[1][0])}


def kernels(B, H, W, rounds):
    """the four kernels at the level-1 shapes (64 channels at full resolution, the 128 + 64 junction) against what they replace: us and TB/s
    of the bytes each variant has to move; four tensors rotate so that nothing is served from the cache"""
    dev, C = torch.device("cuda"), 64
    zs = [torch.relu(torch.randn(B, H, W, C, device=dev)) for _ in range(4)]
    ups = [torch.randn(B, H // 2, W // 2, 128, device=dev) for _ in range(4)]
    dcat = [torch.randn(B, H, W, 192, device=dev) for _ in range(4)]
    dpool = [torch.randn(B, H // 2, W // 2, C, device=dev) for _ in range(4)]
    idx = ops.maxpool2_fwd(zs[0])[1]
    nz, nup, ncat, npool = zs[0].numel(), ups[0].numel(), dcat[0].numel(), dpool[0].numel()

    def composed_upcat(i):
        cat = torch.empty((B, H, W, 192), device=dev)
        ops.bilinear_fwd(ups[i % 4], H, W, True, out=cat[..., :128])
        ops.axpy(zs[i % 4], cat[..., 128:], 1.0, False)

    def composed_junction(i):
        d = torch.empty((B, H, W, C), device=dev)
        ops.axpy(dcat[i % 4][..., 128:], d, 1.0, False)
        ops.maxpool2_bwd(dpool[i % 4], idx, d, accumulate=True)
        ops.relu_bwd(d, zs[i % 4])

    cases = {
        "amax_record": (lambda i: ops.amax_record(zs[i % 4]), None, 4 * nz),
        "maxpool2x2_fwd_rec": (lambda i: ops.maxpool2_fwd_rec(ops.drop_amax(zs[i % 4])), lambda i: ops.maxpool2_fwd(zs[i % 4]), 4 * nz + 5 * npool),
        "upcat2x_fwd": (lambda i: ops.upcat2x_fwd(ups[i % 4], zs[i % 4]), composed_upcat, 4 * (nup + nz + ncat)),
        "relu_bwd_rec": (lambda i: ops.relu_bwd_rec(dcat[i % 4][..., :C], zs[i % 4]), lambda i: ops.relu_bwd(dcat[i % 4][..., :C], zs[i % 4]), 12 * nz),
        "relu_bwd_rec_junction": (lambda i: ops.relu_bwd_rec(dcat[i % 4][..., 128:], zs[i % 4], pool=(dpool[i % 4], idx)), composed_junction,
                                  12 * nz + 5 * npool),
    }
    out = {}
    for name, (new, old, nbytes) in cases.items():
        tn, to = [], []
        for fn in (new, old):
            if fn is not None:
                timed(fn, 4)
        for _ in range(rounds):
            tn.append(timed(new, 8))
            if old is not None:
                to.append(timed(old, 8))
        m = statistics.median(tn)
        out[name] = {"us": round(1e3 * m, 1), "tb_per_s": round(nbytes / m / 1e9, 2), "bytes": nbytes,
                     "composed_us": round(1e3 * statistics.median(to), 1) if to else None}
    return out


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--height", type=int, default=544)
    ap.add_argument("--width", type=int, default=960)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--steps", type=int, default=4)
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "unet_step_time.json"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("tools/time_unet.py measures on an MI355X: no device found")
    B, H, W = a.batch, a.height, a.width
    g = torch.Generator().manual_seed(1)
    batches = [(torch.rand(B, 3, H, W, generator=g).cuda(),
                torch.randint(0, 18, (B, H // 16, W // 16), generator=g).repeat_interleave(16, 1).repeat_interleave(16, 2).contiguous().cuda())
               for _ in range(3)]
    saved = ops.BNFREE_RECORDS
    res = {"model": "UNet, task 2 (18 logit channels), Lovasz + FusedAdam", "shape": [B, 3, H, W], "rounds": a.rounds, "steps_per_window": a.steps,
           "precision": ops.PRECISION, "runs": 1}
    try:
        S = {"on": Setting(True, batches), "off": Setting(False, batches)}
        for s in S.values():
            for i in range(2):
                s.eager(i)
        torch.cuda.synchronize()
        eager = {k: [] for k in S}
        for _ in range(a.rounds):
            for k, s in S.items():
                eager[k].append(timed(s.eager, a.steps))
        res["launch_loop_ms"] = {k: {"median": round(statistics.median(v), 3), "all": [round(t, 3) for t in v]} for k, v in eager.items()}
        res["kinds"] = {k: s.kinds() for k, s in S.items()}
        for s in S.values():
            s.capture()
        replay = {k: [] for k in S}
        for _ in range(a.rounds):
            for k, s in S.items():
                replay[k].append(timed(s.replay, a.steps))
        res["graph_replay_ms"] = {k: {"median": round(statistics.median(v), 3), "all": [round(t, 3) for t in v]} for k, v in replay.items()}
        del S
        ops.release_b3_cache()
        torch.cuda.empty_cache()
        ops.BNFREE_RECORDS = True
        res["kernels_level1"] = kernels(B, H, W, a.rounds)
    finally:
        ops.BNFREE_RECORDS = saved
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps({k: res.get(k) for k in ("shape", "launch_loop_ms", "graph_replay_ms", "kernels_level1")}))
