"""What Dropout2d costs inside the fused head kernels (csrc/headfuse.h, DROP) against the pass it replaces (csrc/dropout.hip,
catseg_dropout2d_apply), at the bench's head shape: 8 x 136 x 240 pixels, 512 channels, 25 classes.

One process times, interleaved round by round with HIP events around every call and inputs rotated through tensors that together exceed the
256 MB last-level cache:  head_fwd / head_backward without dropout, the same with a p = 0.5 mask, dropout2d_apply.  Medians over the rounds.
    python3 tools/time_headfuse_dropout.py [--root TREE] [--rounds N] [--json FILE]
--root: import the package from another checkout (a build of the parent commit: it has no dropout, only the first two rows are timed)."""
import argparse
import json
import os
import statistics
import sys

ap = argparse.ArgumentParser()
ap.add_argument("--root", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
ap.add_argument("--rounds", type=int, default=15)
ap.add_argument("--json", default=None)
args = ap.parse_args()
sys.path.insert(0, os.path.abspath(args.root))
import torch  # noqa: E402
from miccai2021_cataract_semantic_segmentation_amd import ops  # noqa: E402

dev = torch.device("cuda")
B, H, W, C, K, NBUF = 8, 136, 240, 512, 25, 3          # 535 MB per activation: three of them rotate
has_drop = hasattr(ops, "dropout2d_apply")
y = [torch.randn(B, H, W, C, device=dev) for _ in range(NBUF)]
gamma, beta = 1 + 0.1 * torch.randn(C, device=dev), 0.1 * torch.randn(C, device=dev)
stats, scale = ops.bn_train_stats(y[0], gamma, 1e-5, 0.1, torch.zeros(C, device=dev), torch.ones(C, device=dev))
wh, bh = torch.randn(K, C, 1, 1, device=dev) * 0.05, torch.randn(K, device=dev)
dl = [ops.new_act(B, H, W, K, dev, ld=32, zero=True) for _ in range(NBUF)]
for t in dl:
    t.copy_(torch.randn(B, H, W, K, device=dev) * 1e-5)
dwh, dbh, dg, db = torch.empty(K, C, 1, 1, device=dev), torch.empty(K, device=dev), torch.empty(C, device=dev), torch.empty(C, device=dev)
calls = {"head_fwd": lambda i: ops.head_fwd(y[i], stats[:C], scale, beta, wh, bh, K, 32),
         "head_backward": lambda i: ops.head_backward(dl[i], y[i], stats, gamma, beta, wh, dwh, dbh, dg, db, None)}
if has_drop:
    dm = ops.dropout2d_mask_fixed((torch.rand(B, C, device=dev) >= 0.5).float(), 0.5)
    out = torch.empty(B, H, W, C, device=dev)
    calls["head_fwd_drop"] = lambda i: ops.head_fwd(y[i], stats[:C], scale, beta, wh, bh, K, 32, drop=dm)
    calls["head_backward_drop"] = lambda i: ops.head_backward(dl[i], y[i], stats, gamma, beta, wh, dwh, dbh, dg, db, None, drop=dm)
    calls["dropout2d_apply"] = lambda i: ops.dropout2d_apply(y[i], dm, out=out)
for name, fn in calls.items():          # warm-up: workspaces, code objects
    for i in range(NBUF):
        fn(i)
torch.cuda.synchronize()
times = {name: [] for name in calls}
for r in range(args.rounds):
    events = []
    for name, fn in calls.items():
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn(r % NBUF)
        e1.record()
        events.append((name, e0, e1))
    torch.cuda.synchronize()
    for name, e0, e1 in events:
        times[name].append(e0.elapsed_time(e1) * 1e3)
res = {"shape": [B, H, W, C, K], "rounds": args.rounds, "root": os.path.abspath(args.root),
       "us": {n: {"median": statistics.median(v), "min": min(v), "max": max(v)} for n, v in times.items()}}
if has_drop:
    u = res["us"]
    res["extra_us"] = {"forward": u["head_fwd_drop"]["median"] - u["head_fwd"]["median"],
                       "backward": u["head_backward_drop"]["median"] - u["head_backward"]["median"],
                       "separate_pass_forward_or_backward": u["dropout2d_apply"]["median"]}
print(json.dumps(res))
if args.json:
    with open(args.json, "w") as f:
        json.dump(res, f, indent=1)
