"""Times forward + backward of SoftIoU, GenDiceLoss ('auto') and FocalLoss (gamma 2, alpha) at the bench shape (8 x 25 x 544 x 960,
P = 4 177 920, NHWC logits), with device events, alternating with the fp32 torch-ops restatement (tests/_overlap_ref.py) on the same
device.  Per call the algorithmic bytes are 418 MB logits + 33 MB labels read forward, the same again plus 418 MB of dlogits written
backward: 1.32 GB.  Prints one JSON line.  Kernel times of their own: rocprofv3 --kernel-trace --stats -- python tools/time_overlap_losses.py"""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import torch  # noqa: E402

import _overlap_ref as R  # noqa: E402
from miccai2021_cataract_semantic_segmentation_amd import losses  # noqa: E402

B, K, H, W = 8, 25, 544, 960
P = B * H * W
BYTES = {"fwd": 4.0 * P * K + 8.0 * P, "bwd": 8.0 * P * K + 8.0 * P}
dev = torch.device("cuda")
torch.manual_seed(0)
lbl = torch.randint(0, K + 1, (B, H // 16, W // 16), device=dev).repeat_interleave(16, 1).repeat_interleave(16, 2)
onehot = torch.nn.functional.one_hot(lbl.clamp(max=K - 1), K).permute(0, 3, 1, 2).float()
logits = (torch.randn(B, K, H, W, device=dev) * 2 + onehot * 4).contiguous(memory_format=torch.channels_last)
del onehot
x = logits.clone().requires_grad_()
up = torch.ones((), device=dev)
CASES = [("SoftIoU", {"experiment": 3}), ("GenDiceLoss", {"experiment": 3, "weights": "auto"}),
         ("FocalLoss", {"experiment": 3, "gamma": 2, "alpha": [0.5 + 0.05 * i for i in range(K)]})]


def hip_step(crit):
    x.grad = None
    loss = crit(x, lbl)
    loss.backward(up)


def torch_step(name, cfg):
    x.grad = None
    loss = R.loss_of(name, cfg, x, lbl)
    loss.backward(up)


def timed(fn, n):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(n):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / n * 1e3     # us


res = {"shape": [B, K, H, W], "bytes_per_call_GB": (BYTES["fwd"] + BYTES["bwd"]) / 1e9, "losses": {}}
for name, cfg in CASES:
    crit = getattr(losses, name)(dict(cfg))
    for _ in range(3):
        hip_step(crit)
        torch_step(name, cfg)
    torch.cuda.synchronize()
    th, tt = [], []
    for _ in range(5):                                     # alternating rounds
        th.append(timed(lambda: hip_step(crit), 10))
        tt.append(timed(lambda: torch_step(name, cfg), 3))
    th.sort()
    tt.sort()
    res["losses"][name] = {"hip_fwd_bwd_us_median": th[2], "hip_fwd_bwd_us_min": th[0], "torch_fp32_fwd_bwd_us_median": tt[2],
                           "speedup": tt[2] / th[2], "hip_effective_TBps": (BYTES["fwd"] + BYTES["bwd"]) / (th[2] * 1e-6) / 1e12}
print(json.dumps(res), flush=True)
