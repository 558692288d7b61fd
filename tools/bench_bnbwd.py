"""standalone times of the two routes through the backward of relu(bn1(.)) -> conv2: (a) plain backward-data + catseg_bn_backward,
(b) catseg_dconv3_bnbwd + catseg_bn_backward from its partials, at the HRNet-W48 trunk shapes of the bs-8 step"""
import os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from miccai2021_cataract_semantic_segmentation_amd import ops
dev = torch.device("cuda")
def timeit(fn, n=30):
    for _ in range(3): fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(n): fn()
    e1.record(); torch.cuda.synchronize()
    return e0.elapsed_time(e1) / n * 1e3
ops.PRECISION = "bf16x3"
for (B, H, W, C) in [(8, 136, 240, 48), (8, 68, 120, 96), (8, 34, 60, 192), (8, 17, 30, 384), (8, 136, 240, 64)]:
    q = torch.randn(B, H, W, C, device=dev)
    dy = torch.randn(B, H, W, C, device=dev)
    w = (torch.randn(C, C, 3, 3, device=dev) * 0.05).contiguous(memory_format=torch.channels_last)
    gam, bet = torch.rand(C, device=dev) + 0.5, torch.randn(C, device=dev) * 0.3
    stats, _ = ops.bn_train_stats(q, gam, 1e-5, 0.1, torch.zeros(C, device=dev), torch.ones(C, device=dev))
    out = torch.empty_like(q); dq = torch.empty_like(q)
    dg, db = torch.empty(C, device=dev), torch.empty(C, device=dev)
    t_a1 = timeit(lambda: ops.conv_bwd_data(dy, w, (B, H, W, C), 3, 3, 1, 1, 1, out=out))
    t_a2 = timeit(lambda: ops.bn_backward(out, None, q, stats, gam, True, dg, db, beta=bet, dy_out=dq))
    r = ops.conv_bwd_data(dy, w, (B, H, W, C), 3, 3, 1, 1, 1, out=out, bn_src=(q, stats, gam, bet))
    t_b1 = timeit(lambda: ops.conv_bwd_data(dy, w, (B, H, W, C), 3, 3, 1, 1, 1, out=out, bn_src=(q, stats, gam, bet)))
    t_b2 = timeit(lambda: ops.bn_backward_pre(r[0], q, stats, gam, r[1], dg, db, dq_out=dq))
    print("C=%3d %dx%d: backward-data %.1f + bn_backward %.1f = %.1f us | fused backward-data %.1f + merge/apply %.1f = %.1f us"
          % (C, H, W, t_a1, t_a2, t_a1 + t_a2, t_b1, t_b2, t_b1 + t_b2), flush=True)
