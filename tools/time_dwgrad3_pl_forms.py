"""A/B of the forms of the 96+ channel backward-weight kernel on planes (catseg_debug_set_dwgrad3_pl_form; csrc/dwgrad3_pl.hip) from ONE
library: catseg_dwgrad3_pl (kernel + slab reduction) at the benchmark's three branch shapes, 8 frames.  Rounds alternate between the forms in a
fixed order behind a warm-up; per form the median and the min .. max of the rounds.  Usage: python tools/time_dwgrad3_pl_forms.py [rounds] [reps]"""
import os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from miccai2021_cataract_semantic_segmentation_amd import ops
dev = torch.device("cuda")
rounds = int(sys.argv[1]) if len(sys.argv) > 1 else 5
reps = int(sys.argv[2]) if len(sys.argv) > 2 else 20
FORMS = (0, 1, 2, 3, 4)
NAMES = {0: "rows 1, builtin DMA (parent)", 1: "rows 1, late wait", 2: "rows 3, 96 co, late wait", 3: "rows 3, 48 co, late wait",
         4: "rows 3, 96 co, builtin DMA"}


def t(fn, n):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        for i in range(n):
            fn(i)
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / (n * reps) * 1e3


B = 8
for (H, W, C) in [(68, 120, 96), (34, 60, 192), (17, 30, 384)]:
    n = 4        # operand sets walked in turn: 4 x 2 x 25 MB at 96 channels, so that a launch does not find its operands in the L2
    g = torch.Generator(device=dev).manual_seed(C)
    xps = [ops.planes_from_f32(torch.randn(B, H, W, C, device=dev, generator=g)) for _ in range(n)]
    dps = [ops.planes_from_f32(torch.randn(B, H, W, C, device=dev, generator=g) * 1e-3) for _ in range(n)]
    dw = torch.empty(C, C, 3, 3, device=dev).contiguous(memory_format=torch.channels_last)
    ref, res = None, {f: [] for f in FORMS}
    try:
        for f in FORMS:                     # warm-up of every form, and the bits of every form against form 0
            ops.lib.catseg_debug_set_dwgrad3_pl_form(f)
            for i in range(n):
                ops.dwgrad3_pl(xps[i], dps[i], dw)
            torch.cuda.synchronize()
            ref = dw.clone() if f == 0 else ref
            assert torch.equal(dw, ref), "form %d differs from form 0" % f
        for _ in range(rounds):
            for f in FORMS:
                ops.lib.catseg_debug_set_dwgrad3_pl_form(f)
                res[f].append(t(lambda i: ops.dwgrad3_pl(xps[i], dps[i], dw), n))
    finally:
        ops.lib.catseg_debug_set_dwgrad3_pl_form(-1)
    gf = 2.0 * B * H * W * C * C * 9 / 1e9
    print("C=%3d B=%d %dx%d, kernel + slab reduction, us per call (%d rounds of %d calls):" % (C, B, H, W, rounds, n * reps))
    for f in FORMS:
        v = sorted(res[f])
        print("   form %d %-30s median %6.1f  min %6.1f  max %6.1f   (%.2f of the three-product peak at the median)"
              % (f, NAMES[f], v[len(v) // 2], v[0], v[-1], gf * 1e3 / v[len(v) // 2] / 833.3), flush=True)
    del xps, dps
    ops.release_b3_cache()
