"""The measured bound that the kernel tests against float64 share (tests/test_small_kernels_gpu.py, tests/test_batchnorm_gpu.py).

The bound of a floating-point comparison is measured, not chosen: the reference lines run in float32 on the CPU give the yardstick
`e32 = max |ref32 - ref64|`, and the kernel may be off by at most 4 x e32, with a floor of 4 ulp (2^-23) of the reference's scale where
the float32 CPU result happens to be exact -- both scaled as close() of test_kernels_gpu.py scales an error, by max |ref64|."""
import torch

EPS32 = 2.0 ** -23
WORST = {}      # kernel -> (worst ratio of the kernel's error to the yardstick, case): printed by every check (run with -s to collect)


def within(kernel, case, got, ref64, ref32):
    """max |got - ref64| <= max(4 max |ref32 - ref64|, 4 ulp of max |ref64|)"""
    got, ref64, ref32 = got.detach().cpu().double(), ref64.detach().double(), ref32.detach().double()
    assert got.shape == ref64.shape == ref32.shape, (got.shape, ref64.shape, ref32.shape)
    assert torch.isfinite(ref64).all() and torch.isfinite(ref32).all(), "%s %s: the reference is not finite" % (kernel, case)
    assert torch.isfinite(got).all(), "%s %s: the kernel wrote inf / nan" % (kernel, case)
    scale = ref64.abs().max().item() + 1e-12
    err, e32 = (got - ref64).abs().max().item(), (ref32 - ref64).abs().max().item()
    yard = max(e32, EPS32 * scale)
    ratio = err / yard
    if ratio > WORST.get(kernel, (-1.0, None))[0]:
        WORST[kernel] = (ratio, case)
    print("RATIO %-22s %-40s err %.3e  fp32-cpu %.3e  scale %.3e  ratio %.3f  (worst so far %.3f)" % (kernel, case, err, e32, scale, ratio, WORST[kernel][0]))
    assert err <= 4 * yard, "%s %s: max abs err %g > 4 x yardstick %g (fp32 CPU err %g, ref scale %g)" % (kernel, case, err, yard, e32, scale)
