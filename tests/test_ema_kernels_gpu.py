"""The kernels of include/catseg_ema.h on the GPU: catseg_ema_update against torch.lerp evaluated on the CPU in fp64, with its fp32
evaluation as the yardstick (tests/_yardstick.within, the bar of tests/test_optim_kernels_gpu.py); catseg_ema_swap exactly; catseg_ema_table
over ~700 small buffers with 4-byte aligned live pointers and gaps in the shadow.

Run with -s to collect the RATIO lines."""
import os
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

f32 = lambda x: float(np.float32(x))
SIZES = [1, 3, 6, 64, 65, 1003, "sweep+1"]
WEIGHTS = [1.0, 0.5, f32(1 / 7), f32(0.1), f32(1e-4)]          # the C ABI takes float: the values the kernels see, on both sides
CANARY = 8


def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")


def _ops():
    from miccai2021_cataract_semantic_segmentation_amd import ops
    return ops


def _n(n):
    from miccai2021_cataract_semantic_segmentation_amd import _lib
    return _lib.lib.catseg_ema_grid_cap() * 256 * 4 + 1 if n == "sweep+1" else n        # one sweep of the capped grid plus one element


def _bits(t):
    return t.detach().cpu().view(torch.int32)


@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("w", WEIGHTS)
def test_update_against_fp64(n, w):
    """ten successive updates from a zero shadow.  w = 1 writes the bits of p; the by-value form, a second by-value run and the
    device-scalar form agree bit for bit; every fifth element is padding (p = 0 throughout) and stays exactly 0; the elements behind n
    are untouched"""
    _need_gpu()
    from _yardstick import within
    ops = _ops()
    n = _n(n)
    gen = torch.Generator().manual_seed(n % 1009 + int(w * 1000))
    pad = torch.arange(n) % 5 == 4
    shadows = [torch.zeros(n + CANARY, device="cuda") for _ in range(3)]
    for s in shadows:
        s[n:] = -7.0
    w_dev = torch.tensor([w, 55.0], dtype=torch.float32, device="cuda")
    a64, a32 = torch.zeros(n, dtype=torch.float64), torch.zeros(n)
    for step in range(10):
        p = torch.randn(n, generator=gen) * (1.0 + step)
        p[pad] = 0.0
        p_dev = torch.cat([p, torch.full((CANARY,), 3.0)]).cuda()
        ops.ema_update(p_dev[:n], shadows[0][:n], w)
        ops.ema_update(p_dev[:n], shadows[1][:n], w)
        ops.ema_update(p_dev[:n], shadows[2][:n], w_dev)
        a64 = torch.lerp(a64, p.double(), w)
        a32 = torch.lerp(a32, p, w)
        torch.cuda.synchronize()
        got = shadows[0].cpu()
        assert torch.equal(_bits(shadows[0]), _bits(shadows[1])), "two launches differ"
        assert torch.equal(_bits(shadows[0]), _bits(shadows[2])), "the by-value and the device-scalar form differ"
        assert bool((got[n:] == -7.0).all()) and bool((p_dev[n:] == 3.0).all()), "an element behind n was written"
        assert not bool(got[:n][pad].any()) and torch.equal(_bits(got[:n][pad]), torch.zeros(int(pad.sum()), dtype=torch.int32)), "padding moved"
        if w == 1.0:
            assert torch.equal(_bits(got[:n]), _bits(p)), "w = 1 is not the copy"
        else:
            within("ema_update", "n %d w %g step%d" % (n, w, step + 1), got[:n], a64, a32)


@pytest.mark.parametrize("n", SIZES)
def test_swap_is_exact_and_an_involution(n):
    _need_gpu()
    ops = _ops()
    n = _n(n)
    gen = torch.Generator().manual_seed(n % 1009)
    a0, b0 = torch.randn(n + CANARY, generator=gen), torch.randn(n + CANARY, generator=gen)
    a0[0], b0[0] = -0.0, float("inf")                                      # bits travel, not values
    a, b = a0.cuda(), b0.cuda()
    ops.ema_swap(a[:n], b[:n])
    torch.cuda.synchronize()
    assert torch.equal(_bits(a[:n]), _bits(b0[:n])) and torch.equal(_bits(b[:n]), _bits(a0[:n]))
    assert torch.equal(_bits(a[n:]), _bits(a0[n:])) and torch.equal(_bits(b[n:]), _bits(b0[n:])), "an element behind n was written"
    ops.ema_swap(a[:n], b[:n])
    torch.cuda.synchronize()
    assert torch.equal(_bits(a), _bits(a0)) and torch.equal(_bits(b), _bits(b0))


def test_table_update_and_swap():
    """~700 entries of sizes {1, 3, 18, 48, 64, 65, 2048, 2049}, every third live buffer a view one float into its allocation, gaps of
    0..5 floats between the entries' slices of the shadow.  Mode 0 against fp64 with the bar of test_update_against_fp64 (by-value and
    device-scalar forms bit-identical); mode 1 exact and an involution; the gaps are never written."""
    _need_gpu()
    from _yardstick import within
    ops = _ops()
    rng = np.random.RandomState(11)
    gen = torch.Generator().manual_seed(11)
    sizes = rng.choice([1, 3, 18, 48, 64, 65, 2048, 2049], size=701)
    assert set(sizes.tolist()) == {1, 3, 18, 48, 64, 65, 2048, 2049}
    allocs, lives, rec, off = [], [], [], int(rng.randint(0, 6))
    for i, n in enumerate(sizes.tolist()):
        shift = 1 if i % 3 == 0 else 0
        base = torch.full((n + shift + 1,), -5.0, device="cuda")           # one canary float behind (and, shifted, one in front of) the view
        allocs.append(base)
        lives.append(base[shift:shift + n])
        rec.append((lives[-1].data_ptr(), off, n, 0))
        off += n + int(rng.randint(0, 6))
    assert any(r[0] % 16 == 4 for r in rec), "no live pointer is only 4-byte aligned"
    total = off
    table = torch.from_numpy(np.array(rec, dtype=ops.EMA_ENTRY).view(np.uint8).copy()).cuda()
    gap = torch.ones(total, dtype=torch.bool)
    for _, o, n, _ in rec:
        gap[o:o + n] = False
    assert int(gap.sum()) > 100

    def shadow0():
        s = torch.zeros(total)
        s[gap] = 9.0
        return s.cuda()

    def gather(s):
        s = s.cpu()
        return torch.cat([s[o:o + n] for _, o, n, _ in rec])

    sh, sh_dev = shadow0(), shadow0()
    a64 = torch.zeros(int(sizes.sum()), dtype=torch.float64)
    a32 = a64.float()
    for step, w in enumerate([1.0, 0.5, f32(1 / 7), f32(0.1), f32(1e-4)]):
        vals = [torch.randn(n, generator=gen) for n in sizes.tolist()]
        for t, v in zip(lives, vals):
            t.copy_(v)
        p = torch.cat(vals)
        ops.ema_table(table, len(rec), sh, ops.EMA_LERP, w)
        ops.ema_table(table, len(rec), sh_dev, ops.EMA_LERP, torch.tensor([w], dtype=torch.float32, device="cuda"))
        a64, a32 = torch.lerp(a64, p.double(), w), torch.lerp(a32, p, w)
        torch.cuda.synchronize()
        assert torch.equal(_bits(sh), _bits(sh_dev)), "the by-value and the device-scalar form differ"
        assert bool((sh.cpu()[gap] == 9.0).all()), "a gap of the shadow was written"
        assert torch.equal(torch.cat([t.cpu() for t in lives]), p), "mode 0 wrote a live buffer"
        if w == 1.0:
            assert torch.equal(_bits(gather(sh)), _bits(p))
        else:
            within("ema_table", "w %g step%d" % (w, step + 1), gather(sh), a64, a32)
    # ---- mode 1: exact, an involution
    before_live, before_sh = torch.cat([t.cpu() for t in lives]), sh.cpu().clone()
    ops.ema_table(table, len(rec), sh, ops.EMA_SWAP)
    torch.cuda.synchronize()
    assert torch.equal(_bits(torch.cat([t.cpu() for t in lives])), _bits(gather(before_sh)))
    assert torch.equal(_bits(gather(sh)), _bits(before_live))
    assert bool((sh.cpu()[gap] == 9.0).all())
    ops.ema_table(table, len(rec), sh, ops.EMA_SWAP)
    torch.cuda.synchronize()
    assert torch.equal(_bits(torch.cat([t.cpu() for t in lives])), _bits(before_live)) and torch.equal(_bits(sh), _bits(before_sh))
    for base, live in zip(allocs, lives):
        assert float(base[-1]) == -5.0 and (live.data_ptr() == base.data_ptr() or float(base[0]) == -5.0), "a float next to a live buffer was written"


def test_refusals_with_device_buffers():
    """CATSEG_EINVAL before anything is launched: the buffers are untouched afterwards"""
    _need_gpu()
    from miccai2021_cataract_semantic_segmentation_amd import _lib
    lib = _lib.lib
    n = 1000
    p, a = torch.full((n + 4,), 1.0, device="cuda"), torch.full((n + 4,), 2.0, device="cuda")
    st = torch.cuda.current_stream().cuda_stream
    P = lambda t, off=0: t.data_ptr() + off
    calls = [lambda: lib.catseg_ema_update(P(p, 4), P(a), n, 0.5, None, st), lambda: lib.catseg_ema_update(P(p), P(a), 0, 0.5, None, st),
             lambda: lib.catseg_ema_update(P(p), P(a), n, 1.5, None, st), lambda: lib.catseg_ema_update(P(p), P(a), n, float("nan"), None, st),
             lambda: lib.catseg_ema_swap(P(p), P(a, 8), n, st), lambda: lib.catseg_ema_swap(P(p), None, n, st),
             lambda: lib.catseg_ema_table(P(p), 0, P(a), 0, 0.5, None, st), lambda: lib.catseg_ema_table(P(p), 1, P(a), 2, 0.5, None, st),
             lambda: lib.catseg_ema_table(None, 1, P(a), 0, 0.5, None, st), lambda: lib.catseg_ema_table(P(p), 1, None, 0, 0.5, None, st),
             lambda: lib.catseg_ema_table(P(p), 1, P(a), 0, -0.5, None, st)]
    for call in calls:
        assert call() == 1 and lib.catseg_last_error().startswith(b"catseg_ema_")
    torch.cuda.synchronize()
    assert bool((p == 1.0).all()) and bool((a == 2.0).all())
