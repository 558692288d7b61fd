"""The tile forms of the 96+ channel backward-weight kernel on planes (csrc/dwgrad3_pl.hip, catseg_debug_set_dwgrad3_pl_form): every form --
the LDS-DMA awaited behind the MFMAs, all three filter rows in one block -- against form 0 (one filter row per block, the builtin LDS-DMA)
on the same planes and records, BIT FOR BIT: the split count, the 32-pixel K-steps, the product order and the slab order are those of form 0,
so no tolerance is involved.  Form by form against fp64 on one ragged shape, with the bound of tests/test_dwgrad3_pl_gpu.py."""
import functools
import inspect
import re

import pytest
import torch

import test_dwgrad3_pl_gpu as parent_tests

pytestmark = pytest.mark.gpu

FORMS = [1, 2, 3, 4]
# (B, H, W): ragged in both directions, the last tile row partly below the image; exactly two tile rows and one tile column; several splits
# per frame boundary
SHAPES = [(2, 9, 17), (1, 4, 16), (3, 6, 40)]
CHANNELS = [96, 192, 384]


def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")


def _fp64_bound():
    """the relative bound test_dwgrad3_pl_vs_fp64 asserts (its `assert e <= ...` line): reused, not chosen here"""
    m = re.search(r"assert e <= ([0-9.e+-]+), e", inspect.getsource(parent_tests.test_dwgrad3_pl_vs_fp64))
    return float(m.group(1))


@functools.lru_cache(maxsize=None)
def _case(C, B, H, W, log2_scale=0):
    """planes of x and dy (seeded) and dw of every form: {form: tensor}; computed once per case"""
    from miccai2021_cataract_semantic_segmentation_amd import ops
    dev = torch.device("cuda")
    g = torch.Generator().manual_seed(1000 * C + 10 * W + B)
    x = torch.randn(B, H, W, C, generator=g) * torch.exp(torch.randn(C, generator=g) * 1.5) * 2.0 ** log2_scale
    dy = torch.randn(B, H, W, C, generator=g) * torch.exp(torch.randn(C, generator=g)) * 2.0 ** (log2_scale - 10)
    xp, dyp = ops.planes_from_f32(x.to(dev)), ops.planes_from_f32(dy.to(dev))
    out = {}
    try:
        for form in [0] + FORMS:
            ops.lib.catseg_debug_set_dwgrad3_pl_form(form)
            dw = torch.full((C, C, 3, 3), float("nan"), device=dev).contiguous(memory_format=torch.channels_last)
            ops.dwgrad3_pl(xp, dyp, dw)
            torch.cuda.synchronize()
            out[form] = dw
    finally:
        ops.lib.catseg_debug_set_dwgrad3_pl_form(-1)
    return xp, dyp, out


def _dequantised(p):
    """fp64 value of every element of a Planes object: (high + low) * 2^-exponent; planes [2][C / 8][P][8] of fp16"""
    B, H, W, C = p.shape
    pl = p.buf[: 2 * B * H * W * C * 2].view(torch.float16).view(2, C // 8, B * H * W, 8).double()
    ex = int(p.rec.view(torch.int32)[1])                 # CS_REC_EXP
    v = (pl[0] + pl[1]) * 2.0 ** (-ex)
    return v.permute(1, 0, 2).reshape(B, H, W, C).cpu()


@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("shape", SHAPES)
@pytest.mark.parametrize("C", CHANNELS)
def test_forms_bit_identical_to_form0(C, shape, form):
    _need_gpu()
    _, _, out = _case(C, *shape)
    assert torch.isfinite(out[0]).all()
    assert torch.equal(out[form], out[0]), float((out[form] - out[0]).abs().max())


@pytest.mark.parametrize("form", [0] + FORMS)
def test_forms_vs_fp64_of_own_operands(form):
    """dw[o][ky][kx][c] = sum dy * x evaluated in fp64 from the dequantised planes: the kernel held to its own operands"""
    _need_gpu()
    C, shape = 96, SHAPES[0]
    xp, dyp, out = _case(C, *shape)
    x, dy = _dequantised(xp).permute(0, 3, 1, 2), _dequantised(dyp).permute(0, 3, 1, 2)
    ref = torch.nn.grad.conv2d_weight(x, (C, C, 3, 3), dy, 1, 1)
    e = float((out[form].cpu().double() - ref).abs().max()) / float(ref.abs().max())
    print("form %d: max |dw - fp64| / max |fp64| = %.3g" % (form, e))
    assert e <= _fp64_bound(), e


@pytest.mark.parametrize("form", FORMS)
def test_forms_exponent_corner(form):
    """ex_x + ex_d outside +-120 (two ldexp steps on the way out instead of one multiplication): bit-identical to form 0 too"""
    _need_gpu()
    xp, dyp, out = _case(96, *SHAPES[0], log2_scale=-52)
    ex = int(xp.rec.view(torch.int32)[1]) + int(dyp.rec.view(torch.int32)[1])
    assert abs(ex) > 120, ex
    assert torch.isfinite(out[0]).all() and float(out[0].abs().max()) > 0
    assert torch.equal(out[form], out[0])
