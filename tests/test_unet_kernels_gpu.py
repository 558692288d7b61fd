"""The streaming kernels of csrc/unet.hip against the existing kernels they fuse, bit for bit, and their amax records against the bits of
max|.| over the valid columns of what they wrote or read."""
import pytest
import torch

pytestmark = pytest.mark.gpu

PAD = 1e30      # what the pad columns of a strided view hold: a kernel that read them would raise its record to it


def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")


def _record_bits(rec):
    """the value a consumer takes from a record: the maximum over its 16 slots (128 bytes apart)"""
    return int(rec.view(16, 32)[:, 0].max())


def _amax_bits(*tensors):
    """bits of max|.| over the valid columns of the tensors"""
    m = max(float(t.abs().max()) for t in tensors)
    return int(torch.tensor(m, dtype=torch.float32).view(torch.int32))


def _rand(shape, seed, strided=False, relu=False):
    """random NHWC tensor on the device: dense, or a view with ld = C + 4 whose pad columns hold PAD"""
    g = torch.Generator().manual_seed(seed)
    t = torch.randn(shape, generator=g)
    if relu:
        t = torch.relu(t)
    if not strided:
        return t.cuda()
    buf = torch.full(tuple(shape[:-1]) + (shape[-1] + 4,), PAD).cuda()
    buf[..., :shape[-1]] = t.cuda()
    return buf[..., :shape[-1]]


@pytest.mark.parametrize("strided", [False, True], ids=["dense", "strided"])
@pytest.mark.parametrize("B,h,w,Cx,Cs", [(1, 1, 1, 4, 4), (2, 5, 7, 8, 4), (1, 3, 2, 128, 64), (2, 1, 6, 4, 8)])
def test_upcat2x_fwd_is_the_resize_and_the_copy(B, h, w, Cx, Cs, strided):
    _need_gpu()
    from miccai2021_cataract_semantic_segmentation_amd import ops
    x = _rand((B, h, w, Cx), 1 + Cx, strided)
    skip = _rand((B, 2 * h, 2 * w, Cs), 2 + Cs, strided)
    ref = torch.full((B, 2 * h, 2 * w, Cx + Cs), 3.0, device="cuda")
    ops.bilinear_fwd(x, 2 * h, 2 * w, True, out=ref[..., :Cx])
    ops.axpy(skip, ref[..., Cx:], 1.0, False)
    cat = ops.upcat2x_fwd(x, skip)
    assert torch.equal(cat, ref)
    assert _record_bits(ops.amax_of(cat)) == _amax_bits(ref)
    assert ops.amax_of(ops.upcat2x_fwd(x, skip, record=False)) is None


@pytest.mark.parametrize("shape", [(2, 8, 10, 12), (1, 20, 7, 9), (3, 4, 2, 2)])
def test_maxpool2x2_fwd_rec_is_the_pool(shape):
    """the shapes of test_maxpool2x2_bit_exact (NCHW there) with ReLU-zero ties; odd sizes: the input's record covers the row and column
    the pool leaves out"""
    _need_gpu()
    from miccai2021_cataract_semantic_segmentation_amd import ops
    B, C, H, W = shape
    for strided in (False, True):
        x = _rand((B, H, W, C), H * W, strided, relu=True)
        if H % 2 and W % 2:
            x[0, H - 1, W - 1, 1] = -9.0        # the largest magnitude sits in the corner no window covers, and is negative
        y0, i0 = ops.maxpool2_fwd(x)
        y, idx = ops.maxpool2_fwd_rec(x)
        assert torch.equal(y, y0) and torch.equal(idx, i0)
        assert _record_bits(ops.amax_of(x)) == _amax_bits(x)
        assert _record_bits(ops.amax_of(y)) == _amax_bits(y0)


def test_relu_bwd_rec_plain_and_junction():
    _need_gpu()
    from miccai2021_cataract_semantic_segmentation_amd import ops
    # plain form: dense and strided operands, more than one block
    for strided in (False, True):
        z = _rand((2, 9, 11, 12), 5, strided, relu=True)
        dz = _rand((2, 9, 11, 12), 6, strided)
        g = ops.relu_bwd_rec(dz, z)
        assert torch.equal(g, ops.relu_bwd(dz, z))
        assert _record_bits(ops.amax_of(g)) == _amax_bits(g)
    # junction form: the gradient slice sits at channel offset 8 of a 24-channel buffer, pooled sizes 5 x 7 from even and from odd maps
    for H, W in ((10, 14), (11, 15)):
        B, C = 2, 8
        z = _rand((B, H, W, C), H, relu=True)
        _, idx = ops.maxpool2_fwd(z)
        dcat = _rand((B, H, W, 24), W)
        dcat[..., :8] = PAD
        dcat[..., 16:] = PAD
        dslice = dcat[..., 8:16]
        dpool = _rand((B, 5, 7, C), H + W, strided=True)
        d = torch.empty((B, H, W, C), device="cuda")
        ops.axpy(dslice, d, 1.0, False)
        ops.maxpool2_bwd(dpool, idx, d, accumulate=True)
        ref = ops.relu_bwd(d, z)
        g = ops.relu_bwd_rec(dslice, z, pool=(dpool, idx))
        assert torch.equal(g, ref)
        assert _record_bits(ops.amax_of(g)) == _amax_bits(ref)
        assert float(ref.abs().max()) < 100.0


@pytest.mark.parametrize("rows", [1, 257, 70001])
def test_amax_record_bounds_exactly_the_valid_columns(rows):
    _need_gpu()
    from miccai2021_cataract_semantic_segmentation_amd import ops
    C = 12
    zero = torch.zeros((1, 1, rows, C), device="cuda")
    assert _record_bits(ops.amax_of(ops.amax_record(zero))) == 0
    for strided in (False, True):
        x = _rand((1, 1, rows, C), rows, strided)
        x[0, 0, rows - 1, C - 1] = -77.5        # the largest magnitude is negative and sits in the last valid element
        assert _record_bits(ops.amax_of(ops.amax_record(x))) == _amax_bits(x) == _amax_bits(torch.tensor(77.5))
    # the other producers on the same row counts: an all-zero tensor, a negative maximum, pad columns
    z = _rand((1, 1, rows, C), rows + 1, strided=True, relu=True)
    dz = _rand((1, 1, rows, C), rows + 2, strided=True)
    dz[0, 0, 0, 0], z[0, 0, 0, 0] = -123.0, 1.0
    g = ops.relu_bwd_rec(dz, z)
    assert _record_bits(ops.amax_of(g)) == _amax_bits(g) == _amax_bits(torch.tensor(123.0))
    assert _record_bits(ops.amax_of(ops.relu_bwd_rec(dz, torch.zeros_like(z)))) == 0


def test_a_width_that_is_no_multiple_of_4_is_refused():
    _need_gpu()
    from miccai2021_cataract_semantic_segmentation_amd import _lib, ops
    lib, ptr = _lib.lib, _lib.ptr
    x = torch.randn(1, 4, 4, 8, device="cuda")[..., :6]
    out = torch.full((1, 4, 4, 16), 5.0, device="cuda")
    idx = torch.full((1, 2, 2, 8), 9, dtype=torch.uint8, device="cuda")
    rec = ops.new_amax(x.device)
    assert lib.catseg_amax_record(ptr(x), 8, 16, 6, ptr(rec), None) == 1
    assert lib.catseg_maxpool2x2_fwd_rec(ptr(x), 8, ptr(out), 16, ptr(idx), 1, 4, 4, 6, ptr(rec), ptr(rec), None) == 1
    assert lib.catseg_upcat2x_fwd(ptr(x), 8, ptr(x), 8, ptr(out), 16, 1, 2, 2, 6, 6, ptr(rec), None) == 1
    assert lib.catseg_upcat2x_fwd(ptr(x), 8, ptr(x), 8, ptr(out), 16, 1, 2, 2, 4, 6, ptr(rec), None) == 1
    assert lib.catseg_relu_bwd_rec(ptr(x), 8, None, 0, None, ptr(x), 8, ptr(out), 16, 1, 4, 4, 6, ptr(rec), None) == 1
    assert b"multiples of 4" in lib.catseg_last_error()
    torch.cuda.synchronize()
    assert bool((out == 5.0).all()) and bool((idx == 9).all()) and _record_bits(rec) == 0
