"""Cases, operands and references for catseg_gemm_batched (csrc/igemm.hip) and its two callers engine.spatial_gather /
engine.object_attention_core; importable without a GPU.  tests/test_gemm_cpu.py holds this file to its own preconditions,
tests/test_gemm_gpu.py holds the kernels to it.

The operands are INTEGERS stored as float32 with K * max|a| * max|b| < 2^23: every product and every partial sum, in any order, on any
tile, with or without a K split, is an integer below 2^24 and therefore exact in fp32 -- the GPU result has to equal the float64 product
bit for bit and the comparison needs no tolerance.  In the short reductions max|a| = 4099 (odd, > 2^12): an fp16 (11-bit), tf32 (11-bit)
or bf16 (8-bit significand) path cannot even hold the operands.

The buffers follow the operand contract written at catseg_gemm_batched in include/catseg.h: what the contract wants zero is zero, and
every float that is NOT part of a logical operand -- pad columns the kernel may read but that cannot reach C, columns it must never read,
the rows between and behind the batch items, a head in front of the first -- is NaN, so that a read which reaches the result shows.  C
starts as NaNs with one payload per element: 'bit-unchanged' is then a statement about every single float."""
import collections

import torch

Case = collections.namedtuple("Case", "batch M N K lda ldb ldc zero_to")

NT, NN, TN = "NT", "NN", "TN"
LAYOUTS = (NT, NN, TN)

# (batch, M, N, K, lda, ldb, ldc, zero_to).  M crosses one row past the 64-, 128- and 256-row tiles and the 48-row form (1, 63 / 64 / 65,
# 257, 300, 513); N sits inside / across the 16-, 32-, 48-, 64- and 128-wide tiles (1, 8, 17, 25, 36, 40, 49, 100, 256) with N % 4 != 0 and
# ldc = 28 / 32 / 64, zero_to = 0 and = ldc.  The last case of NT and NN has the bench shape's 32 640 pixel rows: only a grid of more than
# 256 tiles makes the planner leave the 64 x 64 tile (NT: the 32-wide class form 4; NN: the 48-wide form 1), everything below that is
# planned onto 64 x 64 or, for N <= 16, the 16-wide form 3.
CASES = {
    # A [M][lda], B [N][ldb]; K a multiple of 4: 4, 36, 64, 256
    NT: [Case(1, 1, 1, 4, 4, 4, 4, 0),
         Case(2, 63, 8, 36, 40, 36, 28, 28),
         Case(1, 64, 64, 64, 64, 64, 64, 0),            # one whole 64 x 64 tile: the unpredicated epilogue
         Case(3, 65, 17, 4, 8, 4, 32, 0),
         Case(2, 257, 25, 256, 256, 256, 32, 32),       # the OCR similarity / dprobs launch in miniature
         Case(2, 300, 25, 256, 260, 256, 28, 0),
         Case(1, 300, 36, 36, 36, 40, 64, 64),
         Case(2, 513, 40, 64, 64, 68, 64, 0),
         Case(1, 65, 49, 36, 36, 36, 64, 64),
         Case(1, 130, 100, 64, 64, 64, 100, 0),
         Case(1, 128, 256, 36, 36, 36, 256, 0),         # whole tiles only, four of them across N
         Case(1, 513, 256, 4, 4, 4, 260, 260),
         Case(1, 32640, 25, 4, 4, 4, 32, 32)],
    # A [M][lda] with K <= lda = 32 / 64: 17, 25, 40; B [K][ldb]
    NN: [Case(1, 1, 1, 17, 32, 4, 4, 0),
         Case(2, 63, 8, 25, 32, 8, 28, 28),
         Case(1, 64, 64, 40, 64, 64, 64, 0),
         Case(3, 65, 17, 25, 32, 20, 32, 0),
         Case(2, 257, 25, 17, 32, 28, 32, 32),
         Case(2, 300, 36, 40, 64, 36, 64, 64),
         Case(2, 513, 40, 25, 32, 44, 64, 0),
         Case(1, 65, 49, 17, 32, 52, 64, 64),
         Case(1, 130, 100, 40, 64, 100, 100, 0),
         Case(2, 300, 256, 25, 32, 256, 256, 0),        # the OCR context / dq launch in miniature
         Case(1, 128, 256, 40, 64, 256, 256, 0),
         Case(1, 32640, 36, 25, 32, 36, 36, 0)],
    # A [K][lda], B [K][ldb]; K is the row count: 1, 15, 16, 17 around the 16-row K step, 1000, 4100 past tn_splits' threshold
    TN: [Case(1, 1, 1, 1, 4, 4, 4, 0),
         Case(2, 25, 64, 15, 32, 64, 64, 0),
         Case(3, 17, 8, 16, 32, 8, 28, 28),
         Case(2, 25, 256, 17, 32, 256, 256, 0),         # the OCR proxy / dv / dk launch in miniature
         Case(1, 63, 17, 1000, 64, 20, 32, 0),
         Case(1, 64, 64, 17, 64, 64, 64, 0),
         Case(2, 65, 25, 15, 68, 28, 32, 32),
         Case(1, 257, 36, 16, 260, 36, 64, 64),
         Case(1, 300, 49, 17, 300, 52, 64, 0),
         Case(1, 513, 40, 1, 516, 40, 64, 64),
         Case(2, 40, 100, 4100, 64, 100, 100, 0),
         Case(1, 25, 256, 4100, 32, 256, 256, 0)],
}

HEAD = 8            # NaN floats in front of the first batch item (a multiple of 4: the operand stays 16-byte aligned)
LIMIT = 2 ** 23     # K max|a| max|b| stays below this; with |C0| <= C0_MAX the accumulated result stays below 2^24
C0_MAX = 1000


def roundup4(n):
    return (n + 3) // 4 * 4


def case_id(case):
    return "b%d_m%d_n%d_k%d_ld%d_%d_%d_z%d" % tuple(case)


def geometry(layout, case):
    """(rows, logical columns, ld, columns that must be ZERO) of A and of B"""
    _, M, N, K, lda, ldb, _, _ = case
    if layout == NT:
        return (M, K, lda, (K, K)), (N, K, ldb, (K, K))
    if layout == NN:
        return (M, K, lda, (K, roundup4(K))), (K, N, ldb, (N, N))
    return (K, M, lda, (M, M)), (K, N, ldb, (N, N))


def magnitudes(K):
    """(max|a|, max|b|) with K max|a| max|b| < LIMIT; max|a| = 4099 in the short reductions"""
    if K <= 256:
        amax = 4099
        bmax = (LIMIT - 1) // (K * amax)
    else:
        amax = bmax = int(((LIMIT - 1) // K) ** 0.5)
    assert bmax >= 1 and K * amax * bmax < LIMIT
    return amax, bmax


def batch_stride(rows, ld):
    """floats from one batch item to the next: the dense item, four more rows and 12 floats -- each operand is a slice of a wider buffer,
    and a reduction that ran on into the rows behind an item (up to the next multiple of 4) would meet NaNs there, inside the buffer"""
    return rows * ld + 4 * ld + 12


def nan_pattern(n, salt=0):
    """n quiet NaNs as float32, every one with its own payload"""
    bits = (torch.arange(n, dtype=torch.int64) * 2654435761 + salt) % (1 << 22)
    return (bits + 0x7FC00000).to(torch.int32).view(torch.float32)


def bits(t):
    return t.contiguous().view(torch.int32)


def strided(flat, batch, rows, ld):
    """[batch][rows][ld] view of a flat buffer built by operand() / c_buffer()"""
    return torch.as_strided(flat, (batch, rows, ld), (batch_stride(rows, ld), ld, 1), HEAD)


def operand(batch, rows, cols, ld, zero, maxabs, gen):
    """flat NaN buffer holding `batch` items of [rows][ld]: integers of |.| <= maxabs (the bound is attained) in columns [0, cols), zeros in
    columns [zero[0], zero[1]).  Returns (flat, logical values [batch, rows, cols])."""
    flat = nan_pattern(HEAD + batch * batch_stride(rows, ld) + HEAD)
    vals = torch.randint(-maxabs, maxabs + 1, (batch, rows, cols), generator=gen).float()
    vals[0, 0, 0] = maxabs
    vals[-1, -1, -1] = -maxabs
    view = strided(flat, batch, rows, ld)
    view[..., :cols] = vals
    view[..., zero[0]:zero[1]] = 0.0
    return flat, vals


Operands = collections.namedtuple("Operands", "layout case A B a b ref sA sB amax bmax")


def operands(layout, case, seed=0):
    """the two flat operand buffers, their logical values (a, b), the float64 product [batch, M, N] and the batch strides"""
    batch, M, N, K = case[:4]
    (ra, ca, lda, za), (rb, cb, ldb, zb) = geometry(layout, case)
    amax, bmax = magnitudes(K)
    gen = torch.Generator().manual_seed(1000 * LAYOUTS.index(layout) + seed + M + 7 * N + 13 * K)
    A, a = operand(batch, ra, ca, lda, za, amax, gen)
    B, b = operand(batch, rb, cb, ldb, zb, bmax, gen)
    ref = product(layout, a.double(), b.double())
    return Operands(layout, case, A, B, a, b, ref, batch_stride(ra, lda), batch_stride(rb, ldb), amax, bmax)


def product(layout, a, b):
    if layout == NT:
        return a @ b.transpose(1, 2)
    if layout == NN:
        return a @ b
    return a.transpose(1, 2) @ b


def c_buffer(case, accumulate, seed=0):
    """flat C: NaNs of distinct payloads everywhere; for an accumulating launch integers of |.| <= C0_MAX in the logical [M][N] block (the
    columns [N, zero_to) stay NaN: the kernel has to write its zeros over them in either mode)"""
    batch, M, N = case[:3]
    ldc = case.ldc
    flat = nan_pattern(HEAD + batch * batch_stride(M, ldc) + HEAD, salt=77)
    if accumulate:
        gen = torch.Generator().manual_seed(seed + 31 * M + N)
        strided(flat, batch, M, ldc)[..., :N] = torch.randint(-C0_MAX, C0_MAX + 1, (batch, M, N), generator=gen).float()
    return flat


def check_c(case, before, after, ref, accumulate, what=""):
    """the statements of the contract about C, on the CPU: `before` / `after` are the flat buffer around one launch"""
    batch, M, N = case[:3]
    ldc, zero_to = case.ldc, case.zero_to
    got, old = strided(after, batch, M, ldc), strided(before, batch, M, ldc)
    want = ref + old[..., :N].double() if accumulate else ref
    assert want.abs().max() < 2 ** 24
    logical = got[..., :N]
    assert not torch.isnan(logical).any(), "%s: NaN in the logical result (a pad or a gap reached C)" % what
    assert torch.equal(logical, want.float()) and torch.equal(logical.double(), want), \
        "%s: %d of %d elements differ from the float64 product, max |diff| %g" % (
            what, int((logical.double() != want).sum()), want.numel(), float((logical.double() - want).abs().max()))
    if zero_to > N:
        assert torch.equal(bits(got[..., N:zero_to]), torch.zeros_like(bits(got[..., N:zero_to]))), "%s: columns [N, zero_to) are not +0" % what
    touched = torch.zeros(after.numel(), dtype=torch.bool)
    strided(touched, batch, M, ldc)[..., :max(N, zero_to)] = True
    same = bits(after) == bits(before)
    assert bool(same[~touched].all()), "%s: %d floats outside the written columns changed" % (what, int((~same[~touched]).sum()))


# ---------------------------------------------------------------------------------------------------------------------------------
# The two modules that call the GEMMs, restated from their formulas in plain torch (any dtype, autograd): pixels flattened to N = H * W.

def spatial_gather(feats, logits):
    """models/OCR.py:158-170: feats [B, N, C], logits [B, N, K] -> [B, K, C]; softmax over the PIXELS of each class, times the features"""
    probs = torch.softmax(logits, dim=1)
    return probs.transpose(1, 2) @ feats


def object_attention(q, key, val, key_channels):
    """models/OCR.py:266-274: q [B, N, Ck], key / val [B, K, Ck] -> [B, N, Ck]; softmax over the classes of Ck^-0.5 q key^T, times val"""
    sim = torch.softmax((float(key_channels) ** -0.5) * (q @ key.transpose(1, 2)), dim=-1)
    return sim @ val


def with_grads(fn, inputs, dout, dtype):
    """(output, [gradient of every input]) of fn(*inputs) under the cotangent dout, computed in dtype"""
    xs = [x.detach().to(dtype).requires_grad_() for x in inputs]
    out = fn(*xs)
    out.backward(dout.to(dtype))
    return out.detach(), [x.grad for x in xs]
