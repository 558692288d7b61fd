"""tests/_gemm_ref.py against its own preconditions, without a GPU: the integer operands really make fp32 exact, the magnitudes are what the
docstring says, every float outside the logical operands is NaN except the pads the contract wants zero, and the checker that the GPU
tests rely on accepts a product written by the rules of the contract and rejects the mistakes it is there to find."""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _gemm_ref as GR  # noqa: E402

ALL = [(lay, c) for lay in GR.LAYOUTS for c in GR.CASES[lay]]
IDS = ["%s-%s" % (lay, GR.case_id(c)) for lay, c in ALL]


def test_case_list_covers_the_boundaries():
    assert sum(len(v) for v in GR.CASES.values()) <= 40
    for lay in GR.LAYOUTS:
        cs = GR.CASES[lay]
        m = {c.K if lay == GR.TN else c.M for c in cs}        # (TN: the long side is the reduction; its M is the class count)
        if lay != GR.TN:
            assert {1, 63, 64, 65, 257, 300, 513} <= m
        else:
            assert {1, 15, 16, 17, 1000, 4100} <= m and {63, 64, 65, 257, 300, 513} <= {c.M for c in cs}
        assert {1, 8, 17, 25, 36, 40, 49, 100, 256} <= {c.N for c in cs}
        assert {28, 32, 64} <= {c.ldc for c in cs}
        assert any(c.zero_to == 0 for c in cs) and any(c.zero_to == c.ldc and c.ldc > c.N for c in cs)
        assert {1, 2, 3} <= {c.batch for c in cs}
        assert any(c.N == 25 and c.ldc == 32 and c.zero_to == 32 for c in cs)
    assert {4, 36, 64, 256} <= {c.K for c in GR.CASES[GR.NT]} and all(c.K % 4 == 0 for c in GR.CASES[GR.NT])
    assert {17, 25, 40} <= {c.K for c in GR.CASES[GR.NN]} and {32, 64} == {c.lda for c in GR.CASES[GR.NN]}
    for lay, c in ALL:                                         # what catseg_gemm_batched requires of a launch
        (ra, ca, lda, _), (rb, cb, ldb, _) = GR.geometry(lay, c)
        assert lda % 4 == 0 and ldb % 4 == 0 and lda >= GR.roundup4(ca) and ldb >= GR.roundup4(cb)
        assert c.ldc >= c.N and c.zero_to <= c.ldc
        assert GR.batch_stride(ra, lda) % 4 == 0 and GR.batch_stride(rb, ldb) % 4 == 0
        assert max(GR.batch_stride(ra, lda) * c.batch, GR.batch_stride(rb, ldb) * c.batch, GR.batch_stride(c.M, c.ldc) * c.batch) * 4 < 8 << 20


@pytest.mark.parametrize("layout,case", ALL, ids=IDS)
def test_operands_are_exact_in_fp32(layout, case):
    op = GR.operands(layout, case)
    K = case.K
    assert float(op.a.abs().max()) == op.amax and float(op.b.abs().max()) == op.bmax
    assert K * op.amax * op.bmax < 2 ** 23 < 2 ** 24
    if K <= 256:
        assert op.amax >= 2 ** 12 and op.amax % 2 == 1         # not an fp16 / tf32 / bf16 number
        assert float(op.a.half().float().sub(op.a).abs().max()) > 0 and float(op.a.bfloat16().float().sub(op.a).abs().max()) > 0
    assert torch.equal(op.a, op.a.round()) and torch.equal(op.b, op.b.round())
    p32 = GR.product(layout, op.a, op.b)
    assert p32.dtype == torch.float32 and op.ref.dtype == torch.float64
    assert torch.equal(p32, op.ref.float()) and torch.equal(p32.double(), op.ref)
    assert float(op.ref.abs().max()) + GR.C0_MAX < 2 ** 24
    # another summation order (a reversed reduction, two halves added) gives the same bits: the property the GPU test stands on
    h = max(K // 2, 1)
    if layout == GR.TN:
        parts = GR.product(layout, op.a[:, h:], op.b[:, h:]) + GR.product(layout, op.a[:, :h].flip(1), op.b[:, :h].flip(1))
    elif layout == GR.NN:
        parts = GR.product(layout, op.a[..., h:], op.b[:, h:]) + GR.product(layout, op.a[..., :h].flip(2), op.b[:, :h].flip(1))
    else:
        parts = GR.product(layout, op.a[..., h:], op.b[..., h:]) + GR.product(layout, op.a[..., :h].flip(2), op.b[..., :h].flip(2))
    assert torch.equal(parts, p32)


@pytest.mark.parametrize("layout,case", ALL, ids=IDS)
def test_buffers_are_nan_outside_the_operands(layout, case):
    op = GR.operands(layout, case)
    for flat, vals, (rows, cols, ld, zero) in zip((op.A, op.B), (op.a, op.b), GR.geometry(layout, case)):
        assert flat.numel() == 2 * GR.HEAD + case.batch * GR.batch_stride(rows, ld) and GR.batch_stride(rows, ld) > rows * ld
        view = GR.strided(flat, case.batch, rows, ld)
        assert torch.equal(view[..., :cols], vals)
        assert zero[0] == cols and torch.equal(view[..., cols:zero[1]], torch.zeros(case.batch, rows, zero[1] - cols))
        known = torch.zeros(flat.numel(), dtype=torch.bool)
        GR.strided(known, case.batch, rows, ld)[..., :zero[1]] = True
        assert bool(torch.isfinite(flat[known]).all()) and bool(torch.isnan(flat[~known]).all())
        assert int((~known).sum()) >= 2 * GR.HEAD + case.batch * (ld + 12)            # head, tail and the gap behind every item
    if layout == GR.NN:                                       # the only pad the contract wants zero: A's columns [K, roundup4(K))
        assert GR.geometry(layout, case)[0][3] == (case.K, GR.roundup4(case.K))
    for acc in (False, True):
        c = GR.c_buffer(case, acc)
        logical = GR.strided(c, case.batch, case.M, case.ldc)[..., :case.N]
        assert bool(torch.isfinite(logical).all()) == acc and int(torch.isnan(c).sum()) == c.numel() - (logical.numel() if acc else 0)
        if not acc:
            assert c.numel() < 1 << 22 and GR.bits(c).unique().numel() == c.numel()          # one payload per NaN


def _emulate(layout, case, before, op, accumulate):
    """a launch that keeps the contract, in torch on the CPU"""
    after = before.clone()
    c = GR.strided(after, case.batch, case.M, case.ldc)
    p = GR.product(layout, op.a, op.b)
    c[..., :case.N] = c[..., :case.N] + p if accumulate else p
    c[..., case.N:case.zero_to] = 0.0
    return after


@pytest.mark.parametrize("layout", GR.LAYOUTS)
def test_checker_accepts_the_contract_and_rejects_its_breaches(layout):
    case = next(c for c in GR.CASES[layout] if c.N == 25 and c.zero_to == 32 and c.batch > 1)
    op = GR.operands(layout, case)
    for acc in (False, True):
        before = GR.c_buffer(case, acc)
        good = _emulate(layout, case, before, op, acc)
        GR.check_c(case, before, good, op.ref, acc)

        def breach(edit):
            bad = good.clone()
            edit(GR.strided(bad, case.batch, case.M, case.ldc), bad)
            with pytest.raises(AssertionError):
                GR.check_c(case, before, bad, op.ref, acc)

        breach(lambda c, flat: c[-1, -1, 24].add_(1.0))                              # one unit in the last logical element
        breach(lambda c, flat: c[0, 3, 7].fill_(float("nan")))                       # a NaN that reached the result
        breach(lambda c, flat: c[1, 0, 25].fill_(-0.0))                              # a zero_to column that is not +0
        breach(lambda c, flat: flat[GR.HEAD + GR.batch_stride(case.M, case.ldc) - 1].fill_(0.0))   # a write into the gap between two items
        breach(lambda c, flat: flat[0].fill_(0.0))                                   # ... in front of the first
        if acc:                                                                      # an accumulating launch that overwrote
            breach(lambda c, flat: c[..., :25].copy_(GR.product(layout, op.a, op.b)))
        else:                                                                        # a plain launch that added to the NaNs / another batch item's block
            breach(lambda c, flat: c[0, :, :25].copy_(c[1, :, :25]))


def test_restatements_match_the_oracle():
    """the two plain-torch modules against the project's CPU oracle of the same reference lines (oracle/nets.py, NCHW)"""
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    from oracle import nets as ON
    g = torch.Generator().manual_seed(3)
    B, H, W, C, K = 2, 3, 5, 8, 6
    feats, logits = torch.randn(B, C, H, W, generator=g).double(), torch.randn(B, K, H, W, generator=g).double()
    want = ON.spatial_gather(feats, logits)[..., 0].transpose(1, 2)                  # B, C, K, 1 -> B, K, C
    got = GR.spatial_gather(feats.flatten(2).transpose(1, 2), logits.flatten(2).transpose(1, 2))
    assert torch.allclose(got, want, rtol=0, atol=1e-14)
    q, key, val = (torch.randn(B, n, C, generator=g).double() for n in (H * W, K, K))
    sim = torch.softmax(C ** -0.5 * torch.matmul(q, key.transpose(1, 2)), dim=-1)    # models/OCR.py:266-274 line by line
    assert torch.allclose(GR.object_attention(q, key, val, C), torch.matmul(sim, val), rtol=0, atol=1e-14)
    out, grads = GR.with_grads(GR.spatial_gather, (feats.flatten(2).transpose(1, 2), logits.flatten(2).transpose(1, 2)), torch.ones_like(got),
                               torch.float32)
    assert out.dtype == torch.float32 and all(x.dtype == torch.float32 for x in grads)
