"""catseg_gemm_batched (csrc/igemm.hip) and its two callers, engine.spatial_gather and engine.object_attention_core.

The batched GEMM is compared WITHOUT a tolerance: tests/_gemm_ref.py builds integer operands whose products and partial sums are exact in
fp32 in any order, so the result equals the float64 product bit for bit on every tile form, and it lays the buffers out by the operand
contract at catseg_gemm_batched in include/catseg.h (NaN wherever the contract promises that nothing is read into the result; a NaN payload
of its own in every float of C the launch must leave alone).  test_exact_* runs every case through the planner's choice, test_forms_*
forces every tile form the dispatcher instantiates for the layout, test_tn_split runs the K-split reduction both ways, test_refusals the
argument checks.

The two engine functions are driven by an engine.Ctx in record mode exactly as models/OCR.py drives them (no network around them) and held
to the float64 restatement of the reference's lines with tests/_yardstick.within: at most 4 x the error of the same lines in float32 on the
CPU.  Worst RATIO (kernel error / yardstick) per function over all cases, forward and every input gradient, fresh and accumulating
destinations, measured on an MI355X:
    spatial_gather          2.006  (50 x 82, K 17, C 256: forward)
    object_attention_core   2.219  (50 x 82, K 17, Ck 256: gradient of val)"""
import os
import re
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _gemm_ref as GR  # noqa: E402
from _yardstick import within  # noqa: E402

pytestmark = pytest.mark.gpu

EINVAL = 1


def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")


def _ops():
    from miccai2021_cataract_semantic_segmentation_amd import ops
    return ops


_DEVICE_OPERANDS = {}


def _operands(layout, case):
    """operands of a case, built once and left unchanged: (Operands, A and B on the GPU from their first logical float on)"""
    key = (layout, case)
    if key not in _DEVICE_OPERANDS:
        op = GR.operands(layout, case)
        _DEVICE_OPERANDS[key] = (op, op.A.cuda()[GR.HEAD:], op.B.cuda()[GR.HEAD:])
    return _DEVICE_OPERANDS[key]


def _launch(ops, layout, case, Ad, sA, Bd, sB, flat_c, accumulate):
    code = {GR.NT: ops.NT, GR.NN: ops.NN, GR.TN: ops.TN}[layout]
    batch, M, N, K, lda, ldb, ldc, zero_to = case
    ops.gemm(code, batch, M, N, K, Ad, lda, sA, Bd, ldb, sB, flat_c[GR.HEAD:], ldc, GR.batch_stride(M, ldc), zero_to=zero_to,
             accumulate=accumulate)


def _exact(ops, layout, case, what):
    """a plain launch into NaNs, then an accumulating one onto integers: the statements of the contract about C (GR.check_c)"""
    op, Ad, Bd = _operands(layout, case)
    for accumulate in (False, True):
        before = GR.c_buffer(case, accumulate)
        cd = before.cuda()
        _launch(ops, layout, case, Ad, op.sA, Bd, op.sB, cd, accumulate)
        GR.check_c(case, before, cd.cpu(), op.ref, accumulate, "%s %s %s%s" % (layout, GR.case_id(case), what, " accumulate" if accumulate else ""))


ALL = [(lay, c) for lay in GR.LAYOUTS for c in GR.CASES[lay]]


@pytest.mark.parametrize("layout,case", ALL, ids=["%s-%s" % (lay, GR.case_id(c)) for lay, c in ALL])
def test_exact_planned(layout, case):
    """(a) every case on the tile the planner picks"""
    _need_gpu()
    _exact(_ops(), layout, case, "planned")


# the (form, mi, ni) that CS_FORM instantiates in launch_igemm (csrc/igemm.hip), per layout: form 0 = (64 mi) x (64 ni) tiles, 1 = 48 ni wide,
# 2 = 48 mi high, 3 / 4 = 16 / 32 wide
_SQUARE = [(0, 1, 1), (0, 1, 2), (0, 2, 1), (0, 2, 2), (0, 4, 2), (0, 2, 4)]
_WIDE48 = [(1, 2, 1), (1, 4, 1), (1, 2, 2), (1, 4, 2)]
FORMS = {GR.NT: _SQUARE + _WIDE48 + [(3, 2, 1), (3, 4, 1), (4, 2, 1), (4, 4, 1)],
         GR.NN: _SQUARE + _WIDE48,
         GR.TN: _SQUARE + [(2, 1, 2), (2, 1, 4), (2, 2, 2), (2, 2, 4)]}
# ... and tiles that it does not: a form of another layout, a shape no layout has
NO_FORMS = {GR.NT: [(2, 1, 2), (0, 4, 1), (3, 1, 1)], GR.NN: [(3, 2, 1), (4, 4, 1), (2, 2, 2), (0, 4, 4)], GR.TN: [(1, 2, 1), (3, 2, 1), (4, 2, 1), (0, 1, 4)]}


def _tile(form, mi, ni):
    return (48 if form == 2 else 64) * mi, {1: 48 * ni, 3: 16, 4: 32}.get(form, 64 * ni)


def _form_cases(layout, form, mi, ni):
    """one case inside the tile, one a row and a column past it, and the OCR launch of the layout in miniature (N = 25, ldc = zero_to = 32)"""
    tm, tn = _tile(form, mi, ni)
    r4 = GR.roundup4
    if layout == GR.NT:
        return [GR.Case(1, tm - 7, min(tn, 16) - 3, 36, 36, 36, r4(tn), 0), GR.Case(2, tm + 1, tn + 1, 64, 68, 64, r4(tn + 1) + 4, r4(tn + 1) + 4),
                GR.Case(2, 300, 25, 256, 256, 256, 32, 32)]
    if layout == GR.NN:
        return [GR.Case(1, tm - 7, min(tn, 16) - 3, 17, 32, 16, r4(tn), 0), GR.Case(2, tm + 1, tn + 1, 40, 64, r4(tn + 1), r4(tn + 1) + 4, r4(tn + 1) + 4),
                GR.Case(2, 300, 25, 25, 32, 28, 32, 32)]
    return [GR.Case(1, tm - 7, min(tn, 16) - 3, 15, r4(tm), 16, r4(tn), 0), GR.Case(2, tm + 1, tn + 1, 17, r4(tm + 1), r4(tn + 1), r4(tn + 1) + 4, r4(tn + 1) + 4),
            GR.Case(2, 25, 256, 40, 32, 256, 256, 0), GR.Case(2, 300, 25, 33, 300, 28, 32, 32)]


def _forced(ops, form, mi, ni, fn):
    ops.lib.catseg_debug_set_tile(mi + 16 * form, ni)
    try:
        return fn()
    finally:
        ops.lib.catseg_debug_set_tile(0, 0)


@pytest.mark.parametrize("layout,form,mi,ni", [(lay, f, mi, ni) for lay in GR.LAYOUTS for f, mi, ni in FORMS[lay]])
def test_forms_exact(layout, form, mi, ni):
    """(b) the same equalities on every tile form of the layout, forced through catseg_debug_set_tile"""
    _need_gpu()
    ops = _ops()
    for case in _form_cases(layout, form, mi, ni):
        _forced(ops, form, mi, ni, lambda: _exact(ops, layout, case, "form %d tile %d x %d" % (form, mi, ni)))


@pytest.mark.parametrize("layout,form,mi,ni", [(lay, f, mi, ni) for lay in GR.LAYOUTS for f, mi, ni in NO_FORMS[lay]])
def test_forms_missing_are_refused(layout, form, mi, ni):
    """a tile form the layout does not have: CATSEG_EINVAL with a message, no launch, C untouched"""
    _need_gpu()
    ops = _ops()
    case = _form_cases(layout, 0, 1, 1)[1]
    op, Ad, Bd = _operands(layout, case)
    before = GR.c_buffer(case, False)
    cd = before.cuda()
    with pytest.raises(RuntimeError, match=r"error %d: .*unsupported tile" % EINVAL):
        _forced(ops, form, mi, ni, lambda: _launch(ops, layout, case, Ad, op.sA, Bd, op.sB, cd, False))
    torch.cuda.synchronize()
    assert torch.equal(GR.bits(cd.cpu()), GR.bits(before))
    _exact(ops, layout, case, "after the refusal")          # (and the forced tile is gone again)


@pytest.mark.parametrize("K,M,N", [(4100, 25, 64), (4100, 17, 256), (8160, 25, 256), (8160, 17, 64)])
def test_tn_split(K, M, N):
    """(c) ops.gemm_tn_split with the K split on and off, fresh and accumulating: exact both ways, so equal to each other"""
    _need_gpu()
    ops = _ops()
    batch, lda = 2, 32
    assert ops.tn_splits(M, N, K) > 1
    amax, bmax = GR.magnitudes(K)
    gen = torch.Generator().manual_seed(K + M + N)
    A = GR.nan_pattern(batch * K * lda).view(batch, K, lda).clone()         # [batch, K, ld] contiguous is what gemm_tn_split takes: no gaps
    a = torch.randint(-amax, amax + 1, (batch, K, M), generator=gen).float()
    b = torch.randint(-bmax, bmax + 1, (batch, K, N), generator=gen).float()
    A[..., :M] = a
    ref = GR.product(GR.TN, a.double(), b.double())
    assert torch.equal(GR.product(GR.TN, a, b), ref.float())
    c0 = torch.randint(-GR.C0_MAX, GR.C0_MAX + 1, (batch, M, N), generator=gen).float()
    Ad, Bd = A.cuda(), b.cuda()
    got = {}
    saved = ops.GEMM_TN_SPLIT
    try:
        for split in (True, False):
            ops.GEMM_TN_SPLIT = split
            fresh = torch.full((batch, M, N), float("nan"), device="cuda")
            ops.gemm_tn_split(batch, M, N, K, Ad, lda, Bd, N, fresh)
            acc = c0.cuda()
            ops.gemm_tn_split(batch, M, N, K, Ad, lda, Bd, N, acc, accumulate=True)
            got[split] = (fresh.cpu(), acc.cpu())
    finally:
        ops.GEMM_TN_SPLIT = saved
    for split in (True, False):
        assert torch.equal(got[split][0].double(), ref), "split %s" % split
        assert torch.equal(got[split][1].double(), ref + c0.double()), "split %s accumulate" % split
    assert torch.equal(got[True][0], got[False][0]) and torch.equal(got[True][1], got[False][1])


def _refusals():
    """(name, layout, a valid case, what is changed in it, which pointer is moved by one float, the message)"""
    nt, nn, tn = GR.Case(2, 65, 25, 36, 36, 36, 32, 32), GR.Case(2, 65, 25, 25, 32, 28, 32, 32), GR.Case(2, 25, 64, 17, 32, 64, 64, 0)
    return [("K % 4 != 0 in NT", GR.NT, nt, dict(K=34), None, "multiple of 4"),
            ("lda < roundup4(K) in NN", GR.NN, nn, dict(lda=24), None, "lda/ldb too small"),
            ("A off by 4 bytes", GR.NT, nt, {}, 0, "16-byte aligned"),
            ("B off by 4 bytes", GR.NN, nn, {}, 1, "16-byte aligned"),
            ("C off by 4 bytes", GR.TN, tn, {}, 2, "16-byte aligned"),
            ("zero_to > ldc", GR.NT, nt, dict(zero_to=36), None, "zero_to > ldc"),
            ("lda % 4 != 0", GR.NT, nt, dict(lda=38), None, "multiples of 4"),
            ("lda % 4 != 0 in TN", GR.TN, tn, dict(lda=30), None, "multiples of 4")]


@pytest.mark.parametrize("name,layout,valid,change,shift,message", _refusals(), ids=[r[0].replace(" ", "_") for r in _refusals()])
def test_refusals(name, layout, valid, change, shift, message):
    """(d) each bad argument returns CATSEG_EINVAL with its message and leaves a NaN-filled C untouched.  The buffers are those of the valid
    case: the refused launch -- had it run -- would have stayed inside them."""
    _need_gpu()
    ops = _ops()
    op, Ad, Bd = _operands(layout, valid)
    before = GR.c_buffer(valid, False)
    cd = before.cuda()
    bad = valid._replace(**change)
    code = {GR.NT: ops.NT, GR.NN: ops.NN, GR.TN: ops.TN}[layout]
    Ad, Bd, Cd = (t[1:] if shift == i else t for i, t in enumerate((Ad, Bd, cd[GR.HEAD:])))
    with pytest.raises(RuntimeError, match=r"error %d: .*%s" % (EINVAL, re.escape(message))):
        ops.gemm(code, bad.batch, bad.M, bad.N, bad.K, Ad, bad.lda, op.sA, Bd, bad.ldb, op.sB, Cd, bad.ldc, GR.batch_stride(valid.M, valid.ldc),
                 zero_to=bad.zero_to)
    torch.cuda.synchronize()
    assert torch.equal(GR.bits(cd.cpu()), GR.bits(before))


# ---------------------------------------------------------------------------------------------------------------------------------
# (e) the two engine functions under an engine.Ctx in record mode

def _wide(x, ld, off, fill=float("nan")):
    """[B, H, W, C] CPU tensor -> CUDA view of pixel stride ld that starts at channel `off` of a wider buffer holding `fill` elsewhere"""
    B, H, W, C = x.shape
    buf = torch.full((B, H, W, ld), fill, dtype=torch.float32, device="cuda")
    buf[..., off:off + C] = x.cuda()
    return buf[..., off:off + C] if ld != C else buf


def _run_tape(engine, fn, inputs, dout, given):
    """forward + backward of one engine function: (output, gradient of every input).  `given`: None = fresh destinations, else a gradient
    that every input already holds when the tape runs (the accumulate branches)."""
    cx = engine.Ctx(train=True, record=True)
    grads = []
    cx.push(lambda: grads.extend(cx.take(t) for t in inputs))      # recorded first, runs last: what a producing layer would do
    out = fn(cx, *inputs)
    cx.give(out, dout)
    if given is not None:
        for t, g in zip(inputs, given):
            cx.give(t, g)
    cx.backward()
    torch.cuda.synchronize()
    return out, grads


ENGINE_CASES = [(hw, K, C) for hw in ((9, 13), (50, 82)) for K in (25, 17, 40) for C in (64, 256)]
ENGINE_IDS = ["%dx%d_k%d_c%d" % (hw[0], hw[1], K, C) for hw, K, C in ENGINE_CASES]


def _hold(kernel, case, names, outs, grads, ref64, ref32, given):
    o64, g64 = ref64
    o32, g32 = ref32
    within(kernel, case + " forward", outs, o64, o32)
    for name, g, r64, r32, g0 in zip(names, grads, g64, g32, given or [None] * len(names)):
        g = g.cpu().double()
        if g0 is not None:
            g = g - g0.double()
        within(kernel, "%s d%s%s" % (case, name, " accumulate" if g0 is not None else ""), g, r64, r32)


@pytest.mark.parametrize("hw,K,C", ENGINE_CASES, ids=ENGINE_IDS)
def test_spatial_gather(hw, K, C):
    """models/OCR.py:158-170 through engine.spatial_gather: feats is the upper half of a 2 C wide concat buffer (as OCRNet passes it), the
    logits are rows of ld = 32 / 64 floats with NaN pads"""
    _need_gpu()
    from miccai2021_cataract_semantic_segmentation_amd import engine
    B, (H, W) = 2, hw
    N, ld = H * W, 32 if K <= 32 else 64
    gen = torch.Generator().manual_seed(H + K + C)
    feats, logits = torch.randn(B, H, W, C, generator=gen), 2.0 * torch.randn(B, H, W, K, generator=gen)
    dout = torch.randn(B, K, C, generator=gen)
    flat = (feats.view(B, N, C), logits.view(B, N, K))
    ref64, ref32 = GR.with_grads(GR.spatial_gather, flat, dout, torch.float64), GR.with_grads(GR.spatial_gather, flat, dout, torch.float32)
    # the gradient already there: at most half the scale of the one added to it, so that the sum rounds at the ulp of that scale
    g0 = ((torch.rand(B, H, W, C, generator=gen) - 0.5) * float(ref64[1][0].abs().max()),
          (torch.rand(B, H, W, K, generator=gen) - 0.5) * float(ref64[1][1].abs().max()))
    case = "%dx%d K%d C%d" % (H, W, K, C)
    for given in (None, g0):
        fd, ld_ = _wide(feats, 2 * C, C), _wide(logits, ld, 0)
        dev_given = None if given is None else (_wide(given[0], 2 * C, C), _wide(given[1], ld, 0, fill=0.0))
        out, grads = _run_tape(engine, lambda cx, f, l: engine.spatial_gather(cx, f, l, K), (fd, ld_), dout.view(B, K, 1, C).cuda(), dev_given)
        assert out.shape == (B, K, 1, C)
        _hold("spatial_gather", case, ("feats", "logits"), out.view(B, K, C), [g.reshape(B, N, -1) for g in grads], ref64, ref32,
              None if given is None else [g.view(B, N, -1) for g in given])
        if given is not None:                                   # the accumulating launches wrote nowhere else in the wide buffers
            assert bool(torch.isnan(dev_given[0]._base[..., :C]).all()) and float(dev_given[1]._base[..., K:].abs().max()) == 0


@pytest.mark.parametrize("hw,K,C", ENGINE_CASES, ids=ENGINE_IDS)
def test_object_attention_core(hw, K, C):
    """models/OCR.py:266-274 through engine.object_attention_core (q, key and val are dense there: the function passes Ck as their row stride)"""
    _need_gpu()
    from miccai2021_cataract_semantic_segmentation_amd import engine
    B, (H, W) = 2, hw
    N = H * W
    gen = torch.Generator().manual_seed(H + K + C + 1)
    q, key, val = torch.randn(B, H, W, C, generator=gen), torch.randn(B, K, 1, C, generator=gen), torch.randn(B, K, 1, C, generator=gen)
    dout = torch.randn(B, N, C, generator=gen)
    flat = (q.view(B, N, C), key.view(B, K, C), val.view(B, K, C))
    fn = lambda a, b, c: GR.object_attention(a, b, c, C)        # noqa: E731
    ref64, ref32 = GR.with_grads(fn, flat, dout, torch.float64), GR.with_grads(fn, flat, dout, torch.float32)
    g0 = tuple((torch.rand(t.shape, generator=gen) - 0.5) * float(r.abs().max()) for t, r in zip((q, key, val), ref64[1]))
    case = "%dx%d K%d Ck%d" % (H, W, K, C)
    for given in (None, g0):
        dev_given = None if given is None else tuple(g.cuda() for g in given)
        out, grads = _run_tape(engine, lambda cx, a, b, c: engine.object_attention_core(cx, a, b, c, K, C), (q.cuda(), key.cuda(), val.cuda()),
                               dout.view(B, H, W, C).cuda(), dev_given)
        assert out.shape == (B, H, W, C)
        _hold("object_attention_core", case, ("q", "key", "val"), out.view(B, N, C), [g.reshape(r.shape) for g, r in zip(grads, ref64[1])],
              ref64, ref32, None if given is None else [g.view(r.shape) for g, r in zip(given, ref64[1])])


@pytest.mark.parametrize("K,ld", [(25, 32), (40, 64)])
def test_class_rows_leave_the_gemm_with_zero_pads(K, ld, monkeypatch):
    """the GEMMs of the two functions that write rows of `ld` class columns (sim, dp, dprobs: torch.empty buffers) pass zero_to = ld, so the pad
    columns [K, ld) that the next kernel's 16-byte loads cover hold zeros, not whatever the allocator left: every such launch is watched"""
    _need_gpu()
    from miccai2021_cataract_semantic_segmentation_amd import engine
    ops = _ops()
    B, H, W, C = 2, 9, 13, 64
    seen = []
    real = ops.gemm

    def watched(layout, batch, M, N, Kr, A, lda, sA, Bm, ldb, sB, Cm, ldc, sC, zero_to=0, accumulate=False):
        rows = ldc <= 64 and ldc > N
        if rows and not accumulate:
            Cm.view(-1, ldc)[:, N:] = float("nan")            # (stands for the allocator's leftovers)
        out = real(layout, batch, M, N, Kr, A, lda, sA, Bm, ldb, sB, Cm, ldc, sC, zero_to=zero_to, accumulate=accumulate)
        if rows:
            seen.append((layout, N, ldc, bool((Cm.view(-1, ldc)[:, N:] == 0).all())))
        return out

    monkeypatch.setattr(ops, "gemm", watched)
    gen = torch.Generator().manual_seed(K)
    q, key, val = torch.randn(B, H, W, C, generator=gen).cuda(), torch.randn(B, K, 1, C, generator=gen).cuda(), torch.randn(B, K, 1, C, generator=gen).cuda()
    _run_tape(engine, lambda cx, a, b, c: engine.object_attention_core(cx, a, b, c, K, C), (q, key, val), torch.randn(B, H, W, C, generator=gen).cuda(), None)
    assert [s[:3] for s in seen] == [(ops.NT, K, ld), (ops.NT, K, ld)] and all(s[3] for s in seen), seen
    del seen[:]
    feats, logits = torch.randn(B, H, W, C, generator=gen).cuda(), _wide(torch.randn(B, H, W, K, generator=gen), ld, 0, fill=0.0)
    _run_tape(engine, lambda cx, f, l: engine.spatial_gather(cx, f, l, K), (feats, logits), torch.randn(B, K, 1, C, generator=gen).cuda(), None)
    assert [s[:3] for s in seen] == [(ops.NT, K, ld)] and all(s[3] for s in seen), seen
