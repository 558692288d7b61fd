"""The route planner (ops.fwd_route / dgrad_route / wgrad_route) on the layers README / DESIGN name, and the predictors (ops.h2_dy_route,
ops.concat_planes_route) against the planner over a grid of shapes.  No device: the planner reads shapes, flags and operand facts only.
The expected names are read off the ladders of conv_fwd / conv_bwd_data / conv_bwd_weight as they stood before the planner; the recorded
traces of tests/golden/route_traces.json (tests/test_route_trace_gpu.py) are the cross-check on the GPU."""
import pytest

from miccai2021_cataract_semantic_segmentation_amd import ops
from miccai2021_cataract_semantic_segmentation_amd.ops import Layer, Route

S4, S8 = (8, 136, 240), (8, 68, 120)            # the stride-4 and stride-8 maps of the bench shape (8 x 3 x 544 x 960)
FORCED = dict(B3_MIN_TAPS=1, B3_MIN_K=64, B3_MIN_N=32, B3_MIN_TILES=1, B3_MIN_WGRAD_ROWS=1, DCONV3_MIN_ROWS=1, P1_MIN_ROWS=1, P1_WGRAD_MIN_DIM=1,
              G1_MIN_ROWS=1, G1_DGRAD_MIN_CIN=1)     # the reduced thresholds of conftest.py's `precision` fixture


@pytest.fixture
def plan():
    """set ops attributes for one test and restore them"""
    saved = {}

    def set_(**kw):
        for k, v in kw.items():
            saved.setdefault(k, getattr(ops, k))
            setattr(ops, k, v)
    yield set_
    for k, v in saved.items():
        setattr(ops, k, v)


def routes(L):
    return ops.fwd_route(L), ops.dgrad_route(L), ops.wgrad_route(L)


def test_default_plan_on_the_named_layers():
    assert ops.plan()["precision"] == "bf16x3" and ops.HEADS == "f16x2" and ops.TRUNK == "f16x2" and ops.PLANES
    H2 = ops.H2_BLOCKED
    # the 3x3 720 -> 512 head of OCRNet-HRNet: blocked f16x2 planes in all three directions, with or without records
    for recs in (False, True):
        assert routes(Layer(S4 + (720,), 512, 3, 3, 1, 1, x_amax=recs, dy_amax=recs)) == (H2, H2, H2)
    # trunk 3x3: 96 / 192 / 384 channels with planes -> the planes kernel forward; backward through the entry points is the in-kernel split
    for shape, C in ((S4, 96), (S8, 96), (S8, 192), (S8, 384)):
        L = Layer(shape + (C,), C, 3, 3, 1, 1, x_planes=True, x_amax=True, dy_amax=True)
        assert routes(L) == (ops.D3P, ops.D3H, ops.D3H), C
        assert ops.fwd_route(Layer(shape + (C,), C, 3, 3, 1, 1, x_amax=True)) == ops.D3P       # (a record is enough: one split pass)
        assert ops.fwd_route(Layer(shape + (C,), C, 3, 3, 1, 1, x_amax=True, bias=True)) == ops.D3H
    # 48 channels: never the planes route; the record decides between f16x2 and bf16x3
    assert routes(Layer(S4 + (48,), 48, 3, 3, 1, 1, x_amax=True, dy_amax=True)) == (ops.D3H, ops.D3H, ops.D3H)
    assert routes(Layer(S4 + (48,), 48, 3, 3, 1, 1)) == (ops.D3, ops.D3, ops.D3)
    assert ops.wgrad_route(Layer(S4 + (48,), 48, 3, 3, 1, 1, x_amax=True)) == ops.D3          # (both operands need one)
    # the wide 1x1 1024 -> 512 at 261 120 pixels, and at 65 280 (OCRNet-R50)
    for shape in (S4, S8):
        assert routes(Layer(shape + (1024,), 512, 1, 1, x_amax=True, dy_amax=True)) == (H2, H2, H2)
    # narrow 1x1 layers with records: the pointwise kernel; without: fp32
    assert routes(Layer(S4 + (256,), 64, 1, 1, x_amax=True, dy_amax=True)) == (ops.P1R, ops.P1R, ops.P1R)
    assert routes(Layer(S4 + (512,), 256, 1, 1, x_amax=True, dy_amax=True)) == (ops.P1R, ops.P1R, ops.P1R)
    assert routes(Layer(S4 + (256,), 64, 1, 1)) == (ops.F32, ops.F32, ops.F32)
    assert routes(Layer(S8 + (256,), 64, 1, 1, x_amax=True, dy_amax=True)) == (ops.P1R, ops.P1R, ops.P1R)      # 65 280 pixels >= p1_min_rows
    assert routes(Layer((8, 34, 60, 256), 64, 1, 1, x_amax=True, dy_amax=True)) == (ops.F32, ops.F32, ops.F32)
    # 3x3 / stride 2, 96 -> 192: gather launches with records, fp32 without
    assert routes(Layer(S4 + (96,), 192, 3, 3, 2, 1, x_amax=True, dy_amax=True)) == (ops.S2P, ops.S2P, ops.S2P)
    assert routes(Layer(S4 + (96,), 192, 3, 3, 2, 1)) == (ops.F32, ops.F32, ops.F32)
    assert ops.dgrad_route(Layer(S4 + (32,), 96, 3, 3, 2, 1, x_amax=True, dy_amax=True)) == ops.F32     # below g1_dgrad_min_cin input channels
    # exact operands: fp32 forward (the flag is a forward flag)
    assert ops.fwd_route(Layer(S4 + (720,), 512, 3, 3, 1, 1, exact=True)) == ops.F32
    assert ops.fwd_route(Layer(S4 + (48,), 48, 3, 3, 1, 1, x_amax=True, exact=True)) == ops.F32
    assert ops.fwd_route(Layer(S4 + (256,), 64, 1, 1, x_amax=True, exact=True)) == ops.F32
    # the stem layout, grouped layers
    assert ops.fwd_route(Layer((8, 544, 960, 4), 64, 7, 7, 2, 3, stem4=True, w4d=False)) == ops.F32
    assert ops.wgrad_route(Layer((8, 544, 960, 4), 64, 7, 7, 2, 3, stem4=True, w4d=False)) == ops.F32
    assert routes(Layer(S8 + (1024,), 1024, 3, 3, 1, 1, groups=32)) == (ops.F32, ops.F32, ops.F32)


GRID = ([(S4, 720, 512, 3), (S4, 1024, 512, 1), (S4, 48, 48, 3), (S4, 512, 256, 1), (S4, 256, 512, 1)]            # test_route_predicate_on_the_bench_shapes
        + [(S8, 2048, 512, 3), (S8, 512, 2048, 1), (S8, 1024, 256, 1), (S4, 96, 96, 3), (S4, 256, 48, 3), (S8, 512, 512, 3), (S4, 64, 64, 1),
           ((2, 24, 40), 64, 64, 3), ((2, 24, 40), 128, 64, 1), ((2, 24, 40), 720, 512, 3), ((2, 24, 40), 48, 48, 3), ((2, 24, 40), 96, 100, 3)])


def test_plan_variants(plan):
    L = [Layer(s + (ci,), co, k, k, 1, k // 2, x_amax=True, dy_amax=True, x_planes=True) for s, ci, co, k in GRID]
    L += [Layer(S4 + (96,), 192, 3, 3, 2, 1, x_amax=True, dy_amax=True)]
    plan(PRECISION="fp32")
    for l in L:
        assert routes(l) == (ops.F32, ops.F32, ops.F32)
    plan(PRECISION="bf16x3", HEADS="bf16x3")
    head = Layer(S4 + (720,), 512, 3, 3, 1, 1)
    assert routes(head) == (Route("b3", True), Route("b3", True), Route("b3", False))
    plan(HEADS="f16x2", H2T_BLOCKED=False)
    assert routes(head) == (ops.H2_BLOCKED, ops.H2_BLOCKED, Route("h2", False))
    plan(H2T_BLOCKED=True, TRUNK="bf16x3")
    trunk = Layer(S4 + (96,), 96, 3, 3, 1, 1, x_amax=True, dy_amax=True, x_planes=True)
    assert routes(trunk) == (ops.D3, ops.D3, ops.D3)
    assert routes(Layer(S4 + (256,), 64, 1, 1, x_amax=True, dy_amax=True)) == (ops.F32, ops.F32, ops.F32)      # p1 / s2p ride on the f16x2 trunk
    plan(TRUNK="f16x2", PLANES=False)
    assert routes(trunk) == (ops.D3H, ops.D3H, ops.D3H)
    plan(PLANES=True, P1=False, G1=False)
    assert routes(Layer(S4 + (256,), 64, 1, 1, x_amax=True, dy_amax=True)) == (ops.F32, ops.F32, ops.F32)
    assert routes(Layer(S4 + (96,), 192, 3, 3, 2, 1, x_amax=True, dy_amax=True)) == (ops.F32, ops.F32, ops.F32)


class _T:
    """shape-only stand-in for a device tensor (the predictors read .shape / .dim() / .is_cuda, never data)"""
    is_cuda = True

    def __init__(self, *shape):
        self.shape = tuple(shape)
        self._amax = object()

    def dim(self):
        return len(self.shape)

    def stride(self, i):
        n = 1
        for s in self.shape[i + 1:]:
            n *= s
        return n


class _Conv:
    def __init__(self, ci, co, k):
        self.in_channels, self.out_channels, self.kernel_size, self.stride, self.padding, self.dilation = ci, co, (k, k), (1, 1), (k // 2, k // 2), (1, 1)
        self.groups, self.bias = 1, None


@pytest.mark.parametrize("forced", [False, True])
def test_predictors_against_the_planner(plan, forced):
    if forced:
        plan(**FORCED)
    H2 = ops.H2_BLOCKED
    seen = set()
    for (B, H, W), ci, co, k in GRID:
        L = Layer((B, H, W, ci), co, k, k, 1, k // 2, x_amax=True, dy_amax=True)
        x, y, w = _T(B, H, W, ci), _T(B, H, W, co), _T(co, ci, k, k)
        for need_dx in (False, True):
            want = co % 64 == 0 and ops.wgrad_route(L) == H2 and (not need_dx or ops.dgrad_route(L) == H2)
            assert ops.h2_dy_route(x, y, w, k, k, 1, k // 2, 1, 1, need_dx) == want, (B, H, W, ci, co, k, need_dx)
            seen.add(want)
        if ci % 16 == 0:
            Lc = Layer((B, H, W, ci), co, k, k, 1, k // 2)
            want = ops.fwd_route(Lc) == H2 and ops.wgrad_route(Lc) == H2
            assert ops.concat_planes_route([_T(B, H, W, ci)], [_Conv(ci, co, k)]) == want, (B, H, W, ci, co, k)
            seen.add(want)
    assert seen == {False, True}
    # the answers of tests/test_heads_dy_planes_gpu.py::test_route_predicate_on_the_bench_shapes, under the production thresholds
    if not forced:
        for ci, co, k, want in [(720, 512, 3, True), (1024, 512, 1, True), (48, 48, 3, False), (512, 256, 1, False), (256, 512, 1, False)]:
            assert ops.h2_dy_route(_T(*S4, ci), _T(*S4, co), _T(co, ci, k, k), k, k, 1, k // 2, 1, 1, True) == want, (ci, co, k)


def test_switches_of_the_predictors(plan):
    x, y, w = _T(*S4, 720), _T(*S4, 512), _T(512, 720, 3, 3)
    assert ops.h2_dy_route(x, y, w, 3, 3, 1, 1, 1, 1, True)
    assert ops.concat_planes_route([_T(*S4, 720)], [_Conv(720, 512, 3)])
    plan(HEAD_DY_PLANES=False, CONCAT_PLANES=False)
    assert not ops.h2_dy_route(x, y, w, 3, 3, 1, 1, 1, 1, True)
    assert not ops.concat_planes_route([_T(*S4, 720)], [_Conv(720, 512, 3)])
    plan(HEAD_DY_PLANES=True, CONCAT_PLANES=True, H2T_BLOCKED=False)
    assert not ops.h2_dy_route(x, y, w, 3, 3, 1, 1, 1, 1, True)
    assert not ops.concat_planes_route([_T(*S4, 720)], [_Conv(720, 512, 3)])
