"""The frozen form of catseg_bn_backward (csrc/norm.hip: bn_bwd_frozen_kernel + bn_bwd_frozen_merge_kernel) against
F.batch_norm(training=False) (+ residual, + ReLU) under autograd on the CPU.  Truth is the float64 run, the float32 CPU run is the yardstick
(`within` of tests/_yardstick.py: the kernel may be off by 4 x the float32 CPU error, floor 4 ulp of the reference's scale).  The residual
gradient is a copy of the masked dz, or ONE float32 addition to its base: compared for equality.

Shapes: per width C the rows that take the kernel's paths -- one row, fewer rows than row lanes, several row blocks with a ragged last one,
one block's tile (the 4-row unrolled sweep of its row lanes) + 1, and enough rows that under the cap on row blocks a block sweeps twice.
gamma has zeros and negative entries, running_var goes down to 1e-10, everywhere.

ReLU and rounding: an element whose pre-activation is within rounding distance of zero has a mask that float32 and float64 may decide
differently.  Every case therefore moves the elements whose float64 pre-activation lies within 2^-10 of zero -- relative to the largest
pre-activation of their channel -- out to 2^-9 (through y; through the residual where gamma == 0) and asserts in float64 that none is left.
No element is set aside.

Run with -s for the RATIO lines (worst ratio per quantity in _yardstick.WORST)."""
import ctypes

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from _yardstick import within

pytestmark = pytest.mark.gpu

NAN = float("nan")
EPS = float(np.float32(1e-5))
BAND = 2.0 ** -10


@pytest.fixture(scope="module")
def ops():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from miccai2021_cataract_semantic_segmentation_amd import ops as o
    return o


def split_of(rows, C):
    """plan_rows of csrc/norm.hip -> (rows per pass of a block, row blocks wanted, rows per block, row blocks): names the cases and
    derives the two row counts that depend on the plan"""
    cpt = (C + 3) // 4
    tpr = min(cpt, 64)
    rpp = 256 // tpr
    gy = (cpt + tpr - 1) // tpr
    want = max(64, min(1024, 2048 // gy))
    rpb = max((rows + want - 1) // want, 4 * rpp)
    rpb = (rpb + rpp - 1) // rpp * rpp
    return rpp, want, rpb, (rows + rpb - 1) // rpb


def tile_plus_one(C):
    return 4 * split_of(1, C)[0] + 1


def two_sweeps(C):
    """rows at which the row-block cap makes a block own two tiles (rows per block = 8 x its row lanes), the last block ragged"""
    rpp, want, _, _ = split_of(1, C)
    rows = want * 8 * rpp - 3
    assert split_of(rows, C)[2] == 8 * rpp and split_of(rows, C)[3] == want
    return rows


WIDTHS = [4, 8, 12, 64, 68, 200, 2052]
CASES = [(rows, C) for C in WIDTHS for rows in (1, 7, 257, tile_plus_one(C), two_sweeps(C))]


def case_id(case):
    rows, C = case
    _, _, rpb, nrb = split_of(rows, C)
    return "r%d-C%d-rpb%d-nrb%d" % (rows, C, rpb, nrb)


def gen(*seed):
    return torch.Generator().manual_seed(sum((i + 1) * int(s) for i, s in enumerate(seed)) % (2 ** 31))


def pre_activation(y, res, gamma, beta, rm, rv):
    """float64 pre-activation from the float32 inputs, and the per-channel scale = gamma / sqrt(rv + eps)"""
    sc = gamma.double() / torch.sqrt(rv.double() + EPS)
    pre = (y.double() - rm.double()) * sc + beta.double()
    return (pre if res is None else pre + res.double()), sc


def out_of_band(y, res, gamma, beta, rm, rv):
    """moves y (res where gamma == 0) until no float64 pre-activation lies within BAND of zero relative to its channel's largest one"""
    for _ in range(4):
        pre, sc = pre_activation(y, res, gamma, beta, rm, rv)
        ref = pre.abs().amax(0, keepdim=True)
        near = pre.abs() < BAND * ref
        if not near.any():
            break
        target = torch.where(pre < 0, -2 * BAND * ref, 2 * BAND * ref)
        live = (sc != 0).expand_as(pre)
        dy = torch.where(near & live, (target - pre) / torch.where(sc == 0, torch.ones_like(sc), sc), torch.zeros_like(pre))
        y = (y.double() + dy).float()
        if res is not None:
            res = (res.double() + torch.where(near & ~live, target - pre, torch.zeros_like(pre))).float()
    pre, _ = pre_activation(y, res, gamma, beta, rm, rv)
    left = int((pre.abs() < BAND * pre.abs().amax(0, keepdim=True)).sum())
    assert left == 0, "%d pre-activations are still within 2^-10 of zero" % left
    return y, res


def inputs(rows, C, with_res):
    g = gen(rows, C, int(with_res))
    rm = torch.randn(C, generator=g)
    rv = 10.0 ** (-10 + 10.6 * torch.rand(C, generator=g))          # 1e-10 .. 4
    rv[0] = 1e-10
    gamma = 1 + 0.5 * torch.randn(C, generator=g)
    gamma[1::4] = -gamma[1::4].abs() - 0.1                           # negative entries ...
    gamma[2::8] = 0.0                                                # ... and zeros (C = 4: channel 2)
    beta = 0.3 * torch.randn(C, generator=g)
    beta[gamma == 0] = torch.where(beta[gamma == 0] < 0, -0.5, 0.5)  # (a channel with gamma == 0 has pre = beta (+ res): not at zero)
    # y around the running mean at the width of the running statistics: the pre-activation is O(gamma) whatever running_var is
    y = rm + torch.sqrt(rv + EPS) * (torch.randn(rows, C, generator=g) + 0.3 * torch.randn(C, generator=g))
    res = torch.randn(rows, C, generator=g) if with_res else None
    dz = torch.randn(rows, C, generator=g)
    y, res = out_of_band(y, res, gamma, beta, rm, rv)
    return dict(y=y, res=res, dz=dz, gamma=gamma, beta=beta, rm=rm, rv=rv)


def reference(t, relu, dt):
    """autograd through F.batch_norm(training=False) (+ residual) (+ ReLU) in dtype dt -> dy, dgamma, dbeta, dres, z"""
    def leaf(v):      # (a copy: .to() of a tensor that already has the dtype returns the shared input itself)
        return v.detach().to(dt).clone().requires_grad_()
    y, gamma, beta = leaf(t["y"]), leaf(t["gamma"]), leaf(t["beta"])
    res = leaf(t["res"]) if t["res"] is not None else None
    v = F.batch_norm(y, t["rm"].to(dt), t["rv"].to(dt), gamma, beta, False, 0.0, EPS)
    if res is not None:
        v = v + res
    z = torch.relu(v) if relu else v
    z.backward(t["dz"].to(dt))
    return dict(dy=y.grad, dgamma=gamma.grad, dbeta=beta.grad, dres=None if res is None else res.grad, z=z.detach())


def wide(src, extra, fill=NAN):
    """src [rows, C] as a channel slice (offset `extra`) of a [rows, C + extra] buffer filled with `fill`: ld = C + extra"""
    if not extra:
        return src.contiguous().cuda()
    rows, C = src.shape
    buf = torch.full((rows, C + extra), fill, device="cuda")
    v = buf[:, extra:]
    v.copy_(src)
    return v


class Device:
    """the tensors of one case on the device, and the launches on them"""

    def __init__(self, ops, t):
        self.ops, self.t = ops, t
        self.gamma, self.beta, self.rm, self.rv = (t[k].cuda() for k in ("gamma", "beta", "rm", "rv"))
        self.scale = ops.bn_eval_scale(self.gamma, self.rv, EPS)        # the row the forward pass normalised with
        self.rows, self.C = t["y"].shape

    def z(self, relu):
        return self.ops.bn_apply(self.t["y"].cuda(), self.rm, self.scale, self.beta, None if self.t["res"] is None else self.t["res"].cuda(), relu)

    def bits(self):
        """the ReLU mask of z as catseg_bn_apply writes it (C % 8 == 0), straight through the C entry point"""
        from miccai2021_cataract_semantic_segmentation_amd._lib import BnApplyDesc, check, lib, ptr, stream
        y = self.t["y"].cuda()
        res = None if self.t["res"] is None else self.t["res"].cuda()
        z = torch.empty_like(y)
        mask = torch.zeros(lib.catseg_bn_mask_bytes(self.rows, self.C), dtype=torch.uint8, device="cuda")
        d = BnApplyDesc(y=ptr(y), ldy=self.C, mean=ptr(self.rm), scale=ptr(self.scale), beta=ptr(self.beta), residual=ptr(res), ldr=self.C,
                        z=ptr(z), ldz=self.C, rows=self.rows, C=self.C, relu=1, mask=ptr(mask))
        check(lib.catseg_bn_apply(ctypes.byref(d), stream()))
        return z, mask

    def run(self, source, extra=None, acc=False, grads=True, y=None, dz=None):
        """one frozen backward.  source: None (no ReLU) / "y" (recomputed) / "z" / "bits"; extra: {operand: floats added to its ld};
        acc: dres accumulates into a random base; grads=False: dgamma and dbeta NULL -> dict(dy, dgamma, dbeta, dres, base)"""
        ops, t, extra = self.ops, self.t, extra or {}
        rows, C = self.rows, self.C
        relu = source is not None
        dzd = wide(t["dz"] if dz is None else dz, extra.get("dz", 0))
        yd = wide(t["y"] if y is None else y, extra.get("y", 0))
        zsrc = None
        if source == "z":
            zsrc = wide(self.z(True).cpu(), extra.get("z", 0))
        elif source == "bits":
            zsrc = torch.empty(0, device="cuda")
            zsrc._relu_mask = self.bits()[1]
        dy = wide(torch.full((rows, C), NAN), extra.get("dy", 0))
        base = dres = None
        if t["res"] is not None:
            base = torch.randn(rows, C, generator=gen(rows, C, 9)) if acc else torch.full((rows, C), NAN)
            dres = wide(base, extra.get("dres", 0))
        dg = torch.full((C,), NAN, device="cuda") if grads else None
        db = torch.full((C,), NAN, device="cuda") if grads else None
        out = ops.bn_backward_frozen(dzd, zsrc, yd, self.rm, self.rv, EPS, self.scale, relu, dg, db, dres, acc, dy_out=dy, beta=self.beta)
        assert out.data_ptr() == dy.data_ptr()
        for name, v in (("dy", dy), ("dres", dres)):
            if v is not None and extra.get(name, 0):
                pad = v._base[:, :extra[name]] if v._base is not None else None
                assert pad is not None and torch.isnan(pad).all(), "%s: written outside its channel slice" % name
        return dict(dy=dy, dgamma=dg, dbeta=db, dres=dres, base=base if acc else None)


def check(cid, got, r64, r32, grads=True):
    if grads:
        within("frozen dbeta", cid, got["dbeta"], r64["dbeta"], r32["dbeta"])
        within("frozen dgamma", cid, got["dgamma"], r64["dgamma"], r32["dgamma"])
    within("frozen dy", cid, got["dy"], r64["dy"], r32["dy"])
    # dy = g * scale[c] and scale spans 1e5 over the channels (running_var from 1e-10): the same comparison with every channel brought to
    # its own largest |dy|, so that each of them counts (a channel with gamma == 0 has dy == 0: left as it is)
    top = r64["dy"].abs().amax(0, keepdim=True)
    top = torch.where(top == 0, torch.ones_like(top), top)
    within("frozen dy per channel", cid, got["dy"].detach().cpu().double() / top, r64["dy"] / top, r32["dy"].double() / top)
    if got["dres"] is not None:
        want = r32["dres"] if got["base"] is None else got["base"] + r32["dres"]        # a copy, or ONE float32 addition: exact
        assert torch.equal(got["dres"].cpu(), want), "%s: the residual gradient is not the masked dz%s" % (cid, "" if got["base"] is None else " added to its base")


def same_bits(a, b):
    return all((a[k] is None and b[k] is None) or torch.equal(a[k], b[k]) for k in ("dy", "dgamma", "dbeta", "dres"))


_REF = {}


def refs(rows, C, with_res, relu):
    """(inputs, float64 reference, float32 reference) of a case: computed once, shared by the tests, never modified"""
    key = (rows, C, with_res, relu)
    if key not in _REF:
        if len(_REF) > 8:
            _REF.clear()        # (the cases come grouped by shape: what is dropped here is not asked for again)
        t = _REF.get(("in", rows, C, with_res)) or inputs(rows, C, with_res)
        _REF[("in", rows, C, with_res)] = t
        _REF[key] = (t, reference(t, relu, torch.float64), reference(t, relu, torch.float32))
    return _REF[key]


# --------------------------------------------------------------------------------------- 1. every shape, every mask source
@pytest.mark.parametrize("case", CASES, ids=case_id)
def test_mask_sources_and_residual(ops, case):
    """no residual: the mask recomputed from y, and read from z; residual: read from z with dres written, and from the bits (C % 8 == 0;
    otherwise from z again) with dres accumulated; the float32 CPU mask agrees with float64 on every element by construction"""
    rows, C = case
    cid = case_id(case)
    t, r64, r32 = refs(rows, C, False, True)
    assert torch.equal(r64["z"] > 0, r32["z"] > 0)
    dev = Device(ops, t)
    a = dev.run("y")
    check(cid + "-recompute", a, r64, r32)
    b = dev.run("z")
    check(cid + "-z", b, r64, r32)
    assert same_bits(a, b), "%s: the recomputed mask and the mask of z give different bits" % cid
    t, r64, r32 = refs(rows, C, True, True)
    assert torch.equal(r64["z"] > 0, r32["z"] > 0)
    dev = Device(ops, t)
    check(cid + "-res-z-write", dev.run("z"), r64, r32)
    check(cid + "-res-%s-acc" % ("bits" if C % 8 == 0 else "z"), dev.run("bits" if C % 8 == 0 else "z", acc=True), r64, r32)


SMALL = [c for c in CASES if c[0] in (7, 257) or c[0] == tile_plus_one(c[1])]


# --------------------------------------------------------------------------------------- 2. without ReLU; without sums
@pytest.mark.parametrize("case", SMALL, ids=case_id)
def test_linear_and_null_parameter_gradients(ops, case):
    """no ReLU, with and without a residual branch; dgamma and dbeta NULL: dy and dres as before, and y is NOT read unless the mask is
    recomputed from it -- handed over as NaN it leaves no trace"""
    rows, C = case
    cid = case_id(case)
    nan_y = torch.full((rows, C), NAN)
    for with_res in (False, True):
        t, r64, r32 = refs(rows, C, with_res, False)
        dev = Device(ops, t)
        tag = cid + ("-lin+res" if with_res else "-lin")
        full = dev.run(None, acc=with_res)
        check(tag, full, r64, r32)
        bare = dev.run(None, acc=with_res, grads=False, y=nan_y)
        check(tag + "-nograd", bare, r64, r32, grads=False)
        assert torch.equal(bare["dy"], full["dy"])
    t, r64, r32 = refs(rows, C, True, True)
    dev = Device(ops, t)
    for source in ("z",) + (("bits",) if C % 8 == 0 else ()):
        bare = dev.run(source, grads=False, y=nan_y)
        check("%s-res-%s-nograd" % (cid, source), bare, r64, r32, grads=False)
    t, r64, r32 = refs(rows, C, False, True)
    check(cid + "-recompute-nograd", Device(ops, t).run("y", grads=False), r64, r32, grads=False)        # (here y IS the mask source)


# --------------------------------------------------------------------------------------- 3. row pitches
PITCH = [c for c in CASES if c[0] == 257 or (c[0] == tile_plus_one(c[1]) and c[1] in (12, 200, 2052))]


@pytest.mark.parametrize("case", PITCH, ids=case_id)
def test_row_pitches(ops, case):
    """ld = C + 4 for dz, y, z, dy and dres one at a time, and for all of them at once; the pad columns stay untouched"""
    rows, C = case
    cid = case_id(case)
    t, r64, r32 = refs(rows, C, True, True)
    dev = Device(ops, t)
    dense = dev.run("z")
    for extra in [{k: 4} for k in ("dz", "y", "z", "dy", "dres")] + [dict(dz=4, y=8, z=12, dy=16, dres=20)]:
        got = dev.run("z", extra=extra)
        assert ops.ld_of(got["dy"]) == C + extra.get("dy", 0) and ops.ld_of(got["dres"]) == C + extra.get("dres", 0)
        check("%s-ld(%s)" % (cid, ",".join(sorted(extra))), got, r64, r32)
        assert same_bits(got, dense)
    t, r64, r32 = refs(rows, C, False, True)
    dev = Device(ops, t)
    check(cid + "-recompute-ld(y,dz,dy)", dev.run("y", extra=dict(y=4, dz=8, dy=4)), r64, r32)


# --------------------------------------------------------------------------------------- 4. mask bits, record, determinism
@pytest.mark.parametrize("case", [(257, 8), (tile_plus_one(64), 64), (257, 200), (two_sweeps(64), 64)], ids=case_id)
def test_recomputed_mask_equals_the_bits_bn_apply_wrote(ops, case):
    """dz = 1 and a scale without zeros: dy != 0 exactly where the kernel's mask is set.  That mask -- recomputed from y with the forward's
    expression -- is the mask catseg_bn_apply wrote as bits, and z > 0, on every element; and the two sources give the same gradients"""
    rows, C = case
    t = dict(refs(rows, C, False, True)[0])
    t["gamma"] = torch.where(t["gamma"] == 0, torch.full_like(t["gamma"], 0.75), t["gamma"])
    dev = Device(ops, t)
    ones = torch.ones(rows, C)
    rec = dev.run("y", dz=ones)
    z, mask = dev.bits()
    unpacked = ((mask.cpu().view(-1, 1) >> torch.arange(8, dtype=torch.uint8)) & 1).bool().view(rows, C)
    assert torch.equal(unpacked, z.cpu() > 0)
    assert torch.equal(rec["dy"].cpu() != 0, unpacked), "the recomputed mask differs from the bits of the forward pass"
    assert same_bits(rec, dev.run("bits", dz=ones)) and same_bits(dev.run("y"), dev.run("bits"))


@pytest.mark.parametrize("case", [(7, 12), (257, 68), (tile_plus_one(2052), 2052), (two_sweeps(200), 200)], ids=case_id)
def test_dy_record_and_bit_identical_launches(ops, case, monkeypatch):
    """the amax record of dy holds the bits of max |dy| (the maximum over its slots, as a consumer reads it); two launches on the same input
    give the same bits in dy, dres, dgamma and dbeta (no atomics in the sums)"""
    rows, C = case
    monkeypatch.setattr(ops, "TRUNK", "f16x2")
    monkeypatch.setattr(ops, "PRECISION", "bf16x3")          # (the wrapper attaches a record on the f16x2 trunk only)
    t, r64, r32 = refs(rows, C, True, True)
    dev = Device(ops, t)
    a, b = dev.run("z", acc=True), dev.run("z", acc=True)
    assert same_bits(a, b)
    check(case_id(case) + "-record", a, r64, r32)
    rec = ops.amax_of(a["dy"])
    assert rec is not None and rec.numel() == ops.AMAX_WORDS
    slots = rec.view(16, ops.AMAX_WORDS // 16)[:, 0]
    assert int(slots.max()) == int(a["dy"].abs().max().view(torch.int32)) and int(slots.max()) > 0
    assert int(rec.view(16, -1)[:, 1:].abs().max()) == 0, "words outside the record's slots were written"
