"""Dropout2d of the OCRNet heads (csrc/dropout.hip, the DROP variants of csrc/headfuse.h, engine.Dropout2d, models/OCR.py): the generator
against its numpy restatement bit for bit, the fused kernels against fp64 with an injected mask, the layer through the engine on the fused
and the separate-pass route, the reference fixture, models.OCRNet, hipGraph replay and the manager."""
import os

import numpy as np
import pytest
import torch

import _dropout_ref as R

pytestmark = pytest.mark.gpu


@pytest.fixture()
def ops():
    from miccai2021_cataract_semantic_segmentation_amd import ops as o
    yield o
    o.PROFILE = None
    o.release_b3_cache()


def _i32(words):
    return torch.tensor([w - (1 << 32) if w >= 1 << 31 else w for w in words], dtype=torch.int32)


# ------------------------------------------------------------------------------------------------ generator
@pytest.mark.parametrize("rank", [0, 1])
@pytest.mark.parametrize("p", [0.1, 0.5, 1.0])
@pytest.mark.parametrize("shape", [(3, 6), (1, 64), (8, 512)])
def test_generator_matches_the_restatement(ops, shape, p, rank):
    B, C = shape
    seed, layer = 0x9E3779B97F4A7C15, 1
    state = _i32([seed & 0xFFFFFFFF, seed >> 32, layer | rank << 16, 0]).cuda()
    for draw in range(3):
        dm = ops.dropout2d_mask(state, p, B, C)
        torch.cuda.synchronize()
        kept, mult, bits = R.mask(seed, layer, rank, draw, p, B, C)
        assert np.array_equal(dm.mult.cpu().numpy().view(np.uint32), mult.view(np.uint32)), (draw, "multipliers")
        assert dm.keep == float(R.keep_of(p))
        if C % 32 == 0:
            got = dm.bits.cpu().numpy().view(np.uint32)
            assert np.array_equal(got, bits), (draw, "bits")
            unpacked = ((got[:, :, None] >> np.arange(32, dtype=np.uint32)) & 1).reshape(B, C).astype(bool)
            assert np.array_equal(unpacked, dm.mult.cpu().numpy() != 0)
        else:
            assert dm.bits is None
        if p == 1.0:
            assert not dm.mult.cpu().numpy().any()
    assert state.cpu().tolist() == _i32([seed & 0xFFFFFFFF, seed >> 32, layer | rank << 16, 3]).tolist()


def test_apply_kernel(ops):
    g = torch.Generator().manual_seed(3)
    x = torch.randn(3, 5, 7, 36, generator=g).cuda()[..., :20]            # (row stride 36, 20 channels)
    keep01 = (torch.rand(3, 20, generator=g) > 0.4).float().cuda()
    dm = ops.dropout2d_mask_fixed(keep01, 0.4)
    assert dm.bits is None
    out = ops.dropout2d_apply(x, dm)
    want = x * dm.mult[:, None, None, :]
    assert torch.equal(out, want)
    xc = x.contiguous()
    assert ops.dropout2d_apply(xc, dm, out=xc) is xc and torch.equal(xc, want)      # in place


# ------------------------------------------------------------------------------------------------ fused kernels
def _planes_to_f64(blk, scale, C):
    e = int(scale.cpu()[1])
    hl = blk.cpu().view(torch.float16).double()          # [2, C/16, rows, 16]
    v = (hl[0] + hl[1]) * 2.0 ** -e
    return v.permute(1, 0, 2).reshape(v.shape[1], -1)[:, :C], e        # [rows, C]


def _keep_table(B, C, g, p):
    """random, but image 0 loses every channel and image 1 keeps every one (where there are that many images)"""
    keep01 = (torch.rand(B, C, generator=g) >= p).float()
    if B >= 2:
        keep01[0] = 0.0
        keep01[1] = 1.0
    return keep01


@pytest.mark.parametrize("shape", [(3, 5, 7, 64, 7), (4, 3, 5, 128, 25), (2, 17, 23, 512, 25), (1, 8, 4, 128, 32)])
def test_fused_kernels_vs_fp64(ops, shape):
    """tests/test_headfuse_gpu.py::test_kernels_vs_fp64 with a mask between the ReLU and the classifier; its bars.  The fp64 evaluation uses the
    stored fp32 multipliers: the dropout adds one fp32 rounding per element (6e-8 relative) under bars of 2 - 4e-6."""
    B, H, W, C, K = shape
    rows, p = B * H * W, 0.4
    g = torch.Generator().manual_seed(rows + C + K)
    dev = torch.device("cuda")
    mean = torch.randn(C, generator=g).double()
    inv = torch.exp(0.5 * torch.randn(C, generator=g)).double()
    gamma, beta = (1 + 0.3 * torch.randn(C, generator=g)), (0.2 * torch.randn(C, generator=g))
    stats = torch.cat([mean, inv]).float()
    scale32 = gamma * stats[C:]
    zt = torch.randn(rows, C, generator=g).double()
    zt = torch.where(zt.abs() < 1e-3, torch.full_like(zt, 1e-3) * torch.where(zt < 0, -1.0, 1.0), zt)
    y = (stats[:C].double() + (zt - beta.double()) / scale32.double()).float()
    wh = (torch.randn(K, C, generator=g) / C ** 0.5)
    bh = torch.randn(K, generator=g)
    keep01 = _keep_table(B, C, g, p)
    dm = ops.dropout2d_mask_fixed(keep01.to(dev), p)
    mult = dm.mult.cpu()
    assert torch.equal(mult != 0, keep01 != 0) and np.array_equal(dm.bits.cpu().numpy().view(np.uint32), R.tables(keep01.numpy() != 0, p)[1])
    dl = torch.full((B, H, W, 32), float("nan"))
    dl[..., :K] = torch.randn(B, H, W, K, generator=g) * 3e-6
    r = R.head_fp64(y, stats[:C], stats[C:], gamma, beta, scale32, wh, bh, mult, dl[..., :K].reshape(rows, K), H * W)
    assert float(r["pre"].abs().min()) > 1e-4
    y_d = y.view(B, H, W, C).to(dev)
    # ---- forward
    out = ops.head_fwd(y_d, stats[:C].to(dev), scale32.to(dev), beta.to(dev), wh.to(dev), bh.to(dev), K, 32, drop=dm)
    torch.cuda.synchronize()
    assert out.shape == (B, H, W, K) and ops.ld_of(out) == 32
    ref, z64 = r["logits"], r["z"]
    got = out.reshape(rows, K).cpu().double()
    err = float((got - ref).abs().max())
    print("forward: err %.3g, bar %.3g" % (err, 2e-6 * float(ref.abs().max() + z64.abs().max())))
    assert err <= 2e-6 * float(ref.abs().max() + z64.abs().max()), err
    if B >= 2:       # the image without a channel: the bias alone
        assert torch.equal(out[0].reshape(-1, K), bh.to(dev).expand(H * W, K))
    pad = out.as_strided((rows, 32), (32, 1))[:, K:]
    assert float(pad.abs().max()) == 0.0 if K < 32 else True
    # ---- backward: NaN in the padding columns of the logits gradient must not matter
    dl_d = dl.to(dev)[..., :K]
    dwh, dbh = torch.full((K, C), float("nan"), device=dev), torch.full((K,), float("nan"), device=dev)
    dgam, dbet, dbias = torch.empty(C, device=dev), torch.empty(C, device=dev), torch.full((C,), float("nan"), device=dev)
    blk, sc = ops.head_backward(dl_d, y_d, stats.to(dev), gamma.to(dev), beta.to(dev), wh.to(dev), dwh, dbh, dgam, dbet, dbias, drop=dm)
    torch.cuda.synchronize()
    dl64 = dl[..., :K].reshape(rows, K).double()
    gz, xh, dy64 = r["g"], r["xh"], r["dy"]
    tol = lambda t: 3e-6 * float(t.abs().max())
    figures = {"dwh": float((dwh.cpu().double() - r["dwh"]).abs().max()), "dbh": float((dbh.cpu().double() - r["dbh"]).abs().max()),
               "dbeta": float((dbet.cpu().double() - r["dbeta"]).abs().max()), "dgamma": float((dgam.cpu().double() - r["dgamma"]).abs().max())}
    print("backward:", figures)
    assert figures["dwh"] <= tol(r["dwh"]) + 1e-6 * float((dl64.abs().t() @ z64.abs()).max())
    assert figures["dbh"] <= 1e-6 * float(dl64.abs().sum(0).max())
    assert figures["dbeta"] <= 1e-6 * float(gz.abs().sum(0).max())
    assert figures["dgamma"] <= 1e-6 * float((gz * xh).abs().sum(0).max())
    v, e = _planes_to_f64(blk, sc, C)
    amax = float(dy64.abs().max())
    bound = np.frombuffer(np.int32(int(sc.cpu()[0])).tobytes(), dtype=np.float32)[0]
    assert bound >= amax and float(bound) * 2.0 ** e < 2.0 ** 15
    err = float((v - dy64).abs().max())
    print("dy planes: err %.3g, bar %.3g" % (err, 4e-6 * amax))
    assert err <= 4e-6 * amax, (err, amax)
    assert float((dbias.cpu().double() - r["dbias"]).abs().max()) <= 2e-6 * float(dy64.abs().sum(0).max())
    # deterministic: a second call reproduces every output bit for bit
    out2 = ops.head_fwd(y_d, stats[:C].to(dev), scale32.to(dev), beta.to(dev), wh.to(dev), bh.to(dev), K, 32, drop=dm)
    dwh2, dbh2 = torch.empty_like(dwh), torch.empty_like(dbh)
    dgam2, dbet2 = torch.empty_like(dgam), torch.empty_like(dbet)
    blk2, sc2 = ops.head_backward(dl_d, y_d, stats.to(dev), gamma.to(dev), beta.to(dev), wh.to(dev), dwh2, dbh2, dgam2, dbet2, None, drop=dm)
    torch.cuda.synchronize()
    assert torch.equal(out, out2) and torch.equal(blk, blk2) and torch.equal(sc, sc2) and torch.equal(dwh, dwh2) and torch.equal(dbh, dbh2)
    assert torch.equal(dgam, dgam2) and torch.equal(dbet, dbet2)


def test_all_kept_mask_reproduces_the_kernels_without_dropout(ops):
    """keep = 1 (p = 0 through the DROP kernels) and every bit set: the same bits as catseg_head_fwd / catseg_head_backward"""
    B, H, W, C, K = 3, 5, 7, 128, 25
    g = torch.Generator().manual_seed(11)
    dev = torch.device("cuda")
    y = torch.randn(B, H, W, C, generator=g).to(dev)
    stats = torch.cat([0.1 * torch.randn(C, generator=g), torch.exp(0.3 * torch.randn(C, generator=g))]).to(dev)
    gamma, beta = (1 + 0.3 * torch.randn(C, generator=g)).to(dev), (0.2 * torch.randn(C, generator=g)).to(dev)
    wh, bh = (torch.randn(K, C, generator=g) / C ** 0.5).to(dev), torch.randn(K, generator=g).to(dev)
    dl = ops.new_act(B, H, W, K, dev, ld=32, zero=True)
    dl.copy_(torch.randn(B, H, W, K, generator=g).to(dev) * 1e-4)
    dm = ops.dropout2d_mask_fixed(torch.ones(B, C, device=dev), 0.0)
    assert dm.keep == 1.0
    res = []
    for drop in (None, dm):
        out = ops.head_fwd(y, stats[:C], gamma * stats[C:], beta, wh, bh, K, 32, drop=drop)
        grads = [torch.empty(K, C, device=dev), torch.empty(K, device=dev), torch.empty(C, device=dev), torch.empty(C, device=dev),
                 torch.empty(C, device=dev)]
        blk, sc = ops.head_backward(dl, y, stats, gamma, beta, wh, grads[0], grads[1], grads[2], grads[3], grads[4], drop=drop)
        res.append([out, blk, sc] + grads)
    torch.cuda.synchronize()
    for a, b in zip(*res):
        assert torch.equal(a, b)


# ------------------------------------------------------------------------------------------------ the layer through the engine
def _net(with_bias, Cin, Cout, k, K, p):
    from miccai2021_cataract_semantic_segmentation_amd.engine import BatchNorm2d, Conv2d, Dropout2d, EngineNet, conv_bn_act

    class Net(EngineNet):
        def __init__(self):
            super().__init__()
            self.pre = Conv2d(Cin, Cin, 1, bias=False)
            self.pre_bn = BatchNorm2d(Cin)
            self.conv = Conv2d(Cin, Cout, k, 1, k // 2, bias=with_bias)
            self.bn = BatchNorm2d(Cout)
            self.drop = Dropout2d(p)
            self.head = Conv2d(Cout, K, 1, 1, 0, bias=True)

        def _body(self, cx, x):
            t = conv_bn_act(cx, x.permute(0, 2, 3, 1).contiguous(), self.pre, self.pre_bn)
            return [conv_bn_act(cx, t, self.conv, self.bn, head=self.head, drop=self.drop)]
    return Net


@pytest.mark.parametrize("case", [(True, 208, 256, 3, 28), (False, 256, 128, 1, 8)])
def test_layer_through_the_engine_matches_the_separate_passes(ops, case):
    """tests/test_headfuse_gpu.py's test of the same name with Dropout2d(0.5) and one injected mask on both routes; its bars"""
    with_bias, Cin, Cout, k, K = case
    saved = (ops.PRECISION, ops.B3_MIN_TAPS, ops.B3_MIN_K, ops.B3_MIN_N, ops.B3_MIN_TILES, ops.B3_MIN_WGRAD_ROWS, ops.HEAD_FUSE,
             ops.B3_1X1_MIN_DIM, ops.B3_1X1_MIN_PROD, ops.B3_1X1_MIN_ROWS)
    try:
        ops.PRECISION, ops.B3_MIN_TAPS, ops.B3_MIN_K, ops.B3_MIN_N, ops.B3_MIN_TILES, ops.B3_MIN_WGRAD_ROWS = "bf16x3", 1, 64, 32, 1, 1
        ops.B3_1X1_MIN_DIM, ops.B3_1X1_MIN_PROD, ops.B3_1X1_MIN_ROWS = 64, 64 * 64, 64
        torch.manual_seed(5)
        net = _net(with_bias, Cin, Cout, k, K, 0.5)().cuda().train()
        net.drop.fixed_mask = _keep_table(2, Cout, torch.Generator().manual_seed(6), 0.5)
        x = torch.randn(2, Cin, 24, 40, device="cuda")
        gout = torch.randn(2, K, 24, 40, device="cuda") * 1e-3
        res, outs = {}, {}
        for mode in (True, False):
            ops.HEAD_FUSE = mode
            ops.release_b3_cache()
            net.zero_grad()
            ops.PROFILE = []
            out = net(x)
            out = out[0] if isinstance(out, (tuple, list)) else out
            out.backward(gout)
            torch.cuda.synchronize()
            kinds = [q[0] for q in ops.PROFILE]
            ops.PROFILE = None
            assert "wgrad_h2" in kinds and "dgrad_h2" in kinds, kinds
            assert ("hbm:head_fwd_drop" in kinds and "hbm:head_backward_drop" in kinds) == mode, kinds
            assert (kinds.count("hbm:dropout2d_apply") == 2) == (not mode), kinds
            assert "hbm:head_fwd" not in kinds and "hbm:head_backward" not in kinds and kinds.count("dropout2d_mask") == 1, kinds
            res[mode] = {n: q.grad.detach().clone() for n, q in net.named_parameters()}
            outs[mode] = out.detach().clone()
        assert int(net.drop.state[3]) == 0                      # (an injected mask draws nothing)
        a, b = outs[True].double(), outs[False].double()
        assert float((a - b).abs().max()) <= 2e-6 * float(b.abs().max()), float((a - b).abs().max())
        assert float((outs[True][0] - net.head.bias.detach()[:, None, None]).abs().max()) == 0.0       # image 0: every channel dropped
        for n in res[True]:
            a, b = res[True][n].double(), res[False][n].double()
            scale = float(b.abs().max())
            if n == "conv.bias":
                assert float((a - b).abs().max()) <= 1e-5 * float(res[False]["conv.weight"].abs().sum() / b.numel() + scale)
                continue
            assert float((a - b).abs().max()) <= 2e-5 * scale, (n, float((a - b).abs().max()), scale)
    finally:
        (ops.PRECISION, ops.B3_MIN_TAPS, ops.B3_MIN_K, ops.B3_MIN_N, ops.B3_MIN_TILES, ops.B3_MIN_WGRAD_ROWS, ops.HEAD_FUSE,
         ops.B3_1X1_MIN_DIM, ops.B3_1X1_MIN_PROD, ops.B3_1X1_MIN_ROWS) = saved
        ops.PROFILE = None


# ------------------------------------------------------------------------------------------------ the reference fixture
@pytest.mark.parametrize("tag", ["ocr", "interm"])
def test_fused_kernels_vs_the_reference_fixture(ops, tag):
    """tests/golden/dropout.npz (tests/golden/make_golden_dropout.py): the reference's modules in train mode, their masks injected.  Bars: those
    of the ocr_modules.npz comparisons (tests/test_oracle_golden.py::test_ocr_modules): 2e-5 absolute forward, 2e-4 absolute on gradients."""
    g = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "dropout.npz"))
    dev = torch.device("cuda")
    T = lambda n: torch.from_numpy(g[tag + "_" + n])
    y = T("y").permute(0, 2, 3, 1).contiguous()
    B, H, W, C = y.shape
    rows64 = y.reshape(-1, C).double()
    mean, inv = rows64.mean(0), (rows64.var(0, unbiased=False) + 1e-5).rsqrt()
    stats = torch.cat([mean, inv]).float().to(dev)
    gamma, beta = T("gamma").to(dev), T("beta").to(dev)
    wh, bh = T("wh").reshape(-1, C).contiguous().to(dev), T("bh").to(dev)
    K, p = wh.shape[0], float(g[tag + "_p"])
    dm = ops.dropout2d_mask_fixed((T("mult") != 0).float().to(dev), p)
    assert torch.equal(dm.mult.cpu(), T("mult"))
    out = ops.head_fwd(y.to(dev), stats[:C], gamma * stats[C:], beta, wh, bh, K, 32, drop=dm)
    np.testing.assert_allclose(out.cpu().numpy(), T("logits").permute(0, 2, 3, 1).numpy(), atol=2e-5)
    dl = ops.new_act(B, H, W, K, dev, ld=32, zero=True)
    dl.copy_(T("dlogits").permute(0, 2, 3, 1).to(dev))
    dwh, dbh, dgam, dbet = torch.empty(K, C, device=dev), torch.empty(K, device=dev), torch.empty(C, device=dev), torch.empty(C, device=dev)
    blk, sc = ops.head_backward(dl, y.to(dev), stats, gamma, beta, wh, dwh, dbh, dgam, dbet, None, drop=dm)
    torch.cuda.synchronize()
    np.testing.assert_allclose(dwh.cpu().numpy(), T("dwh").reshape(K, C).numpy(), atol=2e-4)
    np.testing.assert_allclose(dbh.cpu().numpy(), T("dbh").numpy(), atol=2e-4)
    np.testing.assert_allclose(dgam.cpu().numpy(), T("dgamma").numpy(), atol=2e-4)
    np.testing.assert_allclose(dbet.cpu().numpy(), T("dbeta").numpy(), atol=2e-4)
    v, _ = _planes_to_f64(blk, sc, C)
    np.testing.assert_allclose(v.numpy(), T("dy").permute(0, 2, 3, 1).reshape(-1, C).double().numpy(), atol=2e-4)


# ------------------------------------------------------------------------------------------------ models.OCRNet
def _ocrnet(dropout=None):
    from miccai2021_cataract_semantic_segmentation_amd.models import OCRNet
    cfg = {"backbone": "resnet50", "out_stride": 8, "pretrained": False}
    if dropout is not None:
        cfg["dropout"] = dropout
    return OCRNet(cfg, 3)


def _profiled(ops, fn):
    ops.PROFILE = []
    try:
        res = fn()
        torch.cuda.synchronize()
        return res, [q[0] for q in ops.PROFILE]
    finally:
        ops.PROFILE = None


def test_ocrnet_with_dropout(ops):
    from miccai2021_cataract_semantic_segmentation_amd.engine import Dropout2d, dropout_layers
    torch.manual_seed(0)
    plain, zero, drop = _ocrnet(), _ocrnet(0.0), _ocrnet(0.4)                # (dropout = 0.4 constructs: the model refused the key before)
    assert list(plain.state_dict()) == list(zero.state_dict()) == list(drop.state_dict())
    assert isinstance(drop.interm_prediction_head[3], Dropout2d) and isinstance(drop.spatial_ocr_head.conv_bn_dropout[3], Dropout2d)
    assert [d.p for d in dropout_layers(drop)] == [0.4, 0.4] and sorted(d.layer for d in dropout_layers(drop)) == [0, 1]
    zero.load_state_dict(plain.state_dict())
    drop.load_state_dict(plain.state_dict())
    plain.cuda(), zero.cuda(), drop.cuda()
    x = torch.rand(2, 3, 64, 96, generator=torch.Generator().manual_seed(1)).cuda()

    def step(model):
        model.zero_grad()
        out = model(x)
        (out[0].sum() + out[1].sum()).backward()
        return [o.detach().clone() for o in out]
    # p = 0: the launches of a model built without the key, none of them a dropout's
    plain.train(), zero.train(), drop.train()
    out_p, kinds_p = _profiled(ops, lambda: step(plain))
    out_z, kinds_z = _profiled(ops, lambda: step(zero))
    assert kinds_z == kinds_p and not any("drop" in k for k in kinds_z)
    assert all(torch.equal(a, b) for a, b in zip(out_p, out_z))
    assert all(int(d.state.abs().sum()) == 0 and not d._seeded for d in dropout_layers(zero))
    # p = 0.4 in training: one draw per layer and step, and it changes the logits
    out_d, kinds_d = _profiled(ops, lambda: step(drop))
    assert kinds_d.count("dropout2d_mask") == 2
    assert kinds_d.count("hbm:dropout2d_apply") + 2 * kinds_d.count("hbm:head_fwd_drop") == 4, kinds_d      # forward + backward per layer
    assert not torch.equal(out_d[1], out_p[1]) and all(bool(torch.isfinite(o).all()) for o in out_d)
    assert [int(d.state[3]) for d in dropout_layers(drop)] == [1, 1]
    for d in dropout_layers(drop):
        kept = R.mask(torch.initial_seed(), d.layer, 0, 0, 0.4, 2, 512)[1]
        assert np.array_equal(d.last.mult.cpu().numpy(), kept)
    # eval: bit-identical to the model without dropout, nothing launched, the counter stays
    for m in (plain, drop):
        m.load_state_dict(zero.state_dict())
        m.eval()
    with torch.no_grad():
        ev_p, kinds_ep = _profiled(ops, lambda: plain(x))
        ev_d, kinds_ed = _profiled(ops, lambda: drop(x))
    assert kinds_ed == kinds_ep and not any("drop" in k for k in kinds_ed)
    assert all(torch.equal(a, b) for a, b in zip(ev_p, ev_d))
    assert [int(d.state[3]) for d in dropout_layers(drop)] == [1, 1]


# ------------------------------------------------------------------------------------------------ hipGraph
def test_graph_replay_draws_what_the_eager_steps_draw(ops):
    import bench
    from miccai2021_cataract_semantic_segmentation_amd.engine import dropout_layers
    from miccai2021_cataract_semantic_segmentation_amd.graph import GraphedTrainStep
    from miccai2021_cataract_semantic_segmentation_amd.losses import TwoScaleLoss
    from miccai2021_cataract_semantic_segmentation_amd.models import OCRNet
    from miccai2021_cataract_semantic_segmentation_amd.optim import FusedAdam
    dev = torch.device("cuda")
    torch.manual_seed(0)
    model = OCRNet(dict(bench.MODELS["ocrnet_r50"][0], dropout=0.3), 3).to(dev).train()
    crit = TwoScaleLoss({"experiment": 3, "interm": {"name": "LovaszSoftmax", "args": [], "weight": 0.4},
                         "final": {"name": "LovaszSoftmax", "args": [], "weight": 1.0}})
    opt = FusedAdam(model, lr=1e-3)
    batches = [bench.synth_batch(2, 64, 96, 25, 300 + i, dev) for i in range(3)]
    layers = dropout_layers(model)
    for d in layers:
        d.reseed(1234)
    fp = model.flat()
    w0 = fp.flat.clone()
    bufs0 = [b.clone() for b in model.buffers()]
    masks = []
    for x, y in batches:
        opt.zero_grad()
        crit(*model(x), y).backward()
        opt.step()
        masks.append([d.last.mult.clone() for d in layers])
    torch.cuda.synchronize()
    w_e = fp.flat.clone()
    assert [int(d.state[3]) for d in layers] == [3, 3]
    assert all(not torch.equal(a, b) for a, b in zip(masks[0], masks[1]))          # the masks of steps 1 and 2 differ
    assert np.array_equal(masks[2][0].cpu().numpy(), R.mask(1234, layers[0].layer, 0, 2, 0.3, 2, 512)[1])
    with torch.no_grad():
        fp.flat.copy_(w0)
        opt._m.zero_()
        opt._v.zero_()
        for b, s in zip(model.buffers(), bufs0):
            b.copy_(s)
    opt._steps = 0
    step = GraphedTrainStep(model, lambda o, l: crit(*o, l), opt, *batches[0])
    torch.cuda.synchronize()
    assert [int(d.state[3]) for d in layers] == [0, 0]                             # warm-up and capture consumed no draw
    for x, y in batches:
        step(x, y)
    torch.cuda.synchronize()
    assert [int(d.state[3]) for d in layers] == [3, 3]
    assert torch.equal(fp.flat, w_e)
    step.release()


# ------------------------------------------------------------------------------------------------ manager
def test_manager_trains_with_dropout(tmp_path):
    from miccai2021_cataract_semantic_segmentation_amd.engine import dropout_layers
    from miccai2021_cataract_semantic_segmentation_amd.managers import OCRNetManager, SyntheticCataractDataset
    cfg = {"name": "t", "mode": "training", "manager": "OCRNet", "log_path": str(tmp_path),
           "graph": {"model": "OCRNet", "backbone": "resnet50", "out_stride": 8, "pretrained": False, "dropout": 0.3},
           "data": {"experiment": 2, "batch_size": 2},
           "loss": {"name": "TwoScaleLoss", "interm": {"name": "LovaszSoftmax", "args": [], "weight": 0.4},
                    "final": {"name": "LovaszSoftmax", "args": [], "weight": 1.0}},
           "train": {"learning_rate": 1e-3, "epochs": 1}, "log_every_n_epochs": 1, "seed": 0}
    tr = SyntheticCataractDataset(4, 64, 96, 17, seed=1)        # two steps
    va = SyntheticCataractDataset(2, 64, 96, 17, seed=2)
    m = OCRNetManager(cfg, tr, va)
    assert m.model.dropout == 0.3
    m.train()
    assert np.isfinite(m.history[0]["train_loss"])
    assert [int(d.state[3]) for d in dropout_layers(m.model)] == [2, 2]
    ck = torch.load(str(m.log_dir / "chkpts" / "chkpt_best.pt"), weights_only=False)
    assert not any(k.endswith(".state") for k in ck["model_state_dict"])               # (the reference's keys: no dropout state)
    inf = OCRNetManager(dict(cfg, mode="inference", load_checkpoint=m.run_id), None, va)
    assert np.isfinite(inf.infer()[0])
