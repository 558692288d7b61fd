"""RandAugment's photometric operations on the device (csrc/augment.hip behind catseg_aug_color_op, op codes 4 ... 8): byte for byte against
the Pillow-generated fixture (tests/golden/randaugment.npz) and against the numpy restatement (tests/_photometric_ref.py, which
tests/test_randaugment_cpu.py holds against Pillow) at the sizes where the kernels take another path; the workspace gate; GpuIngest's and
PinnedFrameLoader's wiring."""
import os
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import _photometric_ref as R  # noqa: E402

G = np.load(os.path.join(HERE, "golden", "randaugment.npz"))
NEW_OPS = ((4, 0.0), (5, 0.0), (6, 3.0), (7, 93.5), (8, 1.45), (8, 0.55))


def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")


def _images():
    """name -> uint8 [H, W, 3]: no interior pixel (1x1, 2x7), one interior pixel (3x3), fewer than 255 pixels (5x4: equalize's step is 0), more
    than one block (37x53), odd row bytes and more pixels than one sweep of the 512-block grid (400x401), all counts in one bin (constant),
    two bins (two-valued)"""
    rng = np.random.default_rng(21)
    out = {"%dx%d" % s: rng.integers(0, 256, s + (3,), dtype=np.uint8) for s in ((1, 1), (2, 7), (3, 3), (5, 4), (37, 53))}
    big = (rng.random((400, 401, 3)) ** 2 * 230 + 11).astype(np.uint8)          # skewed, lo > 0, hi < 255
    big[..., 2] = rng.integers(0, 256, (400, 401), dtype=np.uint8)
    out["400x401"] = big
    out["constant"] = np.full((19, 70, 3), 93, dtype=np.uint8)
    out["two-valued"] = rng.choice(np.array([17, 201], dtype=np.uint8), (33, 35, 3))
    return out


_REF = {}


def _reference(name, img):
    """the restatement's outputs for NEW_OPS, computed once per image"""
    if name not in _REF:
        _REF[name] = [R.apply(img, op, v) for op, v in NEW_OPS]
    return _REF[name]


def test_fixture_matches_byte_for_byte():
    _need_gpu()
    from miccai2021_cataract_semantic_segmentation_amd.utils import GpuAugment
    aug = GpuAugment()
    for name in ("imgs", "tiny"):
        cases = G[name]
        dev = torch.from_numpy(cases[0]).cuda()
        B = dev.shape[0]
        for k, (op, value) in enumerate(zip(G["case_ops"], G["case_values"])):
            out = aug.color_ops(dev, np.full((B, 1), op), np.full((B, 1), value))
            assert np.array_equal(out.cpu().numpy(), cases[k]), (name, str(G["case_names"][k]))
        assert np.array_equal(dev.cpu().numpy(), cases[0])                # the input is not modified
    out = aug.color_ops(torch.from_numpy(G["imgs"][0]).cuda(), G["seq_ops"], G["seq_values"])     # a different op per image and step
    assert np.array_equal(out.cpu().numpy(), G["seq_out"])


@pytest.mark.parametrize("name", ["1x1", "2x7", "3x3", "5x4", "37x53", "400x401", "constant", "two-valued"])
def test_every_new_op_equals_the_restatement(name):
    _need_gpu()
    from miccai2021_cataract_semantic_segmentation_amd.utils import GpuAugment
    img = _images()[name]
    want = _reference(name, img)
    dev = torch.from_numpy(np.stack([img] * len(NEW_OPS))).cuda()
    codes, values = np.array([[o for o, _ in NEW_OPS]]).T, np.array([[v for _, v in NEW_OPS]]).T
    out = GpuAugment().color_ops(dev, codes, values)
    again = GpuAugment().color_ops(dev, codes, values)
    assert torch.equal(out, again)                                        # two launches on the same input are bit-identical
    out = out.cpu().numpy()
    for b, (op, v) in enumerate(NEW_OPS):
        assert np.array_equal(out[b], want[b]), (name, op, v, int((out[b] != want[b]).sum()))
    if name in ("constant", "1x1"):                                       # one bin per band: both table ops are the identity
        assert np.array_equal(want[0], img)
    if name in ("constant", "1x1", "5x4"):                                # fewer than 255 pixels: equalize's step is 0
        assert np.array_equal(want[1], img)
    assert np.array_equal(dev.cpu().numpy()[0], img)


def test_mixed_batch_in_one_launch_and_legacy_bits():
    """B = 5 with codes (-1, 1, 5, 8, 4) in ONE extended launch: every image gets its own operation, contrast gives the legacy call's bits,
    the input tensor stays as it is"""
    _need_gpu()
    from oracle import augment as A
    from miccai2021_cataract_semantic_segmentation_amd import ops
    from miccai2021_cataract_semantic_segmentation_amd.utils import GpuAugment
    rng = np.random.default_rng(5)
    imgs = (rng.random((5, 37, 53, 3)) ** 2 * 255).astype(np.uint8)
    codes, values = np.array([-1, 1, 5, 8, 4]), np.array([0.0, 1.31, 0.0, 1.9, 0.0])
    dev = torch.from_numpy(imgs).cuda()
    out = GpuAugment().color_ops(dev, codes[:, None], values[:, None]).cpu().numpy()
    assert np.array_equal(dev.cpu().numpy(), imgs)
    for b in range(5):
        assert np.array_equal(out[b], R.apply(imgs[b], int(codes[b]), float(values[b]))), b
    legacy = torch.from_numpy(imgs).cuda()
    ops.aug_color_op(legacy, torch.full((5,), 1, dtype=torch.int32, device="cuda"), torch.full((5,), 1.31, dtype=torch.float32, device="cuda"))
    assert np.array_equal(out[1], legacy[1].cpu().numpy()) and np.array_equal(out[1], A.adjust(imgs[1], 1, float(np.float32(1.31))))
    # every legacy code through the extended pipeline: the legacy call's bits
    for op, f in ((0, 1.37), (1, 2 / 3), (2, 1.4), (3, 13.0)):
        o, fac = torch.full((5,), op, dtype=torch.int32, device="cuda"), torch.full((5,), f, dtype=torch.float32, device="cuda")
        a, b = torch.from_numpy(imgs).cuda(), torch.from_numpy(imgs).cuda()
        ops.aug_color_op(a, o, fac)
        ops.aug_color_op(b, o, fac, extended="full")
        assert torch.equal(a, b), op
    # codes outside -1 ... 8 leave the image unchanged in the extended pipeline
    c = torch.from_numpy(imgs).cuda()
    ops.aug_color_op(c, torch.tensor([9, -3, 100, 9, -1], dtype=torch.int32, device="cuda"), torch.ones(5, device="cuda"), extended="full")
    assert np.array_equal(c.cpu().numpy(), imgs)


def test_workspace_gate_and_guard_bytes():
    """the workspace size selects the pipeline: with the "lut" size a sharpness image stays unchanged (the others are served), with the "full"
    size it is served; no byte at or behind workspace_bytes is written"""
    _need_gpu()
    from miccai2021_cataract_semantic_segmentation_amd import _lib, ops
    rng = np.random.default_rng(8)
    B, H, W = 3, 21, 38
    imgs = rng.integers(0, 256, (B, H, W, 3), dtype=np.uint8)
    op = torch.tensor([8, 5, 8], dtype=torch.int32, device="cuda")
    fac = torch.tensor([1.45, 0.0, 0.3], dtype=torch.float32, device="cuda")
    lut_b, full_b = ops.aug_color_workspace_bytes(B, H, W, "lut"), ops.aug_color_workspace_bytes(B, H, W, "full")
    assert 8 * B + 256 < lut_b < full_b == lut_b + 3 * B * H * W
    want = {lut_b: [imgs[0], R.equalize(imgs[1]), imgs[2]], full_b: [R.sharpness(imgs[0], 1.45), R.equalize(imgs[1]), R.sharpness(imgs[2], 0.3)],
            full_b - 1: [imgs[0], R.equalize(imgs[1]), imgs[2]]}
    for nbytes, expect in want.items():
        ws = torch.full((full_b + 4096,), 0xA5, dtype=torch.uint8, device="cuda")
        dev = torch.from_numpy(imgs).cuda()
        _lib.check(_lib.lib.catseg_aug_color_op(dev.data_ptr(), B, H, W, op.data_ptr(), fac.data_ptr(), ws.data_ptr(), nbytes, _lib.stream()))
        torch.cuda.synchronize()
        assert bool((ws[nbytes:] == 0xA5).all()), nbytes                  # nothing behind the size handed over
        if nbytes < full_b:
            assert bool((ws[lut_b:] == 0xA5).all()), nbytes               # and no partial source copy
        for b in range(B):
            assert np.array_equal(dev[b].cpu().numpy(), expect[b]), (nbytes, b)


def _compose(img, flips, pad, codes, values):
    ref = img
    if flips & 2:
        ref = ref[::-1]
    if flips & 1:
        ref = ref[:, ::-1]
    if pad:
        ref = np.pad(ref, ((pad, pad), (0, 0), (0, 0)), mode="reflect")
    ref = np.ascontiguousarray(ref)
    for op, v in zip(codes, values):
        ref = R.apply(ref, int(op), float(v))
    return ref


def test_ingest_photometric_equals_the_hand_composition():
    _need_gpu()
    from miccai2021_cataract_semantic_segmentation_amd import ops
    from miccai2021_cataract_semantic_segmentation_amd.utils import GpuAugment, GpuIngest
    rng = np.random.default_rng(13)
    B, H, W = 4, 30, 44
    img = rng.integers(0, 256, (B, H, W, 3), dtype=np.uint8)
    lbl = rng.integers(0, 36, (B, H, W), dtype=np.uint8)
    flips = np.array([0, 1, 2, 3], dtype=np.int32)
    codes = np.array([[8, 4], [5, 1], [-1, 7], [6, 8]])
    values = np.array([[1.27, 0.0], [0.0, 0.73], [0.0, 178.5], [7.0, 0.73]])
    ing = GpuIngest(3, pad=(2, 2))
    x, labels = ing(torch.from_numpy(img), torch.from_numpy(lbl), flips, photometric=(codes, values))
    x_plain, labels_plain = ing(torch.from_numpy(img), torch.from_numpy(lbl), flips)
    assert torch.equal(labels, labels_plain) and not torch.equal(x, x_plain)
    for b in range(B):
        want = torch.from_numpy(_compose(img[b], int(flips[b]), 2, codes[b], values[b])).permute(2, 0, 1).float() / 255.0
        assert torch.equal(x[b].cpu(), want), b
    # a list of pairs, after a jitter: pad / flip + color_jitter + color_ops + ingest composed by hand on the device
    aug = GpuAugment()
    orders, factors = np.array([[0, 1, 2, 3]] * B), np.array([[1.2, 0.8, 1.1, 0.03]] * B)
    x2, _ = ing(torch.from_numpy(img), torch.from_numpy(lbl), flips, jitter=(orders, factors), photometric=[(codes, values), (codes[:, :1], values[:, :1])])
    u8 = ops.aug_pad_flip_u8(torch.from_numpy(img).cuda(), torch.from_numpy(flips).cuda(), 2, 2)
    u8 = aug.color_ops(aug.color_ops(aug.color_jitter(u8, orders, factors), codes, values), codes[:, :1], values[:, :1])
    assert torch.equal(x2, ops.ingest_u8(u8, None, ing.lut, None, 0, 0, None, None)[0])
    # through the warp launch, with a crop: the uint8 window, then the same operations
    origins, px = np.array([[3, 5], [0, 0], [10, 20], [6, 1]], dtype=np.int32), 20
    x3, l3 = ing(torch.from_numpy(img), torch.from_numpy(lbl), flips, crop=(origins, px), photometric=(codes, values))
    _, l3_plain = ing(torch.from_numpy(img), torch.from_numpy(lbl), flips, crop=(origins, px))
    assert torch.equal(l3, l3_plain) and x3.shape == (B, 3, px, px)
    for b in range(B):
        flipped = _compose(img[b], int(flips[b]), 0, [], [])
        v, h = origins[b]
        window = np.ascontiguousarray(flipped[v:v + px, h:h + px])
        want = torch.from_numpy(_compose(window, 0, 0, codes[b], values[b])).permute(2, 0, 1).float() / 255.0
        assert torch.equal(x3[b].cpu(), want), b


class _EpochFrames:
    """deterministic uint8 frames (module level: the forked worker processes inherit it)"""

    def __len__(self):
        return 8

    def __getitem__(self, i):
        rng = np.random.RandomState(300 + i)
        return rng.randint(0, 256, (28, 40, 3)).astype(np.uint8), rng.randint(0, 36, (28, 40)).astype(np.uint8)


@pytest.mark.parametrize("mode", [dict(workers=1), dict(worker_processes=2)])
def test_loader_epoch_equals_a_host_replay_of_the_draws(mode):
    _need_gpu()
    from miccai2021_cataract_semantic_segmentation_amd.utils import GpuIngest, PinnedFrameLoader, sample_color_jitter, sample_randaugment
    from miccai2021_cataract_semantic_segmentation_amd.utils.ingest import sample_flips
    ds = _EpochFrames()
    loader = PinnedFrameLoader(ds, batch_size=4, experiment=3, seed=6, shuffle=False, colorjitter=True, randaugment=True, **mode)
    try:
        out = [(x.clone(), l.clone()) for x, l in loader]
    finally:
        loader.close()
    assert len(out) == 2
    rng = np.random.RandomState(6 * 1000003 + 1)
    gen = torch.Generator().manual_seed(6 * 1000003 + 1)
    flips = [sample_flips(4, (0.0, 0.5), rng) for _ in range(2)]
    jit = [sample_color_jitter(4, generator=gen) for _ in range(2)]
    photo = [sample_randaugment(4, generator=gen) for _ in range(2)]            # after ALL jitter draws of the epoch
    assert any((c >= 4).any() for c, _ in photo)                                 # (the seed draws some of the new operations)
    ing = GpuIngest(3)
    for bi, (x, labels) in enumerate(out):
        img = torch.from_numpy(np.stack([ds[i][0] for i in range(bi * 4, bi * 4 + 4)]))
        lbl = torch.from_numpy(np.stack([ds[i][1] for i in range(bi * 4, bi * 4 + 4)]))
        xr, lr = ing(img, lbl, flips[bi], jitter=jit[bi], photometric=photo[bi])
        assert torch.equal(x, xr) and torch.equal(labels, lr), (mode, bi)
        x_jit, _ = ing(img, lbl, flips[bi], jitter=jit[bi])
        assert not torch.equal(x, x_jit), (mode, bi)                            # the operations did something
