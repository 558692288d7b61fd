"""The label census kernel and the per-batch IoU average (csrc/census.hip) on the device: the census exactly against np.bincount over
misaligned frames, tails, a shifted base pointer, a table, the "other" bin, uniform frames, blobs, 64-bit accumulation; iou_ema bit for bit
against the REAL reference's t_get_mean_iou(..., calculate_mean=False) and update sequences (tests/golden/class_loaders.npz)."""
import functools
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPES = [(3, 5, 7), (1, 1, 1), (2, 17, 33), (2, 64, 64), (2, 540, 960)]      # (3, 5, 7): frame starts 35 bytes apart, tails everywhere


def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")


def _want(frames, nbins, lut=None):
    """np.bincount per frame, values >= nbins folded into the last column"""
    out = np.zeros((len(frames), nbins + 1), dtype=np.int64)
    for b, f in enumerate(frames):
        v = f.reshape(-1).astype(np.int64)
        if lut is not None:
            v = lut.astype(np.int64)[v]
        out[b] = np.bincount(np.minimum(v, nbins), minlength=nbins + 1)
    return out


@functools.lru_cache(maxsize=None)
def _maps(shape, kind):
    B, H, W = shape
    rng = np.random.RandomState(B * 1000003 + H * 1009 + W + 7919 * len(kind))
    if kind == "noise":                                   # every byte value: with nbins 36 the "other" column fills
        return rng.randint(0, 256, (B, H, W)).astype(np.uint8)
    if kind == "blobs":                                   # patches 16 wide, 12 high
        small = rng.randint(0, 36, (B, (H + 11) // 12, (W + 15) // 16)).astype(np.uint8)
        return np.ascontiguousarray(small.repeat(12, 1).repeat(16, 2)[:, :H, :W])
    if kind == "single":                                  # one bin takes every pixel
        return np.full((B, H, W), 6, dtype=np.uint8)
    raise KeyError(kind)


def _lut():
    return (np.random.RandomState(3).randint(0, 45, 256)).astype(np.uint8)      # some values land past 36 bins


@pytest.mark.parametrize("shape", SHAPES, ids=["%dx%dx%d" % s for s in SHAPES])
@pytest.mark.parametrize("kind", ["noise", "blobs", "single"])
def test_census_equals_bincount(shape, kind):
    _need_gpu()
    from miccai2021_cataract_semantic_segmentation_amd import ops
    frames = _maps(shape, kind)
    B, H, W = shape
    lut = _lut()
    lut_d = torch.from_numpy(lut).cuda()
    flat = torch.zeros(frames.size + 1, dtype=torch.uint8, device="cuda")
    flat[1:] = torch.from_numpy(frames).cuda().reshape(-1)
    shifted = flat[1:].view(B, H, W)                      # the base pointer one byte past an aligned address
    assert shifted.data_ptr() % 16 == 1 and shifted.is_contiguous()
    aligned = torch.from_numpy(frames).cuda()
    for nbins in (36, 256, 1):
        for table, table_d in ((None, None), (lut, lut_d)):
            want = _want(frames, nbins, table)
            assert (want.sum(1) == H * W).all()
            for lbl in (aligned, shifted):
                got = ops.label_census(lbl, nbins, table_d)
                again = ops.label_census(lbl, nbins, table_d)
                assert got.dtype == torch.int64 and tuple(got.shape) == (B, nbins + 1)
                assert np.array_equal(got.cpu().numpy(), want), (shape, kind, nbins, table is not None, lbl is shifted)
                assert torch.equal(got, again)            # two launches: the same bits
    if kind == "noise":
        assert _want(frames, 36)[:, 36].sum() > 0 or frames.size < 8


def test_census_accumulates_in_64_bits():
    """counts above 2^32 and just below it: the addition needs the carry into the upper word"""
    _need_gpu()
    from miccai2021_cataract_semantic_segmentation_amd import ops
    frames = _maps((2, 540, 960), "blobs")
    lbl = torch.from_numpy(frames).cuda()
    want = _want(frames, 36)
    start = np.zeros_like(want)
    start[0, :] = 2 ** 32 - 1
    start[1, :] = 2 ** 33 + 7
    out = torch.from_numpy(start.copy()).cuda()
    ops.label_census(lbl, 36, out=out, accumulate=True)
    ops.label_census(lbl, 36, out=out, accumulate=True)
    assert np.array_equal(out.cpu().numpy(), start + 2 * want)
    assert (out.cpu().numpy()[0] >> 32).max() == 1 and want[0].max() > 0
    ops.label_census(lbl, 36, out=out)                    # accumulate = 0 overwrites
    assert np.array_equal(out.cpu().numpy(), want)
    with pytest.raises(ValueError, match="needs out="):
        ops.label_census(lbl, 36, accumulate=True)


class _Frames:
    """a dataset whose item [1] is the uint8 label map"""

    def __init__(self, maps):
        self.maps = maps

    def __len__(self):
        return len(self.maps)

    def __getitem__(self, i):
        return None, self.maps[i], {"index": i}


def test_utils_label_census_in_chunks():
    _need_gpu()
    from miccai2021_cataract_semantic_segmentation_amd import utils
    rng = np.random.RandomState(5)
    maps = rng.randint(0, 36, (9, 17, 33)).astype(np.uint8)
    want = _want(maps, 36)[:, :36]
    for source in (list(maps), maps, _Frames(maps), [maps[:5], torch.from_numpy(maps[5:])], (m for m in maps)):
        got = utils.label_census(source, chunk=4)
        assert got.dtype == np.int64 and got.shape == (9, 36) and np.array_equal(got, want)
    # frames of two sizes: a chunk ends where the shape changes
    other = rng.randint(0, 36, (2, 8, 8)).astype(np.uint8)
    got = utils.label_census(list(maps[:3]) + list(other) + list(maps[3:5]), chunk=4)
    assert np.array_equal(got, np.concatenate([want[:3], _want(other, 36)[:, :36], want[3:5]]))
    # a table; and the reference's "Unknown class found"
    lut = np.arange(256, dtype=np.uint8) // 2
    assert np.array_equal(utils.label_census(maps, nbins=18, lut=lut, chunk=4), _want(maps, 18, lut)[:, :18])
    bad = maps.copy()
    bad[4, 2, 3] = 200
    with pytest.raises(ValueError, match="Unknown class found"):
        utils.label_census(bad, chunk=4)
    got = utils.label_census(bad, chunk=4, allow_other=True)
    assert got.shape == (9, 36) and got[4].sum() == 17 * 33 - 1
    with pytest.raises(ValueError, match="uint8"):
        utils.label_census([maps.astype(np.int64)])
    assert utils.label_census([]).shape == (0, 36)
    # the helpers feed the existing sampler and crop_mode 'freq'
    assert np.array_equal(utils.class_sums_of(want), np.bincount(maps.reshape(-1), minlength=36))
    assert utils.class_info(want, 2).shape == (9, 17) and utils.class_info(want, 1).sum() == maps.size


EINVAL = 1
A = [0x10000 * (i + 1) for i in range(4)]     # fake device pointers: a refusal returns before anything is launched


@pytest.mark.parametrize("fields,message", [(dict(B=0), b"bad dims"), (dict(nbins=300), b"nbins"), (dict(lbl=None), b"label map is NULL"),
                                            (dict(counts=None), b"counts is NULL"), (dict(counts=A[1] + 4), b"8-byte aligned")])
def test_census_refuses_before_a_launch(fields, message):
    _need_gpu()
    from miccai2021_cataract_semantic_segmentation_amd import _lib
    f = dict(lbl=A[0], B=2, H=5, W=7, lut=None, nbins=36, counts=A[1], accumulate=0, stream=None)
    f.update(fields)
    rc = _lib.lib.catseg_label_census_u8(*f.values())
    assert rc == EINVAL and message in _lib.lib.catseg_last_error()
    torch.cuda.synchronize()                              # nothing was launched on the fake pointers


# ---- iou_ema against fixture (c)
@functools.lru_cache(maxsize=None)
def _fixture():
    return np.load(os.path.join(ROOT, "tests", "golden", "class_loaders.npz"))


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


@pytest.mark.parametrize("K", [8, 17, 25])
@pytest.mark.parametrize("a,name", [(1, "1"), (0.3, "03"), (0, "0")])
@pytest.mark.parametrize("with_batch", [False, True], ids=["iou_batch NULL", "iou_batch given"])
def test_iou_ema_bit_for_bit(K, a, name, with_batch):
    _need_gpu()
    from miccai2021_cataract_semantic_segmentation_amd import ops
    g = _fixture()
    cms = g["k%d_cms" % K]
    running = torch.zeros((K, K), dtype=torch.int32, device="cuda")
    prev = torch.zeros_like(running)
    values = torch.full((K,), 0.5, dtype=torch.float32, device="cuda")
    batch = torch.full((K,), -1.0, dtype=torch.float32, device="cuda") if with_batch else None
    assert len(cms) >= 3
    for t in range(len(cms)):                             # consecutive steps on ONE running matrix
        running += torch.from_numpy(cms[t]).cuda()
        ops.iou_ema(running, prev, values, a, iou_batch=batch)
        assert torch.equal(prev, running)
        assert np.array_equal(_bits(values.cpu().numpy()), _bits(g["k%d_ema_a%s" % (K, name)][t])), (K, a, t)
        if with_batch:
            assert np.array_equal(_bits(batch.cpu().numpy()), _bits(g["k%d_cm_iou" % K][t])), (K, t)
