"""RandAugment's photometric operations, host side: the numpy restatement (tests/_photometric_ref.py) against Pillow itself and against the
Pillow-generated fixture (tests/golden/randaugment.npz); the magnitude tables and draws of utils/augment.py as known answers; the refusals of
the 'randaugment' config; the loader's draw order; and the C ABI, which this feature leaves as it was."""
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import _photometric_ref as R  # noqa: E402

G = np.load(os.path.join(HERE, "golden", "randaugment.npz"))


def _random_images(n, seed):
    """the three kinds: uniform, x^4-skewed, drawn from {0, 1, 127, 128, 254, 255}; sizes 1 ... 47 (so: with and without interior pixels,
    below and above 255 pixels)"""
    rng = np.random.default_rng(seed)
    for t in range(n):
        H, W = int(rng.integers(1, 48)), int(rng.integers(1, 48))
        if t % 3 == 0:
            yield rng.integers(0, 256, (H, W, 3), dtype=np.uint8)
        elif t % 3 == 1:
            yield (rng.random((H, W, 3)) ** 4 * 255).astype(np.uint8)
        else:
            yield rng.choice(np.array([0, 1, 127, 128, 254, 255], dtype=np.uint8), (H, W, 3))


def test_restatement_equals_the_pillow_fixture():
    for name in ("imgs", "tiny"):
        cases = G[name]
        for k, (op, value) in enumerate(zip(G["case_ops"], G["case_values"])):
            for b in range(cases.shape[1]):
                assert np.array_equal(R.apply(cases[0, b], int(op), float(value)), cases[k, b]), (name, str(G["case_names"][k]), b)
    for b, (ops, values) in enumerate(zip(G["seq_ops"], G["seq_values"])):
        a = G["imgs"][0, b]
        for op, v in zip(ops, values):
            a = R.apply(a, int(op), float(v))
        assert np.array_equal(a, G["seq_out"][b]), b
    assert os.path.getsize(os.path.join(HERE, "golden", "randaugment.npz")) < 300 * 1024


def test_restatement_equals_pillow_on_random_images():
    pytest.importorskip("PIL")
    from PIL import Image, ImageEnhance, ImageOps
    rng = np.random.default_rng(2)
    n = 0
    for a in _random_images(330, 1):
        im = Image.fromarray(a)
        assert np.array_equal(np.asarray(ImageOps.autocontrast(im)), R.autocontrast(a))
        assert np.array_equal(np.asarray(ImageOps.equalize(im)), R.equalize(a))
        bits, t, f = int(rng.integers(1, 9)), float(rng.choice([0, 0.5, 93.5, 128, 178.5, 255, 256])), float(rng.uniform(0.1, 1.9))
        assert np.array_equal(np.asarray(ImageOps.posterize(im, bits)), R.posterize(a, bits))
        assert np.array_equal(np.asarray(ImageOps.solarize(im, t)), R.solarize(a, t))
        assert np.array_equal(np.asarray(ImageEnhance.Sharpness(im).enhance(f)), R.sharpness(a, f)), (a.shape, f)
        n += 1
    assert n >= 300
    big = rng.integers(0, 256, (300, 700, 3), dtype=np.uint8)          # equalize with a step far above 1
    assert np.array_equal(np.asarray(ImageOps.equalize(Image.fromarray(big))), R.equalize(big))
    assert np.array_equal(np.asarray(ImageEnhance.Sharpness(Image.fromarray(big)).enhance(1.45)), R.sharpness(big, 1.45))


def test_space_table_known_answers():
    from miccai2021_cataract_semantic_segmentation_amd.utils import augment as A
    assert (A.AUTOCONTRAST, A.EQUALIZE, A.POSTERIZE, A.SOLARIZE, A.SHARPNESS) == (4, 5, 6, 7, 8)
    space = A.randaugment_space()
    assert [(n, c, s) for n, c, _, s in space] == [
        ("Identity", -1, False), ("Brightness", 0, True), ("Color", 2, True), ("Contrast", 1, True), ("Sharpness", 8, True),
        ("Posterize", 6, False), ("Solarize", 7, False), ("AutoContrast", 4, False), ("Equalize", 5, False)]
    by_name = {n: m for n, _, m, _ in space}
    assert all(by_name[n] is None for n in ("Identity", "AutoContrast", "Equalize"))
    assert all(len(by_name[n]) == 31 for n in ("Brightness", "Color", "Contrast", "Sharpness", "Posterize", "Solarize"))
    for n in ("Brightness", "Color", "Contrast", "Sharpness"):
        assert abs(by_name[n][9] - 0.27) < 1e-7           # (a float32 linspace, as torchvision's)
        assert by_name[n][0] == 0.0 and abs(by_name[n][30] - 0.9) < 1e-7
    assert by_name["Posterize"][9] == 7 and by_name["Solarize"][9] == 178.5
    assert by_name["Posterize"].tolist() == [8 - int(np.round(i / 7.5)) for i in range(31)] and by_name["Posterize"][30] == 4
    assert by_name["Solarize"][0] == 255.0 and by_name["Solarize"][30] == 0.0
    assert len(A.randaugment_space(11)[1][2]) == 11


def test_sample_randaugment_known_answers_and_draw_order():
    from miccai2021_cataract_semantic_segmentation_amd.utils.augment import randaugment_space, sample_randaugment
    m9 = float(torch.linspace(0.0, 0.9, 31)[9])          # 0.27 as the float32 table holds it
    lo, hi = 1.0 - m9, 1.0 + m9
    known = {0: ([[5, -1], [2, 4], [7, 4], [0, -1]], [[0, 0], [hi, 0], [178.5, 0], [lo, 0]]),
             7: ([[-1, 8], [2, 7], [5, 6], [8, 4]], [[0, lo], [lo, 178.5], [0, 7], [lo, 0]])}
    for seed, (codes, values) in known.items():
        o, v = sample_randaugment(4, generator=torch.Generator().manual_seed(seed))
        assert o.dtype == np.int32 and v.dtype == np.float64 and o.shape == v.shape == (4, 2)
        assert o.tolist() == codes and v.tolist() == values, seed
    # the draws by hand: one randint(9) per slot, one randint(2) only behind a signed entry; the generators end in the same state
    space = randaugment_space()
    for seed in (3, 11):
        g, h = torch.Generator().manual_seed(seed), torch.Generator().manual_seed(seed)
        o, v = sample_randaugment(6, num_ops=3, magnitude=30, generator=g)
        for i in range(6):
            for k in range(3):
                _, code, mags, signed = space[int(torch.randint(9, (1,), generator=h))]
                want = float(mags[30]) if mags is not None else 0.0
                if signed:
                    want = 1.0 - want if int(torch.randint(2, (1,), generator=h)) else 1.0 + want
                assert (o[i, k], v[i, k]) == (code, want)
        assert int(torch.randint(1000, (1,), generator=g)) == int(torch.randint(1000, (1,), generator=h))
    o, v = sample_randaugment(16, generator=torch.Generator().manual_seed(1), apply_probability=0.0)
    assert (o == -1).all() and (v == 0).all()
    o1, _ = sample_randaugment(16, generator=torch.Generator().manual_seed(1), apply_probability=1.0)
    g = torch.Generator().manual_seed(1)
    picks = []
    for _ in range(16):                       # p = 1: the frame's uniform is drawn first, then nothing is skipped
        torch.rand(1, generator=g)
        for _ in range(2):
            picks.append(int(torch.randint(9, (1,), generator=g)))
            if 1 <= picks[-1] <= 4:
                torch.randint(2, (1,), generator=g)
    assert o1.ravel().tolist() == [space[p][1] for p in picks]
    assert sorted(set(o1.ravel().tolist()) - {-1})          # (some operation is drawn; Identity's own code is -1 too)


def test_randaugment_from_transforms_and_its_refusals():
    from miccai2021_cataract_semantic_segmentation_amd.utils.augment import randaugment_from_transforms
    assert randaugment_from_transforms(["pad", "flip"], {"randaugment": {"num_ops": 3}}) is None
    assert randaugment_from_transforms(["randaugment"], None) == {"num_ops": 2, "magnitude": 9, "bins": 31, "p": None, "frames": "all"}
    got = randaugment_from_transforms(["pad", "randaugment"], {"randaugment": {"num_ops": 3, "magnitude": 4, "bins": 11, "p": 0.5, "frames": "pseudo"}})
    assert got == {"num_ops": 3, "magnitude": 4, "bins": 11, "p": 0.5, "frames": "pseudo"}
    for bad, quoted in (({"strength": 2}, "strength"), ({"magnitude": 31}, "31"), ({"magnitude": -1}, "-1"), ({"magnitude": 5, "bins": 5}, "5"),
                        ({"num_ops": 0}, "0"), ({"p": 1.5}, "1.5"), ({"p": -0.1}, "-0.1"), ({"frames": "labelled"}, "'labelled'"),
                        ({"frames": None}, "None")):
        with pytest.raises(ValueError, match=quoted):
            randaugment_from_transforms(["randaugment"], {"randaugment": bad})


class _Frames:
    def __init__(self, n):
        self.n = n

    def __len__(self):
        return self.n

    def __getitem__(self, i):
        raise AssertionError("the draws need no frame")


def test_loader_draws_are_unchanged_without_randaugment_and_follow_the_jitters():
    from miccai2021_cataract_semantic_segmentation_amd.utils import BalancedConcatDataset
    from miccai2021_cataract_semantic_segmentation_amd.utils.augment import PSEUDO_JITTER_PROBABILITY, pseudo_jitter_ranges, sample_color_jitter, sample_randaugment
    from miccai2021_cataract_semantic_segmentation_amd.utils.loader import PinnedFrameLoader
    paired = BalancedConcatDataset(_Frames(5), _Frames(6))
    kw = dict(batch_size=4, experiment=2, seed=3, labels_remapped=(False, True), blur=True, colorjitter=True, pseudo_colorjitter=2, device="cpu")
    batches = [[(0, i), (0, i + 1), (1, i), (1, i + 1)] for i in (0, 2, 4)]

    def draws(**extra):
        loader = PinnedFrameLoader(paired, **dict(kw, **extra))
        loader.epoch = 2
        return loader._draws(batches)

    base, none, ra = draws(), draws(randaugment=None), draws(randaugment={"frames": "pseudo", "num_ops": 3})
    assert base[4] is None and none[4] is None and len(ra[4]) == 3
    for other in (none, ra):                  # flips, blurs and jitters: the same sequence with and without the argument
        for a, b in zip(base[1:4], other[1:4]):
            assert repr(a) == repr(b)
        a, b = base[0].get_state(), other[0].get_state()                    # (the numpy stream the geometry continues)
        assert np.array_equal(a[1], b[1]) and a[2:] == b[2:]
    # the randaugment draws continue the epoch's torch generator after ALL jitter draws
    gen = torch.Generator().manual_seed(3 * 1000003 + 2)
    for _ in batches:
        sample_color_jitter(4, generator=gen)
    for _ in batches:
        sample_color_jitter(4, generator=gen, apply_probability=PSEUDO_JITTER_PROBABILITY, **pseudo_jitter_ranges(2))
    drew = False
    for codes, values in ra[4]:
        want_c, want_v = sample_randaugment(4, 3, 9, 31, generator=gen)
        assert (codes[:2] == -1).all() and (values[:2] == 0).all()        # frames "pseudo": the labelled rows carry -1
        assert np.array_equal(codes[2:], want_c[2:]) and np.array_equal(values[2:], want_v[2:])
        drew = drew or (codes[2:] >= 0).any()
    assert drew
    every = draws(randaugment=True)[4]
    assert any((c[:2] >= 0).any() for c, _ in every) and every[0][0].shape == (4, 2)
    with pytest.raises(ValueError, match="'pseudo'"):
        PinnedFrameLoader(_Frames(8), batch_size=4, experiment=2, randaugment={"frames": "pseudo"}, device="cpu")
    with pytest.raises(ValueError, match="unknown keys"):
        PinnedFrameLoader(_Frames(8), batch_size=4, experiment=2, randaugment={"ops": 2}, device="cpu")


def test_workspace_sizes_mirror_the_header():
    """ops.aug_color_workspace_bytes against the header's formulas (the one-line #defines, evaluated as arithmetic)"""
    import re
    sys.path.insert(0, os.path.dirname(HERE))
    text = open(os.path.join(os.path.dirname(HERE), "include", "catseg.h")).read()
    lut = re.search(r"^#define CATSEG_AUG_WS_LUT\(B\) (.*)$", text, flags=re.M).group(1)
    full = re.search(r"^#define CATSEG_AUG_WS_FULL\(B, H, W\) (.*)$", text, flags=re.M).group(1)

    def c_eval(expr, **names):
        return eval(expr.replace("(size_t)", "").replace("/", "//"), dict(names, CATSEG_AUG_WS_LUT=lambda B: c_eval(lut, B=B)))

    src = open(os.path.join(os.path.dirname(HERE), "miccai2021_cataract_semantic_segmentation_amd", "ops.py")).read()
    ns = {}
    exec(src[src.index("def aug_color_workspace_bytes"):src.index("def aug_color_op")], ns)        # (importing ops needs the built library)
    size = ns["aug_color_workspace_bytes"]
    for B, H, W in ((1, 1, 1), (5, 37, 53), (8, 544, 960), (33, 3, 3)):
        assert size(B, H, W) == 8 * B + 256 < size(B, H, W, "lut") == c_eval(lut, B=B) < size(B, H, W, "full") == c_eval(full, B=B, H=H, W=W)
        assert c_eval(lut, B=B) % 256 == 0
    with pytest.raises(ValueError, match="'both'"):
        size(1, 1, 1, "both")


def test_abi_surface_is_unchanged():
    import _abi
    assert len(_abi.prototypes()) == 197
