"""Fixtures of CropNP(crop_mode='freq') from the REAL reference (utils/transforms.py:254-303), see make_golden.py: per case the offsets and
window edge its __call__ reported, the next random.random() after the call (pins how many draws it consumed) and the distance of the
consumed uniform to the nearest cumulative fraction of the reference's own float64 accumulate.  Experiments 1 and 2 (CropNP.__init__
raises a KeyError for experiment 3).  The integer pick of the device equals the reference's outside a band of 2^-22 around the cumulative
fractions; this maker ASSERTS that every stored case lies outside it.

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_cropfreq.py
"""
import itertools
import os
import random
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
import ref_harness  # noqa: E402

R = ref_harness.load()
from utils import CLASS_SUMS                      # noqa: E402  (the reference's utils package)
from utils.transforms import CropNP               # noqa: E402

BAND = 2.0 ** -22
SIZE = 0.4
FRAMES = ((96, 160, 4), (80, 72, 4), (192, 320, 3))        # h, w, seeds per map (80 x 72: W < H, numpy clips the column slice)
EXPERIMENTS = (1, 2)


def label_map(kind, h, w, k, seed):
    rng = np.random.RandomState(seed)
    if kind == "random":
        return rng.randint(0, k, (h, w)).astype(np.uint8)
    coarse = rng.randint(0, k, ((h + 15) // 16, (w + 11) // 12))          # blobs of 16 x 12 pixels
    return np.kron(coarse, np.ones((16, 12), dtype=np.int64))[:h, :w].astype(np.uint8)


out = {"class_sums": np.array(CLASS_SUMS, dtype=np.int64), "band": np.array(BAND), "size": np.array(SIZE)}
cases, maps = [], []
for exp in EXPERIMENTS:
    crop = CropNP(SIZE, "freq", exp)
    out["class_frequencies_e%d" % exp] = crop.class_frequencies
    assert crop.class_frequencies.dtype == np.float32
    for (h, w, nseeds), kind in itertools.product(FRAMES, ("blob", "random")):
        mi = len(maps)
        lbl = label_map(kind, h, w, crop.num_classes, 1000 * exp + h + len(kind))
        maps.append(lbl)
        img = np.zeros((h, w, 3), dtype=np.uint8)
        for s in range(nseeds):
            seed = 7919 * mi + 13 * s + exp
            random.seed(seed)
            u = random.random()                    # what random.choices(k=1) will consume
            random.seed(seed)
            ic, lc, meta = crop((img, lbl.astype(np.int64), {}))
            after = random.random()
            # the reference's own weights and accumulate (random.choices: bisect(cum, u * total, 0, n - 1))
            px, margin = meta["crop_size"], meta["crop_size"] // 2
            probs = 1 / crop.class_frequencies[lbl.astype(np.int64)][margin:h - margin, margin:h - margin]
            probs /= np.sum(probs)
            cum = np.array(list(itertools.accumulate(probs.flatten().tolist())))
            dist = float(np.min(np.abs(u - cum / cum[-1])))
            assert dist > BAND, "case (exp %d, %d x %d, %s, seed %d) lies in the band: %g -- pick another seed" % (exp, h, w, kind, seed, dist)
            v, hh = meta["crop_offsets"]
            assert v * probs.shape[1] + hh == min(int(np.searchsorted(cum, u * cum[-1], side="right")), probs.size - 1)
            cases.append([exp, mi, seed, px, v, hh])
            out.setdefault("next_random", []).append(after)
            out.setdefault("u", []).append(u)
            out.setdefault("distance", []).append(dist)
            print("exp %d %3d x %3d %-6s seed %6d px %3d offsets %3d %3d  distance %.3g" % (exp, h, w, kind, seed, px, v, hh, dist))
out["cases"] = np.array(cases, dtype=np.int64)                 # experiment, map index, seed, crop_size, crop_offsets (v, h)
for k in ("next_random", "u", "distance"):
    out[k] = np.array(out[k], dtype=np.float64)
for mi, m in enumerate(maps):
    out["map%d" % mi] = m
path = os.path.join(HERE, "cropfreq.npz")
np.savez_compressed(path, **out)
print("wrote cropfreq.npz: %d cases, %.1f KB, closest distance %.3g" % (len(cases), os.path.getsize(path) / 1024, out["distance"].min()))
