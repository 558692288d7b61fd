"""Exact integer restatement of the reference's CropNP(crop_mode='freq') pick (utils/transforms.py:282-293), in plain numpy / Python ints:
what csrc/cropfreq.hip computes, and -- outside a band of 2^-22 around the cumulative fractions -- what the reference's float64
random.choices picks (tests/golden/cropfreq.npz holds the reference's own offsets).

    region   lbl[margin:h - margin, margin:h - margin], margin = px // 2 (the columns sliced with the HEIGHT, clipped at w by numpy)
    weights  wq[label]: the float32 1 / f_c scaled to integers by a power of two
    T        (m * total) >> 53 with m = int(u * 2^53); the pick is the first i with cum_i > T, capped at n - 1 (bisect_right, hi = n - 1)
    origin   (i // region_w, i % region_w)
"""
from fractions import Fraction

import numpy as np


def region(h, w, px):
    margin = px // 2
    return margin, h - 2 * margin, min(h - margin, w) - margin


def weights_of(freqs):
    """(wq, s) from the float32 class frequencies, independently of utils.geometry.freq_weight_table: numerators over the common denominator"""
    w = [Fraction(float(np.float32(1) / np.float32(f))) for f in np.asarray(freqs, dtype=np.float32)]
    den = max(x.denominator for x in w)                 # (powers of two: the largest is the common one)
    wq = [int(x * den) for x in w]
    while all(q % 2 == 0 for q in wq):
        wq, den = [q // 2 for q in wq], Fraction(den) / 2
    return wq, Fraction(den)


def integer_pick(labels, px, wq, m):
    """labels int [h, w] (remapped, flipped, warped: what CropNP sees), wq Python ints, m = int(u * 2^53) -> (v, h, total, flat index)"""
    h, w = labels.shape
    margin, rh, rw = region(h, w, px)
    reg = np.asarray(labels)[margin:h - margin, margin:h - margin]
    assert reg.shape == (rh, rw) and reg.size > 0
    assert max(wq) * reg.size < 1 << 62
    table = np.zeros(256, dtype=np.int64)
    table[:len(wq)] = wq
    cum = np.cumsum(table[reg.reshape(-1)], dtype=np.int64)           # exact: below 2^62
    total = int(cum[-1])
    T = (int(m) * total) >> 53
    i = min(int(np.searchsorted(cum, T, side="right")), reg.size - 1)  # first cum_i > T
    return i // rw, i % rw, total, i


def m_with_threshold(total, T):
    """the smallest m with (m * total) >> 53 == T (T < total)"""
    m = -((-T << 53) // total)          # ceil(T * 2^53 / total)
    assert (m * total) >> 53 == T and m < 1 << 53
    return m
