"""Restatement of csrc/dropout.hip in numpy (Philox4x32-10 and the mask layout, bit for bit) and an fp64 evaluation of
BatchNorm -> ReLU -> Dropout2d -> 1 x 1 classifier with its gradients (what csrc/headfuse.h computes with DROP)."""
import numpy as np
import torch

M0, M1, W0, W1 = 0xD2511F53, 0xCD9E8D57, 0x9E3779B9, 0xBB67AE85


def philox4x32_10(counter, key):
    """counter: four uint32 arrays (or scalars) of one shape, key: two uint32 scalars -> four uint32 arrays"""
    c = [np.asarray(v, dtype=np.uint64) & 0xFFFFFFFF for v in np.broadcast_arrays(*counter)]
    k0, k1 = int(key[0]) & 0xFFFFFFFF, int(key[1]) & 0xFFFFFFFF
    for _ in range(10):
        p0, p1 = M0 * c[0], M1 * c[2]
        c = [(p1 >> 32) ^ c[1] ^ k0, p1 & 0xFFFFFFFF, (p0 >> 32) ^ c[3] ^ k1, p0 & 0xFFFFFFFF]
        k0, k1 = (k0 + W0) & 0xFFFFFFFF, (k1 + W1) & 0xFFFFFFFF
    return [v.astype(np.uint32) for v in c]


def keep_of(p):
    """the multiplier of a kept channel, in fp32 as the library computes it"""
    p = np.float32(p)
    return np.float32(0.0) if p >= 1 else np.float32(1.0) / (np.float32(1.0) - p)


def mask(seed, layer, rank, draw, p, B, C):
    """-> (kept bool [B, C], mult float32 [B, C], bits uint32 [B, C // 32] or None)"""
    i = np.arange(B * C, dtype=np.uint64)
    words = philox4x32_10((i >> 2, np.uint64(draw & 0xFFFFFFFF), np.uint64(0), np.uint64((layer & 0xFFFF) | (rank & 0xFFFF) << 16)),
                          (seed & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF))
    word = np.choose((i & 3).astype(np.int64), words)
    u = (word >> np.uint32(8)).astype(np.float32) * np.float32(2.0 ** -24)
    kept = (u >= np.float32(p)).reshape(B, C)
    return (kept,) + tables(kept, p)


def tables(kept, p):
    """(mult, bits) of a given keep table"""
    keep = keep_of(p)
    kept = np.asarray(kept, dtype=bool)
    B, C = kept.shape
    mult = np.where(kept, keep, np.float32(0)).astype(np.float32)
    bits = None
    if C % 32 == 0:
        on = (kept & (keep != 0)).reshape(B, C // 32, 32).astype(np.uint64)
        bits = (on << np.arange(32, dtype=np.uint64)).sum(-1).astype(np.uint32)
    return mult, bits


def head_fp64(y, mean, invstd, gamma, beta, scale32, wh, bh, mult, dl, hw):
    """y [rows, C] fp32 values, mult [B, C] the STORED fp32 multipliers, dl [rows, K]: everything in fp64.
    -> dict(logits, dwh, dbh, dgamma, dbeta, dy, dbias, z)"""
    f = lambda t: torch.as_tensor(t).double()
    y, mean, invstd, gamma, beta, scale32, wh, bh, mult, dl = map(f, (y, mean, invstd, gamma, beta, scale32, wh, bh, mult, dl))
    rows = y.shape[0]
    m = mult.repeat_interleave(hw, 0)                                 # [rows, C]
    pre = (y - mean) * scale32 + beta
    z = torch.relu(pre) * m
    logits = z @ wh.t() + bh
    g = (dl @ wh) * (pre > 0) * m
    xh = (y - mean) * invstd
    sg, sgx = g.sum(0), (g * xh).sum(0)
    dy = gamma * invstd * (g - sg / rows - xh * (sgx / rows))
    return dict(pre=pre, z=z, logits=logits, dwh=dl.t() @ z, dbh=dl.sum(0), dgamma=sgx, dbeta=sg, dy=dy, dbias=dy.sum(0), g=g, xh=xh)
