"""Restatement of the dense contrastive loss (losses/contrast.py, include/ext/catseg_contrast.h): the anchor pick in numpy integers, the
loss as a torch expression (any dtype; fp64 under autograd is the reference of the tests), an independently written loop form, and the
analytic gradient the kernels implement.  The reference tree names this loss but does not ship it: these lines ARE its definition."""
import numpy as np
import torch

from _dropout_ref import philox4x32_10

STREAM_ANCHORS = 2


# ---------------------------------------------------------------------------------------------------------------- anchors
def low_labels(labels, h, w):
    """labels [B, H, W] -> [B, h, w]: l[b, i, j] = labels[b, (i H) // h, (j W) // w]"""
    labels = np.asarray(labels)
    B, H, W = labels.shape
    ii = (np.arange(h, dtype=np.int64) * H) // h
    jj = (np.arange(w, dtype=np.int64) * W) // w
    return labels[:, ii][:, :, jj]


def draw_u24(seed, layer, rank, draw, A):
    """the top 24 bits of word a & 3 of philox4x32_10((a >> 2, draw, 2, layer | rank << 16), seed)"""
    a = np.arange(A, dtype=np.uint64)
    words = philox4x32_10((a >> 2, np.uint64(draw & 0xFFFFFFFF), np.uint64(STREAM_ANCHORS), np.uint64((layer & 0xFFFF) | (rank & 0xFFFF) << 16)),
                          (seed & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF))
    word = np.choose((a & 3).astype(np.int64), words)
    return (word >> np.uint32(8)).astype(np.int64)


def ranks_of(n, M, u24):
    """the ranks that the M slots of a class with n pixels take (-1: empty slot); u24: M integers in [0, 2^24)"""
    out = np.full(M, -1, dtype=np.int64)
    if n <= M:
        out[:n] = np.arange(n)
        return out
    for m in range(M):
        b0, b1 = (m * n) // M, ((m + 1) * n) // M
        out[m] = b0 + ((int(u24[m]) * (b1 - b0)) >> 24)
    return out


def pick(labels, h, w, K, M, u24):
    """-> (idx [K M], label [K M], n_pos): vectorised per class"""
    low = low_labels(labels, h, w).reshape(-1)
    idx = np.full(K * M, -1, dtype=np.int64)
    lab = np.full(K * M, -1, dtype=np.int64)
    n_pos = 0
    for c in range(K):
        pix = np.flatnonzero(low == c)
        r = ranks_of(len(pix), M, u24[c * M:(c + 1) * M])
        ok = r >= 0
        idx[c * M:(c + 1) * M][ok] = pix[r[ok]]
        lab[c * M:(c + 1) * M][ok] = c
        nc = min(len(pix), M)
        n_pos += nc if nc >= 2 else 0
    return idx, lab, n_pos


def pick_brute(labels, h, w, K, M, u24):
    """the same rule pixel by pixel, slot by slot, in Python integers"""
    labels = np.asarray(labels)
    B, H, W = labels.shape
    per_class = [[] for _ in range(K)]
    for b in range(B):
        for i in range(h):
            for j in range(w):
                l = int(labels[b, (i * H) // h, (j * W) // w])
                if 0 <= l < K:
                    per_class[l].append((b * h + i) * w + j)
    idx, lab, n_pos = [], [], 0
    for c in range(K):
        n = len(per_class[c])
        for m in range(M):
            if n <= M:
                r = m if m < n else None
            else:
                lo, hi = (m * n) // M, ((m + 1) * n) // M
                r = lo + ((int(u24[c * M + m]) * (hi - lo)) >> 24)
            idx.append(-1 if r is None else per_class[c][r])
            lab.append(-1 if r is None else c)
        if min(n, M) >= 2:
            n_pos += min(n, M)
    return np.array(idx, dtype=np.int64), np.array(lab, dtype=np.int64), n_pos


# ---------------------------------------------------------------------------------------------------------------- the loss
def table(m, lam):
    """W[a, b] = 1 + lam * m[b, a]"""
    return 1.0 + lam * torch.as_tensor(m).t()


def loss_torch(feat_rows, idx, label, Wt, tau, eps):
    """feat_rows: [n_pix, d] (requires_grad for the gradient), idx / label: [A] integers, Wt: [K, K] -> the loss, in feat_rows' dtype.
    Written with torch operations only, so that autograd differentiates it."""
    idx = torch.as_tensor(idx, dtype=torch.int64)
    label = torch.as_tensor(label, dtype=torch.int64)
    filled = torch.nonzero(label >= 0).reshape(-1)
    dt = feat_rows.dtype
    if filled.numel() == 0:
        return feat_rows.sum() * 0
    f = feat_rows[idx[filled]]
    y = label[filled]
    z = torch.nn.functional.normalize(f, dim=1, eps=eps)
    s = (z @ z.t()) / tau
    n = len(filled)
    off = ~torch.eye(n, dtype=torch.bool)
    same = (y[:, None] == y[None, :]) & off
    w = torch.where(y[:, None] == y[None, :], torch.ones((), dtype=dt), Wt.to(dt)[y][:, y])
    npos = same.sum(1)
    rows = npos >= 1
    n_pos = int(rows.sum())
    if n_pos == 0:
        return feat_rows.sum() * 0
    logd = torch.logsumexp(torch.where(off, s + torch.log(w), torch.full((), -float("inf"), dtype=dt)), dim=1)
    possum = torch.where(same, s, torch.zeros((), dtype=dt)).sum(1)
    ell = -possum / npos.clamp(min=1).to(dt) + logd
    return ell[rows].sum() / max(n_pos, 1)


def loss_loop(feat_rows, idx, label, Wt, tau, eps):
    """the definition read aloud, in numpy fp64 loops -> (loss, n_pos)"""
    F = np.asarray(feat_rows, dtype=np.float64)
    Wt = np.asarray(Wt, dtype=np.float64)
    A = len(idx)
    z = {}
    for a in range(A):
        if label[a] >= 0:
            f = F[idx[a]]
            z[a] = f / max(np.sqrt((f * f).sum()), eps)
    total, n_pos = 0.0, 0
    for i in z:
        P = [j for j in z if j != i and label[j] == label[i]]
        if not P:
            continue
        n_pos += 1
        D = 0.0
        for j in z:
            if j == i:
                continue
            wij = 1.0 if label[j] == label[i] else Wt[label[i], label[j]]
            D += wij * np.exp(z[i].dot(z[j]) / tau)
        total += -sum(z[i].dot(z[p]) / tau for p in P) / len(P) + np.log(D)
    return total / max(n_pos, 1), n_pos


def grad_analytic(feat_rows, idx, label, Wt, tau, eps, g=1.0):
    """the gradient as the kernels form it: G, dZ = (G + G^T) Z / tau, the adjoint of the normalisation -> [n_pix, d] fp64"""
    F = np.asarray(feat_rows, dtype=np.float64)
    Wt = np.asarray(Wt, dtype=np.float64)
    idx, label = np.asarray(idx), np.asarray(label)
    A, d = len(idx), F.shape[1]
    filled = label >= 0
    f = np.where(filled[:, None], F[np.where(filled, idx, 0)], 0.0)
    norm = np.sqrt((f * f).sum(1))
    den = np.maximum(norm, eps)
    Z = np.where(filled[:, None], f / den[:, None], 0.0)
    s = Z @ Z.T / tau
    pair = filled[:, None] & filled[None, :] & ~np.eye(A, dtype=bool)
    same = pair & (label[:, None] == label[None, :])
    w = np.where(label[:, None] == label[None, :], 1.0, Wt[np.maximum(label, 0)][:, np.maximum(label, 0)])
    e = np.where(pair, w * np.exp(np.where(pair, s, 0.0)), 0.0)
    D = e.sum(1)
    cnt = same.sum(1)
    rows = cnt >= 1
    n_pos = int(rows.sum())
    G = np.zeros((A, A))
    if n_pos:
        G[rows] = g * (e[rows] / D[rows, None] - same[rows] / cnt[rows, None]) / n_pos
    dZ = (G + G.T) @ Z / tau
    dot = (dZ * Z).sum(1)
    df = np.where((norm < eps)[:, None], dZ / eps, (dZ - dot[:, None] * Z) / den[:, None])
    out = np.zeros_like(F)
    out[idx[filled]] = df[filled]
    return out
