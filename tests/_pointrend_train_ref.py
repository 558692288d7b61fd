"""Torch-CPU restatement of the train-mode forward of the reference's PointRend (models/PointRend.py:43-73,
utils/pointrend_utils.py:65-116) and of the manager's point loss (managers/EncDec_Manager.py:158-177), dtype-generic like
tests/_pointrend_ref.py, whose point_sample / point_head it is built on: in fp32 it is the reference's own sequence of torch calls, in
fp64 it is the yardstick of the GPU tests.  The point coordinates are fp32 values in either evaluation (the draw is fp32), as are the
pixel indices and the labels that derive from them.  Fixed here, left open by the reference:
  * the draw: Philox4x32-10 from (seed, layer, rank, draw number), counter word 2 = 1 (csrc/pointrend_train.hip), not torch.rand;
  * the selection: the int(beta P) most uncertain candidates, the LOWER candidate index among equals (tests/_pointrend_ref.select), kept in
    ascending candidate order (the order matters among duplicates of one pixel only: there the later point wins, and the selected points
    come in the order the device's selection emits them)."""
import os
import sys

import numpy as np
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _dropout_ref as DR  # noqa: E402
import _pointrend_ref as PR  # noqa: E402


def draw(seed, layer, rank, number, N, M):
    """the [N, M, 2] fp32 uniforms of draw `number`: float i takes word i & 3 of philox(counter = (i >> 2, number, 1, layer | rank << 16))"""
    i = np.arange(N * M * 2, dtype=np.uint64)
    words = DR.philox4x32_10((i >> 2, np.uint64(number & 0xFFFFFFFF), np.uint64(1), np.uint64((layer & 0xFFFF) | (rank & 0xFFFF) << 16)),
                             (seed & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF))
    word = np.choose((i & 3).astype(np.int64), words)
    u = (word >> np.uint32(8)).astype(np.float32) * np.float32(2.0 ** -24)
    return torch.from_numpy(u.reshape(N, M, 2))


def point_uncertainty(coarse, pts):
    """calculate_uncertainty of the point-sampled coarse logits: [N, M]"""
    top2 = torch.topk(PR.point_sample(coarse, pts), k=2, dim=1)[0]
    return top2[:, 1] - top2[:, 0]


def select_points(unc, cand, rest, kb, ascending=True):
    """(coords [N, P, 2], selected candidate indices [N, kb]): the kb most uncertain candidates, then the random rest.  ascending: the
    selected candidates in ascending candidate order, as the device's selection emits them; False: in descending order of uncertainty,
    torch.topk's order wherever no two values are equal (the reference's point order)"""
    idx = PR.select(unc.unsqueeze(1), kb)
    if ascending:
        idx = torch.sort(idx, dim=1)[0]
    picked = torch.gather(cand, 1, idx.unsqueeze(2).expand(-1, -1, 2))
    return (torch.cat((picked, rest), dim=1) if rest is not None and rest.shape[1] else picked), idx


def counts(P, ratio, beta):
    """(candidates M, importance-sampled points, random points), utils/pointrend_utils.py:89,100-101"""
    kb = int(beta * P)
    return int(P * ratio), kb, P - kb


def pixel_index(pts, h, w):
    """models/PointRend.py:56-57: fp32 tensor arithmetic, torch.round rounds half to even; int64 [N, P]"""
    pts = pts.float()
    return (torch.round(pts[..., 1] * (h - 1)) * w + torch.round(pts[..., 0] * (w - 1))).long()


def point_labels(lbl, pts):
    """managers/EncDec_Manager.py:164: point_sample(lbl.unsqueeze(1).float(), coords, mode='nearest') as int64 [N, P]"""
    grid = (2.0 * pts.float() - 1.0).unsqueeze(2)
    return F.grid_sample(lbl.unsqueeze(1).float(), grid, mode="nearest", padding_mode="zeros", align_corners=False).squeeze(3).squeeze(1).long()


def scatter_last(seg, pix, vals):
    """seg [N, K, h, w] with vals [N, K, P] written at pix [N, P], point after point: the last point of a pixel wins (scatter_ on the CPU)"""
    n, c, h, w = seg.shape
    out = seg.clone().reshape(n, c, h * w)
    for b in range(n):
        for p in range(pix.shape[1]):
            out[b, :, int(pix[b, p])] = vals[b, :, p]
    return out.view(n, c, h, w)


def forward(coarse, feats, head, pts, scale, dtype=torch.float32):
    """models/PointRend.py:59-73 at given points, differentiable: coarse [N, K, h, w], feats NCHW shallow to deep, pts [N, P, 2] fp32
    -> (point_logits [N, K, P], pred [N, K, s h, s w], pix [N, P]).  The scatter is out of place here; its forward (duplicates: the last
    point) and its backward (zero into the interpolate at scattered pixels, every duplicate receives its pixel's gradient) are those of
    the reference's in-place scatter_ on a view of seg_logits."""
    coarse = coarse.to(dtype)
    feats = [f.to(dtype) for f in feats]
    head = head_to(head, dtype)
    fine = torch.cat([PR.point_sample(f, pts) for f in feats[::-1]], 1)
    pl = PR.point_head(fine, PR.point_sample(coarse, pts), head)
    seg = F.interpolate(coarse, scale_factor=scale, mode="bilinear", align_corners=False)
    n, c, h, w = seg.shape
    pix = pixel_index(pts, h, w)
    return pl, _ScatterLast.apply(seg, pix, pl), pix


class _ScatterLast(torch.autograd.Function):
    """scatter_ of the reference (models/PointRend.py:72) spelled out: forward, the last point of a pixel stays; backward, what
    torch.scatter_'s derivative is -- the scattered-into tensor gets zero at every scattered pixel, the source the gradient of its pixel,
    every duplicate included"""

    @staticmethod
    def forward(ctx, seg, pix, vals):
        ctx.save_for_backward(pix)
        return scatter_last(seg, pix, vals)

    @staticmethod
    def backward(ctx, g):
        pix, = ctx.saved_tensors
        n, c, h, w = g.shape
        idx = pix.unsqueeze(1).expand(-1, c, -1)
        flat = g.reshape(n, c, h * w)
        return flat.scatter(2, idx, torch.zeros((), dtype=g.dtype).expand(idx.shape)).view(n, c, h, w), None, flat.gather(2, idx)


def head_to(head, dtype):
    """PR.head_to that keeps the graph of tensors that require a gradient"""
    c = lambda t: t.reshape(t.shape[0], -1, 1).to(dtype)
    return {"fc": [(c(w), b.to(dtype)) for w, b in head["fc"]], "predictor": (c(head["predictor"][0]), head["predictor"][1].to(dtype)),
            "coarse_in_each_layer": head.get("coarse_in_each_layer", True)}


def point_loss(point_logits, labels, ignore_index):
    """managers/EncDec_Manager.py:169-170"""
    return F.cross_entropy(point_logits.unsqueeze(3), labels.unsqueeze(2), ignore_index=ignore_index)


# ---------------------------------------------------------------------------------------------------- the whole network (the fixture's)
FIXTURE = "pointrend_train_r18_e2_tiny"
FIXTURE_P, FIXTURE_RATIO, FIXTURE_BETA = 48, 3, 0.75


def model_config(on_device=True):
    cfg = PR.model_config(96)
    cfg["decoder"].update(pr_train_num_pts=FIXTURE_P, pr_oversample_ratio=FIXTURE_RATIO, pr_importance_sample_ratio=FIXTURE_BETA)
    if on_device:
        cfg["decoder"]["pr_train_on_device"] = True
    return cfg


def network_forward(S, x, pts):
    """EncDec(ResNet18 + PointRend) in train mode at given points, from a state dict with the reference's keys (the oracle's ResNet / UPerNet
    restatements in front of forward() above) -> (deep features, coarse logits, point_logits, pred, pix)"""
    from oracle.upernet import resnet_basic_stages, upernet_forward
    feats = resnet_basic_stages(S, x, "ResNet18", True)
    coarse = upernet_forward(S, feats, True, prefix="dec_model.partial_upernet.", in_scale=1)      # (x 1: the coarse logits themselves)
    pl, pred, pix = forward(coarse, feats, PR.head_of(S), pts, 4, dtype=x.dtype)
    return feats[-1], coarse, pl, pred, pix


def manager_losses(pl, pred, lbl, pts, ignore_index=17):
    """managers/EncDec_Manager.py:163-171 with LossWrapper({'CrossEntropyLoss': 1}): (loss_coarse, loss_points)"""
    return F.cross_entropy(pred, lbl, ignore_index=ignore_index), point_loss(pl, point_labels(lbl, pts), ignore_index)


def fixture_pred(g):
    """the reference's pred of step 0 from what the fixture stores: F.interpolate of the coarse logits with the stored values at the
    scattered pixels (the generator asserts that this reproduces the reference's tensor bit for bit)"""
    T = torch.from_numpy
    seg = F.interpolate(T(g["coarse"]), scale_factor=4, mode="bilinear", align_corners=False)
    n, c, h, w = seg.shape
    return seg.reshape(n, c, h * w).scatter_(2, T(g["pix"]).unsqueeze(1).expand(-1, c, -1), T(g["pred_at_points"])).view(n, c, h, w)


def band(unc, kth, scale):
    """bool [N, M]: the candidates whose uncertainty lies within 4e-3 scale of the k-th value (the k-th candidate itself among them):
    another evaluation of the uncertainties may select these differently"""
    return (unc - kth[:, None]).abs() <= 4e-3 * scale
