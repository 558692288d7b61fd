"""Torch-CPU restatement of the eval-mode refinement loop of the reference's PointRend (models/PointRend.py:74-90,
utils/pointrend_utils.py:25-46,119-148,220-232), dtype-generic: in fp32 it is the reference's own sequence of torch calls (F.interpolate,
torch.topk over the classes, F.grid_sample, torch.cat, F.conv1d, scatter_), in fp64 it is the yardstick of the GPU tests.  Two things are
fixed here that the reference leaves open or implicit:
  * the selection: among equal uncertainties the LOWER pixel index is taken (a stable descending sort; -0.0 == +0.0).  The indices come
    in descending order of uncertainty, which is torch.topk's order wherever no two values are equal, so that the fp32 evaluation runs the
    reference's very sequence of operations; nothing downstream depends on the order, compare index SETS;
  * the point coordinates are always formed in fp32 as the reference does, then cast: the fp64 evaluation is "fed the fp32 coordinates".
Also here: fill_state for state dicts with nn.Conv1d weights, and the reconstruction of the full tensors of the PointRend fixture."""
import os
import sys

import numpy as np
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

CONFIG = {"A": 1024, "B": 96}       # pr_subdivision_num_pts of the fixture's two configurations


def uncertainty(seg):
    """calculate_uncertainty: second-largest - largest logit, [N, h, w]"""
    top2 = torch.topk(seg, k=2, dim=1)[0]
    return top2[:, 1] - top2[:, 0]


def select(u, k):
    """[N, h, w] -> [N, min(k, h w)] int64: the k largest in descending order, the lower index first among equals"""
    N = u.shape[0]
    flat = u.reshape(N, -1)
    k = min(flat.shape[1], int(k))
    return torch.sort(flat, dim=1, descending=True, stable=True)[1][:, :k]


def kth_values(u, k):
    """(k-th, (k+1)-th) largest uncertainty per image; the second is -inf where k covers the map"""
    N = u.shape[0]
    s = torch.sort(u.reshape(N, -1), dim=1, descending=True)[0]
    k = min(s.shape[1], int(k))
    nxt = s[:, k] if k < s.shape[1] else torch.full((N,), -float("inf"), dtype=s.dtype)
    return s[:, k - 1], nxt


def point_coords(idx, h, w):
    """centres of the selected cells of the h x w grid in [0, 1]^2, [N, k, 2] as (x, y), with the reference's fp32 roundings: the step
    1 / size is a double that is rounded to fp32 where it meets the fp32 column / row index; the product and the sum round once each"""
    col, row = (idx % w).float(), (idx // w).float()
    sx, sy = 1.0 / w, 1.0 / h            # Python floats (double), as in the reference
    return torch.stack((col * sx + sx / 2, row * sy + sy / 2), dim=2)


def point_sample(fmap, pts, padding_mode="zeros"):
    """point_sample: F.grid_sample(map, 2 pts - 1) with the defaults (bilinear, align_corners=False, zero padding); [N, C, P]"""
    grid = (2.0 * pts - 1.0).to(fmap.dtype).unsqueeze(2)        # 2 p - 1 is formed in fp32 (the reference's dtype), then cast
    return F.grid_sample(fmap, grid, mode="bilinear", padding_mode=padding_mode, align_corners=False).squeeze(3)


def point_head(fine, coarse, head):
    """StandardPointHead.forward; head = {"fc": [(w [O, I, 1], b)], "predictor": (w, b), "coarse_in_each_layer": bool}"""
    x = torch.cat((fine, coarse), dim=1)
    for w, b in head["fc"]:
        x = F.relu(F.conv1d(x, w, b))
        if head.get("coarse_in_each_layer", True):
            x = torch.cat((x, coarse), dim=1)
    return F.conv1d(x, head["predictor"][0], head["predictor"][1])


def head_to(head, dtype):
    c = lambda t: t.detach().cpu().reshape(t.shape[0], -1, 1).to(dtype)
    return {"fc": [(c(w), b.detach().cpu().to(dtype)) for w, b in head["fc"]], "predictor": (c(head["predictor"][0]), head["predictor"][1].detach().cpu().to(dtype)),
            "coarse_in_each_layer": head.get("coarse_in_each_layer", True)}


def refine(coarse, feats, head, k0, steps, dtype=torch.float32):
    """coarse [N, K, h, w], feats NCHW shallow to deep -> (final [N, K, h 2^steps, w 2^steps], per step a dict with idx (int64, select's order),
    uncertainty [N, h, w], before (the upsampled logits before the scatter), point_logits [N, K, k], kth / next (the k-th and (k+1)-th
    largest uncertainty per image))"""
    seg = coarse.to(dtype).clone()
    feats = [f.to(dtype) for f in feats]
    head = head_to(head, dtype)
    rec = []
    for _ in range(steps):
        seg = F.interpolate(seg, scale_factor=2, mode="bilinear", align_corners=False)
        u = uncertainty(seg)
        n, c, h, w = seg.shape
        idx = select(u, k0)
        kth, nxt = kth_values(u, k0)
        pts = point_coords(idx, h, w)
        fine = torch.cat([point_sample(f, pts) for f in feats[::-1]], 1)
        pl = point_head(fine, point_sample(seg, pts), head)
        before = seg.clone()
        seg = seg.reshape(n, c, h * w).scatter_(2, idx.unsqueeze(1).expand(-1, c, -1), pl).view(n, c, h, w)
        rec.append({"idx": idx, "uncertainty": u, "before": before, "point_logits": pl, "kth": kth, "next": nxt})
    return seg, rec


def fill_state(spec, seed):
    """oracle.state.fill_state for a spec that holds nn.Conv1d weights [O, I, 1]: they are drawn as [O, I, 1, 1] convolution weights"""
    from oracle.state import fill_state as fill
    S = fill([(k, tuple(s) + (1,) if len(s) == 3 else tuple(s)) for k, s in spec], seed)
    for k, s in spec:
        if len(s) == 3:
            S[k] = S[k].reshape(tuple(s))
    return S


def model_config(k0):
    return {"encoder": {"model": "ResNet18", "pretrained": False},
            "decoder": {"model": "PointRend", "pr_train_num_pts": 196, "pr_subdivision_num_pts": k0}}


def head_of(S):
    """the point head of a state dict with the reference's keys"""
    n = len([k for k in S if k.startswith("dec_model.point_head.fc") and k.endswith(".weight")])
    g = lambda name: (S["dec_model.point_head.%s.weight" % name], S["dec_model.point_head.%s.bias" % name])
    return {"fc": [g("fc%d" % (i + 1)) for i in range(n)], "predictor": g("predictor"), "coarse_in_each_layer": True}


def scatter_points(seg, idx, vals):
    n, c, h, w = seg.shape
    idx = torch.as_tensor(idx, dtype=torch.int64)
    return seg.clone().reshape(n, c, h * w).scatter_(2, idx.unsqueeze(1).expand(-1, c, -1), torch.as_tensor(vals)).view(n, c, h, w)


def fixture_tensors(g, cfg):
    """the reference's full tensors of configuration "A" / "B" from what the fixture stores: the logits the reference scattered at the
    selected pixels, every other pixel being F.interpolate of the previous step (the generator asserts that this reproduces the reference's
    output bit for bit).  Returns (step-1 output, final logits before the step-2 scatter, final logits), NCHW fp32."""
    T = torch.from_numpy
    up1 = F.interpolate(T(g["coarse"]), scale_factor=2, mode="bilinear", align_corners=False)
    step1 = scatter_points(up1, g[cfg + "_idx1"], g[cfg + "_points1"])
    up2 = F.interpolate(step1, scale_factor=2, mode="bilinear", align_corners=False)
    return step1, up2, scatter_points(up2, g[cfg + "_idx2"], g[cfg + "_points2"])


def as_np(t):
    return t.detach().cpu().numpy().copy()


# ---------------------------------------------------------------------------------------------------- the seam test's cases (tests/test_pointrend_gpu.py)
SEAM_SHAPES = {
    "fixture": dict(N=2, K=17, sizes=[(16, 16), (8, 8), (4, 4), (2, 2)], channels=(64, 128, 256, 512), fc_dim=256, num_fc=3),
    "non-nested": dict(N=2, K=8, sizes=[(17, 23), (9, 12), (5, 6), (3, 3)], channels=(8, 12, 20, 4), fc_dim=64, num_fc=2),
    # three layers of different widths (a third concatenation buffer), K = 17, and a head that takes the coarse logits in its first layer only
    "mixed widths": dict(N=2, K=17, sizes=[(17, 23), (9, 12), (5, 6), (3, 3)], channels=(8, 12, 20, 4), fc_dim=(64, 32, 48), num_fc=3),
    "coarse once": dict(N=2, K=17, sizes=[(16, 16), (8, 8), (4, 4), (2, 2)], channels=(8, 12, 20, 4), fc_dim=64, num_fc=2, each=False),
}
# (shape, k0, steps) -> seed.  Chosen by `python tests/_pointrend_ref.py` (seam_search below), which takes for every case the first seed for
# which, in the fp64 AND the fp32 evaluation, no step before the last has an undecided pixel and the last has at most 1 % of k per image,
# and the fp32 evaluation selects exactly as fp64 does outside the undecided pixels.
SEAM_SEEDS = {("fixture", 96, 2): 4, ("fixture", 96, 3): 12, ("fixture", 1024, 2): 1, ("fixture", 1024, 3): 2, ("fixture", 10 ** 9, 2): 1,
              ("fixture", 10 ** 9, 3): 1, ("non-nested", 96, 2): 3, ("non-nested", 96, 3): 71, ("non-nested", 1024, 2): 1, ("non-nested", 1024, 3): 7,
              ("non-nested", 10 ** 9, 2): 1, ("non-nested", 10 ** 9, 3): 1, ("mixed widths", 96, 2): 4, ("coarse once", 96, 2): 2}


def seam_inputs(shape, seed):
    """random coarse logits at scale 4 (the finest stage's size), random features, random head weights; the predictor at std 0.05"""
    c = SEAM_SHAPES[shape]
    g = torch.Generator().manual_seed(seed)
    N, K = c["N"], c["K"]
    coarse = torch.randn(N, K, *c["sizes"][0], generator=g) * 3
    feats = [torch.randn(N, ch, h, w, generator=g).relu() for ch, (h, w) in zip(c["channels"], c["sizes"])]
    fan, fc, each = sum(c["channels"]) + K, [], c.get("each", True)
    dims = c["fc_dim"] if isinstance(c["fc_dim"], tuple) else (c["fc_dim"],) * c["num_fc"]
    for d in dims:
        fc.append((torch.randn(d, fan, 1, generator=g) * (2.0 / fan) ** 0.5, torch.randn(d, generator=g) * 0.1))
        fan = d + (K if each else 0)
    head = {"fc": fc, "predictor": (torch.randn(K, fan, 1, generator=g) * 0.05, torch.randn(K, generator=g) * 0.1), "coarse_in_each_layer": each}
    return coarse, feats, head


def undecided(rec, scale):
    """per step a bool [N, h w]: the pixels another evaluation may select differently.  The k-th pixel itself always lies "within 1e-5 scale
    of the k-th value", so the rule is applied to the threshold, the gap between the k-th and the (k+1)-th value: a selected pixel is undecided
    if its uncertainty is within 1e-5 scale of the (k+1)-th value, an unselected one if it is within 1e-5 scale of the k-th.  Every such pixel
    lies within 1e-5 scale of the k-th value; where the gap is wider than the tolerance, or k covers the map, there is none."""
    out = []
    for r in rec:
        u = r["uncertainty"].reshape(r["uncertainty"].shape[0], -1)
        if r["idx"].shape[1] >= u.shape[1]:
            out.append(torch.zeros_like(u, dtype=torch.bool))
            continue
        sel, tol = selected(r["idx"], u.shape[1]), 1e-5 * scale
        out.append((sel & (u - r["next"][:, None] <= tol)) | (~sel & (r["kth"][:, None] - u <= tol)))
    return out


def selected(idx, hw):
    m = torch.zeros(idx.shape[0], hw, dtype=torch.bool)
    return m.scatter_(1, idx.long(), True)


def seam_reference(shape, k0, steps, seed):
    """(inputs, fp64 result, fp32 result, undecided masks of the fp64 evaluation, logit scale)"""
    inp = seam_inputs(shape, seed)
    f64, r64 = refine(*inp, k0, steps, dtype=torch.float64)
    f32, r32 = refine(*inp, k0, steps, dtype=torch.float32)
    scale = float(f64.abs().max())
    return inp, (f64, r64), (f32, r32), undecided(r64, scale), scale


def seam_seed_ok(shape, k0, steps, seed):
    _, (f64, r64), (f32, r32), und, scale = seam_reference(shape, k0, steps, seed)
    for s, (a, b, m) in enumerate(zip(r64, r32, und)):
        k, hw = a["idx"].shape[1], m.shape[1]
        if s < steps - 1 and bool(m.any()):
            return False
        if int(m.sum(1).max()) > 0.01 * k:
            return False
        if bool(((selected(a["idx"], hw) != selected(b["idx"], hw)) & ~m).any()):
            return False
    return True


def seam_cases():
    return [(shape, k0, steps) for shape in ("fixture", "non-nested") for k0 in (96, 1024, 10 ** 9) for steps in (2, 3)] + \
           [("mixed widths", 96, 2), ("coarse once", 96, 2)]


def seam_search():
    found = {}
    for case in seam_cases():
        found[case] = next(s for s in range(1, 200) if seam_seed_ok(*case, s))
        print(case, "->", found[case], flush=True)
    return found


if __name__ == "__main__":
    print("SEAM_SEEDS =", seam_search())
