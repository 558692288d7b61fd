"""Fixture for the egress kernel and the utils.egress functions, generated with the REAL reference's get_remapped_colormap, mask_from_network,
mask_to_colormap, to_comb_image, un_normalise (utils/utils.py) and clipped_argmax (utils/torch_utils.py), experiments 1, 2 and 3.
    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_egress.py
Writes egress.npz.  Per experiment e (K network classes): logits (2, K, 12, 20) at scale 4; images (2, 3, 12, 20) in [0, 1] whose first row
holds values v with fp32(v * 255) an exact k + 0.5; targets with the ignore id; the reference's argmax(Softmax2d), its three-panel
to_comb_image per frame, clipped_argmax at 0.5 and 0.9 with the mask of pixels whose score lies within 1e-5 of the threshold, and a normalised
frame with the bytes of its un_normalise.  The two conditions the tests rely on are checked here and recorded: top-2 logit margin >= 1e-3
everywhere (argmax of the softmax = argmax of the logits), at most 1 % of pixels inside a threshold band."""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import ref_harness  # noqa: E402

R = ref_harness.load()
import utils.utils as RU  # noqa: E402  (the reference's modules: ref_harness put its tree on sys.path)
import utils.torch_utils as RT  # noqa: E402

CLASS_INFO = RU.CLASS_INFO
B, H, W = 2, 12, 20
THRESHOLDS = (0.5, 0.9)
BAND, MARGIN, CAP = 1e-5, 1e-3, 0.01
MEAN, STD = [0.485, 0.456, 0.406], [0.229, 0.224, 0.225]


def half_values():
    """fp32 values in [0, 1] whose fp32 product with 255 is exactly k + 0.5"""
    v = ((np.arange(255) + 0.5) / 255).astype(np.float32)
    p = v * np.float32(255)
    keep = p == (np.arange(255) + 0.5).astype(np.float32)
    assert keep.sum() >= 3 * W, keep.sum()
    return v[keep]


def case(e, seed):
    K = len(CLASS_INFO[e][1]) - (1 if e in (2, 3) else 0)       # network classes (the class table of 2 and 3 also names 255)
    g = torch.Generator().manual_seed(seed)
    logits = torch.randn(B, K, H, W, generator=g) * 4
    top2 = torch.topk(logits, min(2, K), dim=1).values
    margin = float((top2[:, 0] - top2[:, 1]).min())
    img = torch.rand(B, 3, H, W, generator=g)
    hv = torch.from_numpy(half_values())
    img[:, :, 0, :] = hv[torch.randint(0, len(hv), (B, 3, W), generator=g)]
    img[0, :, 1, 0], img[0, :, 1, 1] = 0.0, 1.0
    ignore_id = len(CLASS_INFO[e][1]) - 1 if e in (2, 3) else None
    tgt = torch.randint(0, K + (1 if ignore_id is not None else 0), (B, H, W), generator=g)
    if ignore_id is not None:
        tgt[:, 2, :5] = ignore_id
    with torch.no_grad():
        sm = torch.nn.Softmax2d()(logits)
        pred = torch.argmax(sm, dim=1)                                               # managers/BaseManager.py:722
    assert torch.equal(pred, torch.argmax(logits, dim=1))
    comb = np.stack([RU.to_comb_image(img[b], tgt[b].clone(), pred[b].clone(), e) for b in range(B)])
    assert comb.shape == (B, H, 3 * W, 3) and comb.dtype == np.uint8
    out = {"logits": logits.numpy().copy(), "img": img.numpy().copy(), "target": tgt.numpy().astype(np.uint8), "pred": pred.numpy().astype(np.uint8),
           "comb": comb, "margin": np.float32(margin)}
    scores = sm.max(dim=1).values
    n_excluded = 0
    for t in THRESHOLDS:
        ign = K if ignore_id is None else ignore_id                                  # (experiment 1 has no ignore id: one past the classes)
        clipped = RT.clipped_argmax(sm, t, ign)
        band = (scores - t).abs() <= BAND
        n_excluded = max(n_excluded, int(band.sum()))
        out["clipped_%d" % round(t * 100)] = clipped.numpy().astype(np.uint8)
        out["band_%d" % round(t * 100)] = band.numpy()
        out["clipped_u8_%d" % round(t * 100)] = RU.mask_from_network(clipped.numpy().copy(), e).astype(np.uint8)
    out["excluded"] = np.int32(n_excluded)
    # network-id table and colour table as the reference's functions give them
    out["lut"] = RU.mask_from_network(np.arange(256), e).astype(np.uint8)
    cmap = RU.get_remapped_colormap(CLASS_INFO[e][0])
    out["cmap_keys"] = np.array(list(cmap.keys()), dtype=np.int32)
    out["cmap_colours"] = np.array([np.asarray(c) for c in cmap.values()], dtype=np.uint8)
    # a normalised frame: the bytes of un_normalise(frame) (utils/utils.py:453), as to_comb_image rounds them
    xn = (torch.rand(B, 3, H, W, generator=g) - torch.tensor(MEAN).view(1, 3, 1, 1)) / torch.tensor(STD).view(1, 3, 1, 1)
    un = [RU.un_normalise(xn[b], MEAN, STD) for b in range(B)]
    out["img_norm"] = xn.numpy().copy()
    out["img_norm_u8"] = np.stack([RU.to_comb_image(u, tgt[b].clone(), pred[b].clone(), e)[:, :W] for b, u in enumerate(un)])
    ok = margin >= MARGIN and n_excluded <= CAP * B * H * W
    return out, ok, margin, n_excluded


if __name__ == "__main__":
    arrs = {"cadis_colormap": RU.get_cadis_colormap().astype(np.uint8), "band": np.float32(BAND), "thresholds": np.array(THRESHOLDS),
            "mean": np.array(MEAN, dtype=np.float32), "std": np.array(STD, dtype=np.float32)}
    for e in (1, 2, 3):
        for seed in range(600 + 10 * e, 600 + 10 * e + 10):       # the first seed whose inputs meet both conditions
            out, ok, margin, n_excluded = case(e, seed)
            if ok:
                break
        assert ok, "no seed meets the margin / band conditions for experiment %d" % e
        print("experiment %d: seed %d, top-2 margin %.3g, %d pixels inside a threshold band" % (e, seed, margin, n_excluded))
        arrs.update({"e%d_%s" % (e, k): v for k, v in out.items()})
        arrs["e%d_seed" % e] = np.int32(seed)
    path = os.path.join(HERE, "egress.npz")
    np.savez_compressed(path, **arrs)
    print("wrote egress.npz  %.1f KB" % (os.path.getsize(path) / 1024))
    assert os.path.getsize(path) <= 400 << 10
