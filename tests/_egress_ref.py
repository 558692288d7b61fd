"""numpy restatement of csrc/egress.hip, line by line what the reference does on the host (managers/BaseManager.py:690-741,
utils/utils.py:114-142,202-211,453; utils/torch_utils.py:7-21).  tests/test_egress_cpu.py holds it to the reference's fixture."""
import numpy as np

BAND = 1e-5      # fp32 softmax evaluations differ by a few ulps: pixels whose score is this close to the threshold are not compared


def egress(rows, probs=False, crop=(0, 0), threshold=0.0, ignore_value=0, lut=None, palette=None, frame=None, mean=None, std=None, bgr=False,
           target=None):
    """rows [B, H, W, K] float32 (None: no prediction); frame [B, 3, H, W]; target [B, H, W]; palette in RGB.
    Returns dict(labels, labels_u8, canvas, band): band marks the pixels inside the threshold band (logits only)."""
    ref = rows if rows is not None else target if target is not None else frame[:, 0]
    B, H, W = ref.shape[:3]
    y0, y1 = crop[0], H - crop[1]
    lut = np.arange(256, dtype=np.uint8) if lut is None else lut
    out = {"labels": None, "labels_u8": None, "band": np.zeros((B, y1 - y0, W), dtype=bool)}
    panels = []
    if frame is not None:
        f = frame[:, :, y0:y1].astype(np.float32)
        if mean is not None:
            f = f * np.asarray(std, dtype=np.float32).reshape(1, 3, 1, 1)
            f = f + np.asarray(mean, dtype=np.float32).reshape(1, 3, 1, 1)
        byt = np.clip(np.round(f * np.float32(255)), 0, 255).astype(np.uint8)
        byt = np.moveaxis(byt, 1, -1)
        panels.append(byt[..., ::-1] if bgr else byt)
    pal = palette[:, ::-1] if (bgr and palette is not None) else palette
    if target is not None:
        t = target[:, y0:y1]
        ok = (t >= 0) & (t <= 255)
        panels.append(pal[lut[np.where(ok, t, 0)]] * ok[..., None].astype(np.uint8))
    if rows is not None:
        x = rows[:, y0:y1].astype(np.float32)
        idx = x.argmax(-1)                                   # the first maximum
        if threshold > 0:
            mx = x.max(-1)
            if probs:
                score = mx
            else:
                score = np.float32(1) / np.exp(x - mx[..., None]).sum(-1, dtype=np.float32)
                out["band"] = np.abs(score - np.float32(threshold)) <= BAND
            idx = np.where(score < np.float32(threshold), ignore_value, idx)
        out["labels"] = idx.astype(np.int64)
        out["labels_u8"] = lut[idx]
        if pal is not None:
            panels.append(pal[out["labels_u8"]])
    out["canvas"] = np.concatenate(panels, axis=2) if panels and pal is not None else None
    return out


def tables(golden, e):
    """(lut, palette RGB) of experiment e from the reference's fixture"""
    g = golden("egress")
    pal = np.zeros((256, 3), dtype=np.uint8)
    pal[g["e%d_cmap_keys" % e]] = g["e%d_cmap_colours" % e]
    return g["e%d_lut" % e], pal
