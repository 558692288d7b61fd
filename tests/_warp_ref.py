"""Dense float64 restatement of the reference's geometric augmentation: the literal sequence of AffineNP.__call__ (utils/transforms.py:38-61,
crop_to_fit=False) -- concatenate image, ones mask and K-channel one-hot as float64, warp onto the 2H x 2W canvas, np.round three channels,
np.argmax K channels -- with a numpy remap standing in for cv2.warpPerspective (cv2 is not installed where the fixtures are made, so the warp
is pinned to this restatement of OpenCV's fixed-point bilinear remap, not to a recording):

    Minv = np.linalg.inv(matrix);  X = rint(((Minv00 x + Minv01 y) + Minv02) * 32), Y likewise, each operation rounded on its own in float64,
    clamped to int32;  sx = X >> 5, fx = X & 31;  the four neighbours weigh (32-fx)(32-fy), fx(32-fy), (32-fx)fy, fx fy over 1024 (a float32
    table, exact), a neighbour outside the frame contributes 0 (constant border).

Plus the numpy flip / crop / pad / ToTensor / Normalize around it, in the reference's order (Dataset_from_df.py:49-65, utils/utils.py:353-447)."""
import numpy as np


def to_one_hot_np(array, num_classes):
    res = np.eye(num_classes)[np.array(array).reshape(-1)]
    return res.reshape(*array.shape, num_classes)


def fixed_point_coords(minv, Hc, Wc):
    """(X, Y) int64 [Hc, Wc]: source coordinates of every canvas pixel in 1/32 pixel.  numpy evaluates every operation separately (no FMA)."""
    x = np.arange(Wc, dtype=np.float64)[None, :]
    y = np.arange(Hc, dtype=np.float64)[:, None]
    out = []
    for row in (0, 1):
        v = np.rint(((minv[row, 0] * x + minv[row, 1] * y) + minv[row, 2]) * 32.0)
        out.append(np.clip(v, -2147483648.0, 2147483647.0).astype(np.int64))
    return out[0], out[1]


def warp_bilinear(src, matrix, Hc, Wc):
    """stand-in for cv2.warpPerspective(src, matrix, (Wc, Hc)) on a float64 [H, W, C] array: bilinear, constant border 0"""
    return warp_bilinear_inv(src, np.linalg.inv(matrix), Hc, Wc)


def warp_bilinear_inv(src, minv, Hc, Wc):
    """the same from the canvas -> frame matrix (rows 0 and 1 are used)"""
    H, W, C = src.shape
    X, Y = fixed_point_coords(minv, Hc, Wc)
    sx, fx, sy, fy = X >> 5, X & 31, Y >> 5, Y & 31
    dst = np.zeros((Hc, Wc, C), dtype=np.float64)
    for dy, dx in ((0, 0), (0, 1), (1, 0), (1, 1)):
        w = ((fx if dx else 32 - fx) * (fy if dy else 32 - fy)).astype(np.float32) / np.float32(1024)     # the float weight table
        yy, xx = sy + dy, sx + dx
        ok = (yy >= 0) & (yy < H) & (xx >= 0) & (xx < W)
        v = src[np.clip(yy, 0, H - 1), np.clip(xx, 0, W - 1)] * ok[..., None]
        dst += v * w.astype(np.float64)[..., None]
    return dst


def affine_np(img, lbl, matrix, num_classes, minv=None):
    """AffineNP.__call__ with crop_to_fit=False: img uint8 [H,W,3], lbl int [H,W] (remapped) -> (img uint8 [2H,2W,3], lbl int64 [2H,2W]);
    minv: skip the inversion and use this canvas -> frame matrix"""
    mask = np.ones_like(lbl)
    src = np.concatenate((img, mask[..., np.newaxis], to_one_hot_np(lbl, num_classes)), axis=2)
    assert src.dtype == np.float64
    warped = warp_bilinear_inv(src, np.linalg.inv(matrix) if minv is None else minv, src.shape[0] * 2, src.shape[1] * 2)
    out = np.round(warped[..., :3]).astype('uint8')
    return out, np.argmax(warped[..., 4:], axis=2)


def flip_np(img, lbl, flag):
    """FlipNP: bit 1 vertical first, then bit 0 horizontal"""
    if flag & 2:
        img, lbl = np.flip(img, axis=0), np.flip(lbl, axis=0)
    if flag & 1:
        img, lbl = np.flip(img, axis=1), np.flip(lbl, axis=1)
    return img.copy(), lbl.copy()


def augment_frame(img, lbl, lut, flag, matrix, num_classes, origin=None, window=None, pad=(0, 0)):
    """one frame through remap -> flip -> affine (matrix None: none) -> crop (origin (v, h), window (hw, ww); None: none) -> reflect pad of the rows.
    Returns (img uint8 [H', W', 3], lbl int64 [H', W'])"""
    lbl = lut[lbl].astype('int32')
    img, lbl = flip_np(img, lbl, int(flag))
    if matrix is not None:
        img, lbl = affine_np(img, lbl, matrix, num_classes)
    if origin is not None:
        v, h = int(origin[0]), int(origin[1])
        img, lbl = img[v:v + window[0], h:h + window[1]], lbl[v:v + window[0], h:h + window[1]]
        assert img.shape[:2] == tuple(window)
    if pad != (0, 0):
        img = np.pad(img, (tuple(pad), (0, 0), (0, 0)), mode='reflect')
        lbl = np.pad(lbl, (tuple(pad), (0, 0)), mode='reflect')
    return np.ascontiguousarray(img), np.ascontiguousarray(lbl).astype(np.int64)


def to_tensor(img_u8, mean=None, std=None):
    """ToTensor (+ Normalize) on a uint8 [.., H, W, 3] array -> float32 [.., 3, H, W], with torch's own arithmetic"""
    import torch
    x = torch.from_numpy(np.ascontiguousarray(np.moveaxis(img_u8, -1, -3))).float().div(255)
    if mean is not None:
        m = torch.tensor(mean, dtype=torch.float32).view(3, 1, 1)
        s = torch.tensor(std, dtype=torch.float32).view(3, 1, 1)
        x = x.sub(m).div(s)
    return x.numpy()


def integer_form(img, lbl, minv, Hc, Wc):
    """the exact integer form of the same warp in plain Python (what the kernel computes per canvas pixel)"""
    H, W = lbl.shape
    out_img = np.zeros((Hc, Wc, 3), dtype=np.uint8)
    out_lbl = np.zeros((Hc, Wc), dtype=np.int64)
    X, Y = fixed_point_coords(minv, Hc, Wc)
    for y in range(Hc):
        for x in range(Wc):
            sx, fx, sy, fy = int(X[y, x]) >> 5, int(X[y, x]) & 31, int(Y[y, x]) >> 5, int(Y[y, x]) & 31
            acc, votes = [0, 0, 0], {}
            for dy, dx in ((0, 0), (0, 1), (1, 0), (1, 1)):
                w = (fx if dx else 32 - fx) * (fy if dy else 32 - fy)
                yy, xx = sy + dy, sx + dx
                if w > 0 and 0 <= yy < H and 0 <= xx < W:
                    for ch in range(3):
                        acc[ch] += int(img[yy, xx, ch]) * w
                    votes[int(lbl[yy, xx])] = votes.get(int(lbl[yy, xx]), 0) + w
            for ch in range(3):
                q, r = acc[ch] >> 10, acc[ch] & 1023
                out_img[y, x, ch] = q + (1 if (r > 512 or (r == 512 and q & 1)) else 0)
            if votes:
                top = max(votes.values())
                out_lbl[y, x] = min(k for k, v in votes.items() if v == top)
    return out_img, out_lbl
