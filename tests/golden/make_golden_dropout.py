"""tests/golden/dropout.npz: the reference's two Dropout2d sites in train mode (models/OCR.py:83-89 interm_prediction_head, :287-321
SpatialOCR_Module + the 1 x 1 classifier behind it), the masks recorded by forward hooks on their nn.Dropout2d.

Per site (prefix ocr_ / interm_): y = the output of the convolution in front of the BatchNorm (captured by a hook, NCHW), gamma / beta, the
classifier's wh / bh, mult = the recorded multipliers [B, C], logits, the logits' cotangent dlogits, and the gradients dy (of y), dgamma,
dbeta, dwh, dbh.  Build container only:  python tests/golden/make_golden_dropout.py"""
import os

import numpy as np
import torch
from torch import nn

import ref_harness

B, H, W, C, K = 2, 6, 10, 128, 7


def record(seq, drop_index, x_in, forward, p, out):
    """seq: the Sequential that holds conv [0], BatchNorm [1], ReLU [2], Dropout2d [drop_index]; forward() -> logits"""
    kept = {}

    def conv_hook(mod, inp, res):
        res.retain_grad()
        kept["y"] = res

    def drop_hook(mod, inp, res):
        x = inp[0].detach()
        assert bool((x.amax(dim=(2, 3)) > 0).all()), "a dropout input channel without a positive element: the mask would be ambiguous"
        m = (res.detach().amax(dim=(2, 3)) / x.amax(dim=(2, 3)))            # [B, C]: 0 or 1 / (1 - p)
        kept["mult"] = torch.where(m > 0, torch.full_like(m, float(np.float32(1) / (np.float32(1) - np.float32(p)))), torch.zeros_like(m))
        assert torch.equal(res.detach(), x * kept["mult"][:, :, None, None])
    h1, h2 = seq[0].register_forward_hook(conv_hook), seq[drop_index].register_forward_hook(drop_hook)
    logits = forward()
    h1.remove(), h2.remove()
    dl = torch.randn(logits.shape, generator=torch.Generator().manual_seed(7)) * 1e-2
    logits.backward(dl)
    bn = seq[1]
    out.update(y=kept["y"].detach(), dy=kept["y"].grad, gamma=bn.weight.detach(), beta=bn.bias.detach(), dgamma=bn.weight.grad,
               dbeta=bn.bias.grad, mult=kept["mult"], logits=logits.detach(), dlogits=dl, p=np.float32(p))
    return out


def main():
    ref = ref_harness.load()
    from models.OCR import SpatialOCR_Module
    torch.manual_seed(20)
    res = {}
    # ---- SpatialOCR_Module(dropout = 0.5) + classifier: 2 * 128 -> 128 channels
    ocr = SpatialOCR_Module(C, C // 2, C, 1, 0.5).train()
    cls = nn.Conv2d(C, K, 1, 1, 0, bias=True)
    with torch.no_grad():
        for m in ocr.modules():
            if isinstance(m, nn.BatchNorm2d):
                m.weight.uniform_(0.5, 1.5)
                m.bias.uniform_(-0.3, 0.3)
    feats, proxy = torch.randn(B, C, H, W), torch.randn(B, C, K, 1)
    o = record(ocr.conv_bn_dropout, 3, None, lambda: cls(ocr(feats, proxy)), 0.5, {})
    o.update(wh=cls.weight.detach(), bh=cls.bias.detach(), dwh=cls.weight.grad, dbh=cls.bias.grad)
    res.update({"ocr_" + k: v for k, v in o.items()})
    # ---- interm_prediction_head-shaped Sequential (p = 0.3)
    head = nn.Sequential(nn.Conv2d(48, C, 3, 1, 1), nn.BatchNorm2d(C), nn.ReLU(inplace=True), nn.Dropout2d(0.3),
                         nn.Conv2d(C, K, 1, 1, 0, bias=True)).train()
    with torch.no_grad():
        head[1].weight.uniform_(0.5, 1.5)
        head[1].bias.uniform_(-0.3, 0.3)
    x = torch.randn(B, 48, H, W)
    o = record(head, 3, None, lambda: head(x), 0.3, {})
    o.update(wh=head[4].weight.detach(), bh=head[4].bias.detach(), dwh=head[4].weight.grad, dbh=head[4].bias.grad)
    res.update({"interm_" + k: v for k, v in o.items()})
    for tag in ("ocr", "interm"):
        m = res[tag + "_mult"]
        assert 0 < int((m == 0).sum()) < m.numel()
    path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "dropout.npz")
    np.savez_compressed(path, **{k: (v.numpy() if torch.is_tensor(v) else v) for k, v in res.items()})
    print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
