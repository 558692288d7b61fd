"""Functional CPU restatement of the reference's UNet (models/UNet.py:6-63): state dict in, logits out, in the dtype of the state dict
(fp32 for the train-step comparison, fp64 for the calibration of the GPU tests).  Checked against the fixture the real reference wrote
(tests/golden/make_golden_unet.py) by tests/test_unet_cpu.py."""
import numpy as np
import torch
import torch.nn.functional as F


def _double_conv(S, name, x):
    x = F.relu(F.conv2d(x, S[name + ".0.weight"], S[name + ".0.bias"], padding=1))
    return F.relu(F.conv2d(x, S[name + ".2.weight"], S[name + ".2.bias"], padding=1))


def _up(x):
    return F.interpolate(x, scale_factor=2, mode="bilinear", align_corners=True)


def unet_forward(S, x):
    c1 = _double_conv(S, "dconv_down1", x)
    c2 = _double_conv(S, "dconv_down2", F.max_pool2d(c1, 2))
    c3 = _double_conv(S, "dconv_down3", F.max_pool2d(c2, 2))
    y = _double_conv(S, "dconv_down4", F.max_pool2d(c3, 2))
    y = _double_conv(S, "dconv_up3", torch.cat([_up(y), c3], 1))
    y = _double_conv(S, "dconv_up2", torch.cat([_up(y), c2], 1))
    y = _double_conv(S, "dconv_up1", torch.cat([_up(y), c1], 1))
    return F.conv2d(y, S["conv_last.weight"], S["conv_last.bias"])


def make_inputs(seed, shape, K):
    """the fixture's image and label map: labels 0 .. K - 1 (K - 1 = the 'ignore' entry the reference's UNet keeps as a class) in 8 x 8 patches"""
    g = torch.Generator().manual_seed(seed + 1)
    x = torch.rand(shape, generator=g)
    lbl = torch.randint(0, K, (shape[0], shape[2] // 8, shape[3] // 8), generator=g)
    return x, lbl.repeat_interleave(8, 1).repeat_interleave(8, 2).contiguous()


def summarise(t):
    t = t.detach()
    H = t.shape[2]
    return {"sub": t[:, :, ::4, ::4].numpy().copy(), "rows": t[:, :, [0, H // 2 - 1, H - 1], :].numpy().copy(),
            "sum": np.array(float(t.double().sum())), "abs": np.array(float(t.double().abs().sum()))}
