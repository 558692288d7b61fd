"""UNet on the HIP engine -- constructor / forward contract and state-dict keys of the reference's models/UNet.py:6-63: four double_conv
levels (3x3 conv + bias + ReLU, twice; 64 / 128 / 256 / 512 channels), MaxPool2d(2) between them, and on the way up
Upsample(scale_factor=2, bilinear, align_corners=True) + torch.cat([up, skip], 1) + double_conv, then a 1x1 class layer.  The input height
and width must be multiples of 8 (the reference's torch.cat at :49,53,57 needs the up-sampled map to match the skip tensor).

No layer here has a BatchNorm, so none of the engine's amax-record producers runs; with the plan field `bnfree_records` the pool, the skip
junction and the ReLU backward leave the records instead (csrc/unet.hip) and the layers reach the f16x2 direct and gather kernels."""
from torch import nn

from ..engine import Conv2d, EngineNet, conv_act, conv_bias, image_hw, maxpool2, upcat
from ..utils import num_classes
from ..utils.classes import IGNORE_LABEL


def double_conv(in_channels, out_channels):
    # models/UNet.py:6-12 of the reference: the ReLU modules (indices 1 and 3) own no parameters, the convolutions keep the keys "0" and "2"
    return nn.Sequential(Conv2d(in_channels, out_channels, 3, padding=1), nn.ReLU(inplace=True),
                         Conv2d(out_channels, out_channels, 3, padding=1), nn.ReLU(inplace=True))


class UNet(EngineNet):
    def __init__(self, config, experiment):
        super().__init__()
        # models/UNet.py:20 of the reference counts len(CLASS_INFO[experiment][1]) and, unlike FCN.py:12-13, keeps the 'ignore' entry of
        # tasks 2 and 3: 18 / 26 logit channels (8 for task 1), which is what its checkpoints hold
        self.num_classes = num_classes(experiment) + (IGNORE_LABEL[experiment] is not None)
        self.dconv_down1 = double_conv(3, 64)
        self.dconv_down2 = double_conv(64, 128)
        self.dconv_down3 = double_conv(128, 256)
        self.dconv_down4 = double_conv(256, 512)
        self.dconv_up3 = double_conv(256 + 512, 256)
        self.dconv_up2 = double_conv(128 + 256, 128)
        self.dconv_up1 = double_conv(128 + 64, 64)
        self.conv_last = Conv2d(64, self.num_classes, 1)
        self.apply_freeze_bn(config or {})  # (no BatchNorm here: a freeze_bn key is refused as matching nothing)

    @staticmethod
    def _double(cx, x, block, last):
        """double_conv: the first output feeds the second convolution alone (its record needs a pass of its own); `last`: how the second
        output gets its record -- "pool" for an encoder level (read by the pool and the skip junction), True otherwise"""
        return conv_act(cx, conv_act(cx, x, block[0], record=True), block[2], record=last)

    def _body(self, cx, x):
        H, W = image_hw(x)
        if H % 8 or W % 8:
            raise ValueError("UNet: input %d x %d is not a multiple of 8 (models/UNet.py:49 of the reference concatenates a 2x up-sampled "
                             "map with the skip tensor of the level above)" % (H, W))
        c1 = self._double(cx, x, self.dconv_down1, "pool")
        c2 = self._double(cx, maxpool2(cx, c1, record=True), self.dconv_down2, "pool")
        c3 = self._double(cx, maxpool2(cx, c2, record=True), self.dconv_down3, "pool")
        y = self._double(cx, maxpool2(cx, c3, record=True), self.dconv_down4, True)
        y = self._double(cx, upcat(cx, y, c3), self.dconv_up3, True)
        y = self._double(cx, upcat(cx, y, c2), self.dconv_up2, True)
        y = self._double(cx, upcat(cx, y, c1), self.dconv_up1, True)
        return [conv_bias(cx, y, self.conv_last)]
