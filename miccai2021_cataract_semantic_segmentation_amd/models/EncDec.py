"""Encoder-decoder segmentation nets on the HIP engine: the reference's EncDec (models/EncDec.py:7-53) with
the ResNet / ResNeXt encoder wrappers (models/ResNet.py:5-94, models/ResNeXt.py:5-60: torchvision trunks
returning the four stage outputs), the UPerNet decoder (models/UPerNet.py:7-145) and the PointRend decoder (models/PointRend.py:8-141;
its train-mode forward behind config['decoder']['pr_train_on_device']).  State-dict keys as in the reference: ``enc_model.layer1.0.conv1.weight``,
``dec_model.ppm_conv.0.0.weight``, ``dec_model.partial_upernet.ppm_conv.0.0.weight``, ``dec_model.point_head.fc1.weight`` ..."""
import math

import torch
from torch import nn

from ..engine import (BatchNorm2d, Conv2d, EngineNet, PointSampler, adaptive_avgpool, add_n, bilinear, concat_views, conv_bias,
                      conv_bn_act, copy_into, maxpool, pointrend_refine, pointrend_train)
from ..utils import num_classes
from .backbone import BasicBlock, Bottleneck, _c1, load_pretrained_trunk
from .Projector import make_projector


class _GroupedBottleneck(nn.Module):
    """torchvision Bottleneck with groups / width_per_group (ResNeXt); forward-only on the HIP path"""
    expansion = 4

    def __init__(self, inplanes, planes, stride=1, downsample=None, groups=1, base_width=64):
        super().__init__()
        width = int(planes * (base_width / 64.0)) * groups
        self.conv1 = _c1(inplanes, width)
        self.bn1 = BatchNorm2d(width)
        self.conv2 = Conv2d(width, width, 3, stride, 1, groups=groups, bias=False)
        self.bn2 = BatchNorm2d(width)
        self.conv3 = _c1(width, planes * 4)
        self.bn3 = BatchNorm2d(planes * 4)
        self.relu = nn.ReLU(inplace=True)
        self.downsample = downsample
        self.stride = stride

    def run(self, cx, x):
        o = conv_bn_act(cx, x, self.conv1, self.bn1)
        o = conv_bn_act(cx, o, self.conv2, self.bn2, private_in=True)
        idt = x if self.downsample is None else conv_bn_act(cx, x, self.downsample[0], self.downsample[1], relu=False)
        return conv_bn_act(cx, o, self.conv3, self.bn3, relu=True, residual=idt)


_ENC = {  # name -> (block, layers, groups, width_per_group)
    "ResNet18": (BasicBlock, [2, 2, 2, 2], 1, 64), "ResNet34": (BasicBlock, [3, 4, 6, 3], 1, 64),
    "ResNet50": (Bottleneck, [3, 4, 6, 3], 1, 64), "ResNet101": (Bottleneck, [3, 4, 23, 3], 1, 64),
    "ResNeXt50": (_GroupedBottleneck, [3, 4, 6, 3], 32, 4), "ResNeXt101": (_GroupedBottleneck, [3, 4, 23, 3], 32, 8),
}


class Encoder(nn.Module):
    """conv1/bn1/relu/maxpool/layer1..4 of a torchvision ResNet(-XT); run() returns the 4 stage outputs"""

    def __init__(self, name, config=None):
        super().__init__()
        block, layers, groups, wpg = _ENC[name]
        self.pretrained = (config or {}).get("pretrained", False)
        self._inplanes = 64
        self.conv1 = Conv2d(3, 64, 7, 2, 3, bias=False)
        self.conv1.stem = True
        self.bn1 = BatchNorm2d(64)
        self.relu = nn.ReLU(inplace=True)
        self.maxpool = nn.MaxPool2d(3, 2, 1)
        for i, (planes, n) in enumerate(zip([64, 128, 256, 512], layers)):
            setattr(self, "layer%d" % (i + 1), self._make_layer(block, planes, n, 1 if i == 0 else 2, groups, wpg))
        nn.Linear(512 * block.expansion, 1000)  # torchvision's fc (RNG parity), dropped
        for m in self.modules():
            if isinstance(m, nn.Conv2d):
                nn.init.kaiming_normal_(m.weight, mode="fan_out", nonlinearity="relu")
            elif isinstance(m, nn.BatchNorm2d):
                nn.init.constant_(m.weight, 1)
                nn.init.constant_(m.bias, 0)
        if self.pretrained:                 # models/ResNet.py:32-33: torchvision's ImageNet checkpoint
            load_pretrained_trunk(self, name, config)

    def _make_layer(self, block, planes, blocks, stride, groups, wpg):
        downsample = None
        if stride != 1 or self._inplanes != planes * block.expansion:
            downsample = nn.Sequential(_c1(self._inplanes, planes * block.expansion, stride), BatchNorm2d(planes * block.expansion))
        kw = dict(groups=groups, base_width=wpg) if block is _GroupedBottleneck else {}
        layers = [block(self._inplanes, planes, stride, downsample, **kw)]
        self._inplanes = planes * block.expansion
        for _ in range(1, blocks):
            layers.append(block(self._inplanes, planes, **kw))
        return nn.Sequential(*layers)

    def out_channels(self):
        outs = []
        for i in range(1, 5):
            blk = getattr(self, "layer%d" % i)[-1]
            outs.append((blk.conv3 if hasattr(blk, "conv3") else blk.conv2).out_channels)
        return outs

    def run(self, cx, x):
        x = conv_bn_act(cx, x, self.conv1, self.bn1, need_dx=False)
        x = maxpool(cx, x)
        outs = []
        for i in range(1, 5):
            for blk in getattr(self, "layer%d" % i):
                x = blk.run(cx, x)
            outs.append(x)
        return outs


def _cbr3(cin, cout):
    return nn.Sequential(Conv2d(cin, cout, 3, 1, 1, bias=False), BatchNorm2d(cout), nn.ReLU(inplace=True))


class UPerNet(nn.Module):
    def __init__(self, config, experiment):
        super().__init__()
        self.num_classes = num_classes(experiment)
        self.pool_scales = config.get("pool_scales", [1, 2, 3, 6])
        self.in_channels = config["input_channels"]
        self.in_scales = config["input_scales"]
        self.ppm_num_ch = config.get("ppm_num_ch", 512)
        self.fpn_num_ch = config.get("fpn_num_ch", 512)
        self.fpn_num_lvl = min(max(config.get("fpn_num_lvl", len(self.in_scales)), 1), len(self.in_scales))
        self.interpolate_result_up = config.get("interpolate_result_up", True)
        self.ppm_pooling = nn.ModuleList([nn.AdaptiveAvgPool2d(s) for s in self.pool_scales])
        self.ppm_conv = nn.ModuleList([nn.Sequential(Conv2d(self.in_channels[-1], self.ppm_num_ch, 1, bias=False),
                                                     BatchNorm2d(self.ppm_num_ch), nn.ReLU(inplace=True))
                                       for _ in self.pool_scales])
        self.ppm_last_conv = _cbr3(self.in_channels[-1] + len(self.pool_scales) * self.ppm_num_ch, self.fpn_num_ch)
        self.fpn_in = nn.ModuleList([nn.Sequential(Conv2d(c, self.fpn_num_ch, 1, bias=False), BatchNorm2d(self.fpn_num_ch),
                                                   nn.ReLU(inplace=True)) for c in self.in_channels[-self.fpn_num_lvl:-1]])
        self.fpn_out = nn.ModuleList([nn.Sequential(_cbr3(self.fpn_num_ch, self.fpn_num_ch)) for _ in range(self.fpn_num_lvl - 1)])
        self.conv_last = nn.Sequential(_cbr3(self.fpn_num_lvl * self.fpn_num_ch, self.fpn_num_ch),
                                       Conv2d(self.fpn_num_ch, self.num_classes, 1))

    def run(self, cx, conv_out):
        conv5 = conv_out[-1]
        B, h, w, c5 = conv5.shape
        npp, pc = len(self.pool_scales), self.ppm_num_ch
        cat = torch.empty((B, h, w, c5 + npp * pc), dtype=torch.float32, device=conv5.device)
        parts = [(copy_into(cx, conv5, cat[..., :c5]), 0, c5)]
        for k, (s, conv) in enumerate(zip(self.pool_scales, self.ppm_conv)):
            up = bilinear(cx, adaptive_avgpool(cx, conv5, s), h, w, False)
            c0 = c5 + k * pc
            parts.append((conv_bn_act(cx, up, conv[0], conv[1], out=cat[..., c0:c0 + pc]), c0, c0 + pc))
        concat_views(cx, cat, parts)
        feature = conv_bn_act(cx, cat, self.ppm_last_conv[0], self.ppm_last_conv[1])
        fpn = [feature]
        for i in range(2, self.fpn_num_lvl + 1):
            lat = self.fpn_in[-i + 1]
            conv_x = conv_bn_act(cx, conv_out[-i], lat[0], lat[1])
            feature = add_n(cx, [conv_x, bilinear(cx, feature, conv_x.shape[1], conv_x.shape[2], False)], relu=False)
            fo = self.fpn_out[-i + 1][0]
            fpn.append(conv_bn_act(cx, feature, fo[0], fo[1]))
        fpn.reverse()
        H, W = fpn[0].shape[1:3]
        fc = self.fpn_num_ch
        fus = torch.empty((B, H, W, self.fpn_num_lvl * fc), dtype=torch.float32, device=conv5.device)
        parts = [(copy_into(cx, fpn[0], fus[..., :fc]), 0, fc)]
        for i in range(2, self.fpn_num_lvl + 1):
            c0 = (i - 1) * fc
            parts.append((bilinear(cx, fpn[-i + 1], H, W, False, out=fus[..., c0:c0 + fc]), c0, c0 + fc))
        concat_views(cx, fus, parts)
        y = conv_bn_act(cx, fus, self.conv_last[0][0], self.conv_last[0][1])
        x = conv_bias(cx, y, self.conv_last[1])
        if self.interpolate_result_up:
            sc = self.in_scales[-self.fpn_num_lvl]
            x = bilinear(cx, x, H * sc, W * sc, False)
        return x


POINTREND_TRAINING_REFUSAL = ("PointRend's train-mode forward runs on the accelerated path only where the configuration asks for it with "
                              "config['decoder']['pr_train_on_device'] = True: the random point sampling "
                              "(get_uncertain_point_coords_with_randomness) then draws from the device generator (engine.PointSampler), not "
                              "from torch.rand, so a run does not reproduce the reference's points; the point cross-entropy loss and the "
                              "backward of the point gather are HIP kernels.  Without the key only the eval-mode forward (model.eval(): "
                              "validation, inference, Ensemble member, TTA, demo_infer) runs")


class StandardPointHead(nn.Module):
    """models/PointRend.py:93-141 of the reference: num_fc layers nn.Conv1d(kernel_size=1) + ReLU over the points, the coarse logits
    concatenated to every layer's input, and the predictor.  The parameters keep the reference's shapes [out, in, 1]; the layers run as
    1 x 1 convolutions over the N k points (ops.pointrend_refine)."""

    def __init__(self, config, num_classes):
        super().__init__()
        self.num_classes = num_classes
        self.fc_dim = config.get("ph_fc_dim", 256)
        self.num_fc = config.get("ph_num_fc", 3)
        self.coarse_pred_each_layer = config.get("ph_coarse_in_each_layer", True)
        coarse = num_classes if self.coarse_pred_each_layer else 0
        widths = [sum(config["input_channels"]) + num_classes] + [self.fc_dim + coarse] * self.num_fc      # input width of fc1 .. fcN, predictor
        for i, cin in enumerate(widths[:-1], 1):
            setattr(self, "fc%d" % i, nn.Conv1d(cin, self.fc_dim, 1))
        self.predictor = nn.Conv1d(widths[-1], num_classes, 1)
        nn.init.normal_(self.predictor.weight, std=0.001)      # (the reference's start: point logits near zero)
        nn.init.zeros_(self.predictor.bias)
        self._images = {}       # zero-padded device images of the weights (ops.pointrend_refine), per parameter version

    @property
    def fc_layers(self):
        return [getattr(self, "fc%d" % i) for i in range(1, self.num_fc + 1)]

    def tensors(self):
        """the head as ops.pointrend_refine takes it (detached parameters: they share the parameters' version counters)"""
        pair = lambda m: (m.weight.detach(), m.bias.detach())
        return {"fc": [pair(fc) for fc in self.fc_layers], "predictor": pair(self.predictor), "coarse_in_each_layer": self.coarse_pred_each_layer,
                "images": self._images}


class PointRend(nn.Module):
    """models/PointRend.py:8-90 of the reference.  Eval mode: UPerNet's logits at 1/s resolution, then log2(s) times upsample x 2, pick the
    pr_subdivision_num_pts most uncertain pixels, re-predict them from point features of the four encoder stages and the coarse logits,
    write them back.  Train mode (config['pr_train_on_device'] = True, a build-side key; refused without it: POINTREND_TRAINING_REFUSAL):
    pr_train_num_pts points per image, int(pr_importance_sample_ratio P) of them the most uncertain of P pr_oversample_ratio uniform
    candidates, the rest uniform; the point head's predictions there, and the x s interpolation of the coarse logits with those
    predictions scattered in (engine.pointrend_train).  The points are the draws of `sampler` (an engine.PointSampler: device-resident
    state, a non-persistent buffer; reseed(); sampler.fixed_points replaces the sampling in tests)."""

    def __init__(self, config, experiment):
        super().__init__()
        self.num_classes = num_classes(experiment)
        if self.num_classes < 2:
            raise ValueError("PointRend's uncertainty is the difference of the two largest logits: it needs at least 2 classes (got %d)" % self.num_classes)
        self.train_num_pts = config["pr_train_num_pts"]
        self.oversample_ratio = config.get("pr_oversample_ratio", 3)
        self.importance_sample_ratio = config.get("pr_importance_sample_ratio", .75)
        self.subdivision_num_pts = config["pr_subdivision_num_pts"]
        self.train_on_device = bool(config.get("pr_train_on_device", False))
        self.in_channels = config["input_channels"]
        self.in_scales = config["input_scales"]
        self.fpn_num_lvl = min(max(config.get("fpn_num_lvl", len(self.in_scales)), 1), len(self.in_scales))
        config["interpolate_result_up"] = False     # the coarse prediction stays at 1/s resolution
        self.partial_upernet = UPerNet(config, experiment)
        self.point_head = StandardPointHead(config, self.num_classes)
        self.sampler = PointSampler()

    def reseed(self, seed, rank=None):
        self.sampler.reseed(seed, rank)

    def run(self, cx, conv_out):
        coarse = self.partial_upernet.run(cx, conv_out)
        scale = self.in_scales[-self.fpn_num_lvl]
        if cx.train:
            if not self.train_on_device:
                raise NotImplementedError(POINTREND_TRAINING_REFUSAL)
            return pointrend_train(cx, coarse, conv_out, self.point_head, self.sampler, self.train_num_pts, self.oversample_ratio,
                                   self.importance_sample_ratio, scale)
        return pointrend_refine(cx, coarse, conv_out, self.point_head.tensors(), self.subdivision_num_pts, int(math.log2(scale)))


_DECODERS = {"UPerNet": UPerNet, "PointRend": PointRend}


class EncDec(EngineNet):
    backbone_modules = ("enc_model",)       # what freeze_bn: "backbone" means here

    def __init__(self, config, experiment):
        super().__init__()
        self.config = config
        self.experiment = experiment
        self.enc_model = Encoder(config["encoder"]["model"], config["encoder"])
        if config["decoder"]["model"] not in _DECODERS:
            raise NotImplementedError("only the UPerNet and PointRend decoders are on the accelerated path")
        config["decoder"]["input_channels"] = self.enc_model.out_channels()
        config["decoder"]["input_scales"] = [4, 8, 16, 32]
        self.dec_model = _DECODERS[config["decoder"]["model"]](config["decoder"], experiment)
        # models/EncDec.py:32-37 of the reference: the projector reads the last encoder stage; deep_features is then its output
        self.projector_model = make_projector(config, self.enc_model.out_channels()[-1])
        self.get_features = True
        self.num_classes = self.dec_model.num_classes
        self.out_stride = 32
        self.apply_freeze_bn(config)

    def forward(self, x):
        if not (self.training and isinstance(self.dec_model, PointRend)):
            return super().forward(x)
        if not self.dec_model.train_on_device:
            raise NotImplementedError(POINTREND_TRAINING_REFUSAL)
        # models/PointRend.py:73 with the encoder's features in front (models/EncDec.py of the reference): (deep_features, point_coords
        # [N, P, 2], point_logits [N, K, P], seg_logits, pred) -- the last two are ONE tensor, as the reference's in-place scatter leaves them
        outs = super().forward(x)
        coords, logits, pred = outs[-3:]
        res = (coords.squeeze(3).permute(0, 2, 1), logits.squeeze(3), pred, pred)
        return (outs[0],) + res if self.get_features else res

    def _body(self, cx, x):
        feats = self.enc_model.run(cx, x)
        pred = self.dec_model.run(cx, feats)
        pred = list(pred) if isinstance(pred, tuple) else [pred]
        if not self.get_features:
            return pred
        deep = feats[-1] if self.projector_model is None else self.projector_model.run(cx, feats[-1])
        return [deep] + pred
