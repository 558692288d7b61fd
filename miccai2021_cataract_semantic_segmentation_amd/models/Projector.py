"""The contrastive projection head -- models/Projector.py:6-49 of the reference: ``config['mlp']`` conv + ReLU layers [k, c, s] and a final
1 x 1 convolution to d channels over the trunk's deepest features.  Same keys, assertions, padding (k - s + 1) // 2, parameter names and
``project.N.*`` numbering (the ReLU modules keep their places in the Sequential).  The mlp layers run through engine.conv_act (bias and
ReLU in the convolution's epilogue), the last one through engine.conv_bias; the output is the dense [B, h, w, d] activation, a view of
the first d columns where conv_bias pads the row pitch.

``use_bn: True`` puts a BatchNorm BEHIND the ReLU of every mlp layer; no route of the engine normalises in that position, so it is
refused.  The module also owns the device generator state of the anchors that losses.DenseContrastiveLoss draws (``sampler``: a
non-persistent buffer, the state-dict keys stay the reference's)."""
import torch
from torch import nn

from .. import ops
from ..engine import AnchorSampler, Conv2d, conv_act, conv_bias

USE_BN_REFUSAL = ("Projector(use_bn=True) places a BatchNorm behind the ReLU of every mlp layer (conv -> ReLU -> BatchNorm): no route of the "
                  "accelerated path normalises in that position (conv_bn_act is conv -> BatchNorm -> ReLU); build the projector with "
                  "use_bn: False")


class Projector(nn.Module):
    def __init__(self, config):
        super().__init__()
        self.d = config["d"] if "d" in config else 128
        self.c_in = config["c_in"]
        self.mlp = config["mlp"] if "mlp" in config else []
        self.use_bn = config["use_bn"] if "use_bn" in config else False
        assert isinstance(self.mlp, list), ('config["mlp"] must be [[k_1, c_1, s_1], ., [k_n, c_n, s_n]] or [] '
                                            'k_i is kernel (k_i x k_i) c_i is channels and s_i is stride')
        for layer in self.mlp:
            assert isinstance(layer, list) and (layer[0] < layer[1]), \
                "kernel size is first element of list, got {} {}".format(layer[0], layer[1])
            assert len(layer) == 3 and layer[2] in [1, 2], \
                "must provide list of lists of 3 elements each[kernel, channels, stride] instead {}".format(layer[2])
        if self.use_bn:
            raise NotImplementedError(USE_BN_REFUSAL)
        convs = []
        c_prev = self.c_in
        for (k, c_out, s) in self.mlp:
            convs.append(Conv2d(c_prev, c_out, kernel_size=k, stride=s, padding=(k - s + 1) // 2, bias=True))
            convs.append(nn.ReLU(inplace=True))
            c_prev = c_out
        convs.append(Conv2d(c_prev, self.d, kernel_size=1, stride=1))
        self.project = nn.Sequential(*convs)
        self.sampler = AnchorSampler()

    def reseed(self, seed, rank=None):
        self.sampler.reseed(seed, rank)

    def forward(self, x):  # pragma: no cover
        raise RuntimeError("engine Projector is executed by the owning network, not called directly")

    def run(self, cx, x):
        convs = [m for m in self.project if isinstance(m, Conv2d)]
        if any(m.in_channels % 4 for m in convs[1:]):
            # an mlp width that is no multiple of 4 (the engine's convolutions read multiples of 4 input channels): the layers run on
            # zero-padded copies of their weights (_padded_layer)
            for i, m in enumerate(convs):
                x = _padded_layer(cx, x, m, last=i == len(convs) - 1)
            return x
        for m in convs[:-1]:
            x = conv_act(cx, x, m)
        return conv_bias(cx, x, convs[-1])


def _padded_layer(cx, x, conv, last):
    """conv_act (last: conv_bias) of a layer whose input or output width is no multiple of 4.  x has r4(Cin) channels, the added ones
    exactly zero; the layer runs with its weight zero-padded to [r4(Cout), r4(Cin)] (last: [Cout, r4(Cin)]) and its bias to match, so an
    mlp layer's added outputs are relu(0 + 0) = 0 and feed the next layer's zero weights.  The padded copies are made per pass from the
    parameters (two small fills and copies; the widths the trunks and the reference's configurations use never come here); the backward
    writes the padded gradients and copies the parameters' part out."""
    w, Cout, kh, kw, s, p, d, _, b = ops.conv_args(conv)
    cin, cin_p = w.shape[1], ops.r4(w.shape[1])
    assert x.shape[-1] == cin_p, (tuple(x.shape), cin)
    cout_p = Cout if last else ops.r4(Cout)
    wp = torch.zeros((cout_p, cin_p, kh, kw), dtype=torch.float32, device=x.device).contiguous(memory_format=torch.channels_last)
    wp[:Cout, :cin].copy_(w.data)
    bp = torch.zeros(cout_p, dtype=torch.float32, device=x.device)
    if b is not None:
        bp[:Cout].copy_(b.data)
    cx.claim(w, b)
    if last:
        ld = max(32, ops.r4(Cout))
        z = ops.conv_fwd(x, wp, bp, Cout, kh, kw, s, p, d, zero_to=ld, train=cx.record)
    else:
        z = ops.conv_fwd_fused(x, wp, bp, None, True, cout_p, kh, kw, s, p, d)
    if cx.record:
        def bwd():
            dz = cx.take(z)
            if dz is None:
                return
            if last:
                dy = dz
                if ops.ld_of(dy) % 4:       # (a dense gradient of d columns, d no multiple of 4: re-pitched, as conv_bias does)
                    dy = ops.new_act(dz.shape[0], dz.shape[1], dz.shape[2], Cout, dz.device, ld=ld, zero=True)
                    dy.copy_(dz)
            else:
                dy = ops.relu_bwd(dz, z)
            dwp, dbp = torch.empty_like(wp), torch.empty_like(bp)
            ops.conv_bwd_weight(x, dy, dwp, dbp, kh, kw, s, p, d)
            cx.pgrad(w).copy_(dwp[:Cout, :cin])
            if b is not None:
                cx.pgrad(b).copy_(dbp[:Cout])
            dx, acc = cx.dest(x)
            ops.conv_bwd_data(dy, wp, tuple(x.shape), kh, kw, s, p, d, out=dx, accumulate=acc)
            cx.done(w, b)
        cx.push(bwd)
    return z


def make_projector(config, c_in):
    """what the four constructors share (models/OCR.py:99-105 of the reference): None without the key, else the Projector on c_in channels"""
    if "projector" not in config:
        return None
    config["projector"]["c_in"] = c_in
    return Projector(config["projector"])
