"""Torch restatement of the ensemble's arithmetic in any dtype (fp64 = the oracle of the GPU tests, fp32 = the calibration of their bar
and, on the CPU, an exact reproduction of the reference fixture): ImageNet normalisation for the UPerNet members, the members'
eval forwards through the oracle's networks, nn.Softmax2d per member, and the merge over the stacked members
(torch.mean(torch.stack(outputs), 0); 'max' = the element-wise maximum)."""
import torch

IMAGENET_MEAN, IMAGENET_STD = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)
# the three members of tests/golden/ensemble.npz, in key order: (name in the ensemble config, member config without 'ckpt')
MEMBERS = (
    ("OCRNet", {"model": "OCRNet", "backbone": "resnet50", "out_stride": 8, "pretrained": False}),
    ("DeepLabv3Plus", {"model": "DeepLabv3Plus", "backbone": "resnet50", "out_stride": 8, "pretrained": False}),
    ("UPerNet", {"model": "UPerNet", "encoder": {"model": "ResNet18", "pretrained": False}, "decoder": {"model": "UPerNet"}}),
)


def member_configs():
    import copy
    return {str(i + 1): dict(copy.deepcopy(cfg), ckpt="member%d" % (i + 1)) for i, (_, cfg) in enumerate(MEMBERS)}


def normalize(x, mean=IMAGENET_MEAN, std=IMAGENET_STD):
    """torchvision.transforms.Normalize on [..., 3, H, W]: tensor.sub_(mean).div_(std)"""
    m = torch.tensor(mean, dtype=x.dtype).view(3, 1, 1)
    s = torch.tensor(std, dtype=x.dtype).view(3, 1, 1)
    return (x - m) / s


def merge(logits, mode="mean"):
    """logits: list of NCHW tensors of one dtype -> merged probabilities NCHW"""
    stacked = torch.stack([torch.softmax(z, 1) for z in logits])
    return torch.mean(stacked, dim=0) if mode == "mean" else torch.max(stacked, dim=0).values


def member_logits(name, S, x):
    """eval forward of one member through the oracle's networks; S, x of the dtype to evaluate in; x is the RAW frame"""
    from oracle import nets as ON, upernet as OU
    with torch.no_grad():
        if name == "OCRNet":
            return ON.ocrnet_forward(S, x, train=False)[1]
        if name == "DeepLabv3Plus":
            return ON.deeplabv3plus_forward(S, x, train=False)
        if name == "UPerNet":
            out = OU.encdec_forward(S, normalize(x), "ResNet18", train=False)
            return out[1] if isinstance(out, (tuple, list)) else out
    raise KeyError(name)


def ensemble_forward(states, x, mode="mean"):
    """normalise -> members -> softmax -> merge; states: one state dict per entry of MEMBERS"""
    return merge([member_logits(name, S, x) for (name, _), S in zip(MEMBERS, states)], mode)


def merge_case_logits(K, M=3):
    """the random member logits of tests/golden/ensemble_merge.npz (stored there as this seed rule + the reference's output)"""
    g = torch.Generator().manual_seed(520 + K)
    return [torch.randn(1, K, 64, 64, generator=g) * 4 for _ in range(M)]
