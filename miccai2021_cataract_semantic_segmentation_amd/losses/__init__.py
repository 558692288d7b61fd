from .lovasz import LovaszSoftmax  # noqa: F401
from .cross_entropy import CrossEntropyLoss  # noqa: F401
from .ohem import OhemCrossEntropy  # noqa: F401
from .two_scale import TwoScaleLoss  # noqa: F401
from .wrapper import LossWrapper  # noqa: F401
from .overlap import GenDiceLoss, SoftIoU  # noqa: F401
from .focal import FocalLoss  # noqa: F401
from .semi import SemiSupervisedLoss  # noqa: F401
from .contrast import DenseContrastiveLoss  # noqa: F401
