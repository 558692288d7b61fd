from .OCR import OCRNet  # noqa: F401
from .DeepLabv3Plus import DeepLabv3, DeepLabv3Plus  # noqa: F401
from .HRNetv2 import HRNetv2  # noqa: F401
from .EncDec import EncDec, PointRend, StandardPointHead, UPerNet  # noqa: F401
from .FCN import FCN  # noqa: F401
from .UNet import UNet  # noqa: F401
from .Ensemble import Ensemble  # noqa: F401
from .Projector import Projector  # noqa: F401
from . import backbone  # noqa: F401
