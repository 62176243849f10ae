from .barlow import BarlowTwinsLoss, barlow_reference  # noqa: F401
from .vicreg import VICRegLoss, vicreg_reference  # noqa: F401
from .swav import SwAVLoss, swav_reference  # noqa: F401
from .moco import MoCoLoss, moco_reference  # noqa: F401
from .nnclr import NNCLRLoss, nnclr_reference  # noqa: F401
from .dino import DINOLoss, dino_reference  # noqa: F401
