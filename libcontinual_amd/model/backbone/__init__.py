from .resnet import *  # noqa: F401,F403
from .vit import ViTZoo, VisionTransformer, vit_pt_imnet, vit_pt_imnet_in21k_adapter  # noqa: F401
from .sinet import SiNet_vit, ViT_lora_co  # noqa: F401
from .clip import CLIP, VisualTransformer, clip  # noqa: F401
