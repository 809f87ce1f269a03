"""`model` package surface of the reference (model/__init__.py:1-3): the eight segmentation wrappers (seg_models.py) and the four ResNet
classification wrappers (cls_models.py; model/modelResNet.py of the reference), all backed by the HIP engine, so `from model import *` in the
reference scripts gives twelve working classes; no method of theirs is a stub.  `Grad_CAM_Visual` (modelResNet.py:419-426, there on MutilResNet2dModel
only) is on all four ResNet wrappers, computed on the device from the engine's feature taps (visualization.GradCAM)."""
from .cls_models import BinaryResNet2dModel, BinaryResNet3dModel, MutilResNet2dModel, MutilResNet3dModel
from .seg_models import (BinaryUNet2dModel, BinaryUNet3dModel, BinaryVNet2dModel, BinaryVNet3dModel, MutilUNet2dModel,
                         MutilUNet3dModel, MutilVNet2dModel, MutilVNet3dModel)

__all__ = ["BinaryVNet2dModel", "BinaryVNet3dModel", "MutilVNet2dModel", "MutilVNet3dModel", "BinaryUNet2dModel", "BinaryUNet3dModel",
           "MutilUNet2dModel", "MutilUNet3dModel", "BinaryResNet2dModel", "BinaryResNet3dModel", "MutilResNet2dModel", "MutilResNet3dModel"]
