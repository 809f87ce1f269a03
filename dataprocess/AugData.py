from pytorchdeeplearing_amd.augment2d import Segmenation_Aug  # noqa: F401
