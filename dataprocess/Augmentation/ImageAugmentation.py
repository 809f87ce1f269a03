from pytorchdeeplearing_amd.augment import DataAug3D  # noqa: F401
