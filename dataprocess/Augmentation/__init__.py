from pytorchdeeplearing_amd.augment import DataAug3D, ImageDataGenerator3D  # noqa: F401
