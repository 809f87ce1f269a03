from pytorchdeeplearing_amd.augment import *  # noqa: F401,F403
