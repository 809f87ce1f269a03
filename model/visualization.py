from pytorchdeeplearing_amd.model.visualization import *  # noqa: F401,F403
