"""Per-epoch picture dumps (model/visualization.py:9-49 of the reference): loss/accuracy curves and
the predicted / ground-truth mask montages; and GradCAM (visualization.py:112-238) on the engine's feature taps."""
import os

import numpy as np

from . import _io


class GradCAM:
    """Gradient-weighted class activation mapping with the reference's constructor and call (model/visualization.py:112-238), computed on the device by
    the engine (SegEngine.grad_cam -> seg_gradcam) instead of module hooks and numpy / cv2.

    target_layers are MODULE OBJECTS of `model` (a networks.ResNet2d / ResNet3d), as in the reference; each must be one of the five blocks whose output the
    engine exposes - model.in_tr, model.down_tr32, model.down_tr64, model.down_tr128, model.down_tr256 - anything else raises ValueError.  Several layers
    are aggregated as the reference does (mean of the per-layer maps, scaled once more).  reshape_transform is not supported.
    As shipped the reference's class cannot run on its own ResNet2d (it unpacks (logits, softmax, argmax) from a forward that returns the logits alone);
    the map here is what it computes when handed such a triple.  ResNet3d and (N, D, H, W) maps are an extension: the reference resizes with cv2 (2-D)."""

    def __init__(self, model, target_layers, reshape_transform=None, use_cuda=False):
        if reshape_transform is not None:
            raise NotImplementedError("GradCAM: reshape_transform is not supported (the engine's taps are NC[D]HW tensors of a convolutional network)")
        self.model = model.eval()
        self.cuda = use_cuda
        if self.cuda:
            self.model = model.cuda()
        self.target_layers = target_layers
        from ..engine import SegEngine
        named = dict((id(m), n) for n, m in model.named_modules())
        self.names = []
        for layer in target_layers:
            name = named.get(id(layer))
            if name not in SegEngine.FEATURE_NAMES:
                raise ValueError("GradCAM: target layer %s is not one of the modules whose output the engine exposes: %s"
                                 % ("'%s'" % name if name is not None else "(not a module of the model)", ", ".join("model." + n for n in SegEngine.FEATURE_NAMES)))
            self.names.append(name)

    def __call__(self, input_tensor, target_category=None):
        import torch
        eng = self.model.engine
        x = input_tensor.to(device=eng.device, dtype=torch.float32).contiguous()
        cam = eng.grad_cam(x, target_category, self.names)          # None: each sample's arg-max class, from the call's own forward pass
        if target_category is None:
            print(f"category id: {eng.last_cam_categories}")
        return cam.cpu().numpy()

    def __enter__(self):
        return self

    def __exit__(self, exc_type, exc_value, exc_tb):
        return False


def plot_result(model_dir, H_train, H_validation, H_train_name, H_validation_name, labelname):
    try:
        import matplotlib
        matplotlib.use("Agg")
        import matplotlib.pyplot as plt
    except Exception:  # pragma: no cover
        return
    plt.figure()
    plt.plot(H_train, label=H_train_name)
    plt.plot(H_validation, label=H_validation_name)
    plt.title(H_train_name + "," + H_validation_name + " on Dataset")
    plt.xlabel("Epoch #")
    plt.ylabel(labelname)
    plt.legend(loc="lower left")
    plt.savefig(os.path.sep.join([model_dir, H_train_name + "_" + H_validation_name + "plot.png"]))
    plt.close()


def _montage(vol, size):
    h, w = vol.shape[1], vol.shape[2]
    out = np.zeros((h * size[0], w * size[1]))
    for idx, sl in enumerate(vol):
        i, j = idx % size[1], idx // size[1]
        if j >= size[0]:
            break
        out[j * h:j * h + h, i * w:i * w + w] = sl
    return out


def save_images3d(pdmask, gtmask, size, path, pixelvalue=255.0):
    pd = pdmask.detach().cpu().squeeze().numpy()
    gt = gtmask.detach().cpu().squeeze().numpy()
    if pd.ndim == 4:          # multi-class probabilities: show the arg-max label map
        pd = pd.argmax(0)
    _io.imwrite(path + "pdmask.bmp", np.clip(_montage(pd, size) * pixelvalue, 0, 255).astype("uint8"))
    _io.imwrite(path + "gtmask.bmp", np.clip(_montage(gt, size) * pixelvalue, 0, 255).astype("uint8"))


def save_images2d(pdmask, gtmask, path, pixelvalue=255.0):
    pd = pdmask.detach().cpu().squeeze().numpy()
    gt = gtmask.detach().cpu().squeeze().numpy()
    if pd.ndim == 3:
        pd = pd.argmax(0).astype(np.float32)
    elif np.max(gt) == 1:
        pd = (pd > 0.5).astype(np.float32)
    _io.imwrite(path + "pdmask.bmp", np.clip(pd * pixelvalue, 0, 255).astype("uint8"))
    _io.imwrite(path + "gtmask.bmp", np.clip(gt * pixelvalue, 0, 255).astype("uint8"))
