"""Script-facing classification wrappers: Binary/Mutil x ResNet 2d/3d `...Model` classes with the reference's constructor keywords and methods
(model/modelResNet.py:22-859): `trainprocess`, `predict`, `inference`, `clear_GPU_cache`, `_dataloder`, `_loss_function`, `_accuracy_function`.  The
per-batch body of `trainprocess` (modelResNet.py:110-131) runs as ONE engine train step - forward, loss, zero_grad, backward, fused Adam - through
libsegengine (SEG_NET_RESNET); there is no CPU fallback, CPU tensors raise as elsewhere.

Where the reference cannot run as shipped:
  * networks/ResNet3d.py:51 reads an undefined global `prob`; the engine uses p = 0.2, the VNet value;
  * in train mode the reference's `loss.backward()` raises (the in-place dropout overwrites what the in-place ReLU saved); the step here is the
    backward pass of the same function;
  * `_loss_function` compares strings with `is`; `==` is used;
  * `Grad_CAM_Visual` hands `self.model` to visualization.GradCAM, which unpacks (logits, softmax, argmax) from `model(x)` - ResNet2d.forward returns the
    logits alone, so the call raises; the map here is the one the class computes when handed that triple (tests/golden/gradcam_2d.npz).
Reproduced as written: `calc_accuracy` on the binary wrappers' (N, 1) against (N,) tensors (see metric.calc_accuracy); `optim.Adam` (coupled weight
decay 0); the checkpoint is written whenever the epoch-mean validation accuracy improves."""
import os
import threading
import time
from pathlib import Path

import numpy as np
import torch
from torch.utils.data import DataLoader

from .. import _capi, metric as M, networks
from . import _io
from .dataset import datasetModelClassifywithnpy, datasetModelClassifywithopencv
from .visualization import GradCAM, plot_result

_LOSSES = {True: ("BinaryCrossEntropyLoss", "BinaryFocalLoss"), False: ("MutilCrossEntropyLoss", "MutilFocalLoss")}


class _ClsModel(object):
    _net = None
    _ndim = 3
    _binary = True
    _pth = "model.pth"

    def _init(self, dims, image_channel, numclass, batch_size, loss_name, inference, model_path, use_cuda):
        self.batch_size, self.loss_name, self.accuracyname = batch_size, loss_name, "accu"
        if self._ndim == 3:
            self.image_depth, self.image_height, self.image_width = dims
        else:
            self.image_height, self.image_width = dims
        self.image_channel, self.numclass = image_channel, numclass
        self.alpha = 0.25 if self._binary else [1.] * numclass
        self.gamma = 2
        self.use_cuda = use_cuda
        self.device = torch.device("cuda" if use_cuda else "cpu")
        self.model = self._net(image_channel, numclass)
        self.model.to(device=self.device)
        self._lock = threading.Lock()
        if inference:
            print(f"Loading model {model_path}")
            print(f"Using device {self.device}")
            self.model.load_state_dict(torch.load(model_path, map_location=self.device))
            print("Model loaded!")

    def _dataloder(self, images, labels, shuffle=False):
        if self._ndim == 3:
            dataset = datasetModelClassifywithnpy(images, labels, targetsize=(self.image_channel, self.image_depth, self.image_height, self.image_width))
        else:
            dataset = datasetModelClassifywithopencv(images, labels, targetsize=(self.image_channel, self.image_height, self.image_width))
        return DataLoader(dataset, shuffle=shuffle, batch_size=self.batch_size, num_workers=0, pin_memory=self.device.type == "cuda")

    def _loss_function(self, lossname):
        """the loss module of that name (model/losses.py), as the reference's method returns it; trainprocess itself hands the NAME to the engine's step"""
        from .. import losses as L
        if lossname not in _LOSSES[self._binary]:
            raise ValueError("loss_name must be one of %s" % (_LOSSES[self._binary],))
        if lossname == "BinaryCrossEntropyLoss":
            return L.BinaryCrossEntropyLoss()
        if lossname == "BinaryFocalLoss":
            return L.BinaryFocalLoss(alpha=self.alpha, gamma=self.gamma)
        if lossname == "MutilCrossEntropyLoss":
            return L.MutilCrossEntropyLoss(alpha=self.alpha)
        return L.MutilFocalLoss(alpha=self.alpha, gamma=self.gamma)

    def _accuracy_function(self, accuracyname, input, target):
        if accuracyname == "accu":
            if self.numclass == 1:
                return M.calc_accuracy((input > 0.5).float(), (target > 0.5).float())
            return M.calc_accuracy(torch.argmax(input, 1), target)

    def _step_args(self):
        binary = self._binary
        alpha = None if binary else torch.as_tensor(self.alpha, dtype=torch.float32, device=self.device)
        return dict(focal_alpha=self.alpha if binary else 0.25, focal_gamma=self.gamma, class_alpha=alpha)

    def trainprocess(self, trainimage, trainmask, validationimage, validationmask, model_dir, epochs=50, lr=1e-3):
        print("[INFO] training the network...")
        Path(model_dir).mkdir(parents=True, exist_ok=True)
        MODEL_PATH = os.path.join(model_dir, self._pth)
        if self.loss_name not in _LOSSES[self._binary]:
            raise ValueError("loss_name must be one of %s" % (_LOSSES[self._binary],))
        eng = self.model.engine
        kw = self._step_args()
        train_loader = self._dataloder(trainimage, trainmask, True)
        val_loader = self._dataloder(validationimage, validationmask)
        H = {"train_loss": [], "train_accuracy": [], "valdation_loss": [], "valdation_accuracy": []}
        startTime = time.time()
        best_validation_dsc = 0.0
        writer = _io.SummaryWriter(log_dir=model_dir) if _io.SummaryWriter is not None else None
        for e in range(epochs):
            self.model.train()
            totalTrainLoss, totalTrainAccu, totalValidationLoss, totalValiadtionAccu = [], [], [], []
            for batch in train_loader:
                x = batch["image"].to(self.device).float().contiguous()
                y = batch["label"].to(self.device)
                # forward, loss, zero_grad, backward, optim.Adam step (coupled weight decay 0) as one library call
                out3 = eng.train_step(x, y, self.loss_name, lr=lr, weight_decay=0.0, decoupled=False, mask_mode=_capi.MASKS_RANDOM, **kw)
                totalTrainLoss.append(out3[0].clone())
                totalTrainAccu.append(self._accuracy_function(self.accuracyname, eng._last_probs, y))
            with torch.no_grad():
                self.model.eval()
                for batch in val_loader:
                    x = batch["image"].to(self.device).float().contiguous()
                    y = batch["label"].to(self.device)
                    logits, probs = eng.forward(x, _capi.MASKS_EVAL)
                    out3 = eng.loss_forward(logits, y, self.loss_name, **kw)
                    totalValidationLoss.append(out3[0].clone())
                    totalValiadtionAccu.append(self._accuracy_function(self.accuracyname, probs, y))
            avgTrainLoss = torch.mean(torch.stack(totalTrainLoss))
            avgValidationLoss = torch.mean(torch.stack(totalValidationLoss))
            avgTrainAccu = torch.mean(torch.stack(totalTrainAccu))
            avgValidationAccu = torch.mean(torch.stack(totalValiadtionAccu))
            H["train_loss"].append(avgTrainLoss.cpu().detach().numpy())
            H["valdation_loss"].append(avgValidationLoss.cpu().detach().numpy())
            H["train_accuracy"].append(avgTrainAccu.cpu().detach().numpy())
            H["valdation_accuracy"].append(avgValidationAccu.cpu().detach().numpy())
            print("[INFO] EPOCH: {}/{}".format(e + 1, epochs))
            print("Train loss: {:.5f}, Train accu: {:.5f}, validation loss: {:.5f}, validation accu: {:.5f}".format(
                avgTrainLoss, avgTrainAccu, avgValidationLoss, avgValidationAccu))
            if writer is not None:
                writer.add_scalar("Train/Loss", avgTrainLoss, e + 1)
                writer.add_scalar("Train/accu", avgTrainAccu, e + 1)
                writer.add_scalar("Valid/loss", avgValidationLoss, e + 1)
                writer.add_scalar("Valid/accu", avgValidationAccu, e + 1)
                writer.flush()
            if avgValidationAccu > best_validation_dsc:
                best_validation_dsc = avgValidationAccu
                torch.save(self.model.state_dict(), MODEL_PATH)
        endTime = time.time()
        print("[INFO] total time taken to train the model: {:.2f}s".format(endTime - startTime))
        plot_result(model_dir, H["train_loss"], H["valdation_loss"], "train_loss", "valdation_loss", "loss")
        plot_result(model_dir, H["train_accuracy"], H["valdation_accuracy"], "train_accuracy", "valdation_accuracy", "accuracy")
        self.clear_GPU_cache()

    def predict(self, full_img, out_threshold=0.5):
        """0 / 255 for one class (probability > out_threshold), the arg-max class index otherwise (modelResNet.py:186-210)"""
        self.clear_GPU_cache()
        self.model.eval()
        img = torch.as_tensor(np.asarray(full_img)).float().contiguous().unsqueeze(0).to(device=self.device, dtype=torch.float32)
        with self._lock, torch.no_grad():
            _, probs = self.model.forward_probs(img)
            full_mask_np = probs[0].detach().cpu().squeeze().numpy()
        if self.numclass == 1:
            return (full_mask_np > out_threshold) * 255
        return np.squeeze(np.argmax(full_mask_np, axis=0))

    def inference(self, image):
        if self._ndim == 2:         # modelResNet.py:212-221
            imageresize = _io.resize(np.asarray(image), (self.image_width, self.image_height)) / 255.
            h, w = np.shape(imageresize)[0], np.shape(imageresize)[1]
            return self.predict(np.transpose(np.reshape(imageresize, (h, w, 1)), (2, 0, 1)))
        d, h, w = np.shape(image)[0], np.shape(image)[1], np.shape(image)[2]      # modelResNet.py:638-647
        return self.predict(np.transpose(np.reshape(image, (d, h, w, 1)), (3, 0, 1, 2)))

    def Grad_CAM_Visual(self, full_img, target_category, target_layers):
        """Grad-CAM of one image (C, H, W) / volume (C, D, H, W) (modelResNet.py:419-426): float32 of the input's spatial shape, values in [0, 1].
        target_layers: module objects out of self.model.in_tr, .down_tr32, .down_tr64, .down_tr128, .down_tr256 (visualization.GradCAM); target_category: the
        class index, or None for the arg-max class.  The reference has this method on MutilResNet2dModel only; the other three wrappers and the 3-D maps
        (trilinear resize) are extensions.  The call overwrites the parameter gradients (the reference's GradCAM calls model.zero_grad() too).

        16-bit run dtypes: the channel weights and the weighted sum are cancelling sums at the shallow layers (the raw map of in_tr spans +-2e-3), so 16-bit
        storage of activations and gradients moves single pixels by tenths there - in stock PyTorch under torch.autocast as in the engine.  Measured
        on MI355X against the float64 map (tests/test_gradcam_lowp.py: three test networks, every class; engine / torch.autocast on the same device):
            layer         f16 worst |d|    f16 mean |d|       bf16 worst |d|   bf16 mean |d|
            down_tr256    2.6e-3           -                  6.4e-2           -
            down_tr128    0.10 / 0.13      0.0048 / 0.0051    0.43 / 0.14      0.017 / 0.018
            down_tr64     0.14 / 0.16      0.0089 / 0.0093    0.25 / 0.31      0.027 / 0.027
            down_tr32     0.20 / 0.26      0.014  / 0.014     0.47 / 0.52      0.032 / 0.035
            in_tr         0.36 / 0.31      0.011  / 0.012     0.50 / 0.93      0.023 / 0.027
        For attribution at the shallow layers construct the network with dtype="f32" (SEGENGINE_DTYPE=f32): maps within 4e-6 of float64."""
        if not len(target_layers):
            raise NotImplementedError("Grad_CAM_Visual needs the activation of a target layer and its gradient, and no target layer was given "
                                      "(pass modules of self.model: in_tr, down_tr32, down_tr64, down_tr128, down_tr256)")
        input_tensor = torch.as_tensor(np.asarray(full_img)).float().contiguous().unsqueeze(0).to(device=self.device, dtype=torch.float32)
        with self._lock:
            cam = GradCAM(model=self.model, target_layers=target_layers, use_cuda=self.use_cuda)
            grayscale_cam = cam(input_tensor=input_tensor, target_category=target_category)
        return grayscale_cam[0]

    def clear_GPU_cache(self):
        if self.device.type == "cuda":
            torch.cuda.empty_cache()


class BinaryResNet2dModel(_ClsModel):
    """model/modelResNet.py:22-225"""
    _net, _ndim, _binary, _pth = networks.ResNet2d, 2, True, "BinaryResNet2d.pth"

    def __init__(self, image_height, image_width, image_channel, numclass, batch_size, loss_name="BinaryCrossEntropyLoss", inference=False,
                 model_path=None, use_cuda=True):
        self._init((image_height, image_width), image_channel, numclass, batch_size, loss_name, inference, model_path, use_cuda)


class MutilResNet2dModel(_ClsModel):
    """model/modelResNet.py:228-441"""
    _net, _ndim, _binary, _pth = networks.ResNet2d, 2, False, "MutilResNet2d.pth"

    def __init__(self, image_height, image_width, image_channel, numclass, batch_size, loss_name="MutilFocalLoss", inference=False, model_path=None,
                 use_cuda=True):
        self._init((image_height, image_width), image_channel, numclass, batch_size, loss_name, inference, model_path, use_cuda)


class BinaryResNet3dModel(_ClsModel):
    """model/modelResNet.py:444-651"""
    _net, _ndim, _binary, _pth = networks.ResNet3d, 3, True, "BinaryResNet3d.pth"

    def __init__(self, image_depth, image_height, image_width, image_channel, numclass, batch_size, loss_name="BinaryCrossEntropyLoss", inference=False,
                 model_path=None, use_cuda=True):
        self._init((image_depth, image_height, image_width), image_channel, numclass, batch_size, loss_name, inference, model_path, use_cuda)


class MutilResNet3dModel(_ClsModel):
    """model/modelResNet.py:654-859"""
    _net, _ndim, _binary, _pth = networks.ResNet3d, 3, False, "MutilResNet3d.pth"

    def __init__(self, image_depth, image_height, image_width, image_channel, numclass, batch_size, loss_name="MutilFocalLoss", inference=False,
                 model_path=None, use_cuda=True):
        self._init((image_depth, image_height, image_width), image_channel, numclass, batch_size, loss_name, inference, model_path, use_cuda)
