"""`model.metric` boundary: dice_coeff / iou_coeff / multiclass_dice_coeff /
multiclass_iou_coeff of model/metric.py:146-215 (threshold 0.5, per-sample, mean over batch; the
multi-class variants skip the background class), computed by one reduction kernel; Seg_Metirc3d of model/metric.py:11-142 (the nine overlap and
surface-distance numbers a segmentation result is reported with) and its batched form surface_metrics, computed by csrc/surface.hip."""
import math

import numpy as np
import torch

from . import _capi
from .engine import aligned_empty
from .losses import _LABEL_OK


def _metric(probs, target, c):
    p = probs.float().contiguous()
    t = target if target.dtype in _LABEL_OK else target.to(torch.int64)
    t = t.contiguous()
    n = p.shape[0]
    v = p.numel() // (n * c)
    assert t.numel() == n * v
    lib = _capi.lib_for(p.device)
    ws = aligned_empty(8 * 3 * n * c + 256, p.device)
    out2 = torch.zeros(2, dtype=torch.float32, device=p.device)
    lib.check(lib.seg_metric(p.data_ptr(), t.data_ptr(), _capi.LABEL_TYPES[str(t.dtype)], n, c, v, ws.data_ptr(), out2.data_ptr(),
                             _capi.stream_for(p.device)), "seg_metric")
    return out2


def dice_coeff(input, target):
    return _metric(input, target, 1)[0]


def iou_coeff(input, target):
    return _metric(input, target, 1)[1]


def multiclass_dice_coeff(input, target):
    return _metric(input, target, input.shape[1])[0]


def multiclass_iou_coeff(input, target):
    return _metric(input, target, input.shape[1])[1]


def predict_mask(probs, threshold=0.5, scale=255):
    """predict() post-processing on the device (modelVNet.py:670-676, modelUnet.py:672-680): probs (N, C, *spatial) fp32 ->
    uint8 mask (N, *spatial); C == 1: (p > threshold) * scale, C > 1: np.argmax over the class axis (first maximum)."""
    p = probs.float().contiguous()
    n, c = p.shape[0], p.shape[1]
    v = p.numel() // (n * c)
    lib = _capi.lib_for(p.device)
    out = torch.empty((n,) + tuple(p.shape[2:]), dtype=torch.uint8, device=p.device)
    lib.check(lib.seg_predict_mask(p.data_ptr(), out.data_ptr(), n, c, v, float(threshold), int(scale), _capi.stream_for(p.device)),
              "seg_predict_mask")
    return out


SURFACE_METRICS = ("dice", "jaccard", "VOE", "RVD", "FNR", "FPR", "ASSD", "RMSD", "MSD")


def _labels_u8(a, device, binarize):
    """numpy array / torch tensor -> contiguous uint8 tensor; a numpy array is uploaded to `device`, a tensor stays where it is"""
    kind = a.dtype.kind if isinstance(a, np.ndarray) else ("f" if a.dtype.is_floating_point or a.dtype.is_complex else "i")
    if kind not in "biu":
        raise TypeError("masks / label volumes must have a bool or integer dtype, got %s" % a.dtype)
    if isinstance(a, np.ndarray):
        a = torch.from_numpy(np.ascontiguousarray((a != 0) if binarize else a).astype(np.uint8, copy=False)).to(device if device is not None else "cuda")
    elif binarize and a.dtype != torch.uint8:          # (uint8 is binarised by the kernel: cls == -1 reads label != 0)
        a = a != 0
    return a.to(torch.uint8).contiguous()


def _surface_call(lib, real, pred, cls, spacing_zyx, ws, out16, nn_r=None, nn_p=None):
    d, h, w = real.shape
    lib.check(lib.seg_surface_metrics(real.data_ptr(), pred.data_ptr(), d, h, w, int(cls), spacing_zyx[0], spacing_zyx[1], spacing_zyx[2],
                                      ws.data_ptr(), out16.data_ptr(), nn_r.data_ptr() if nn_r is not None else None,
                                      nn_p.data_ptr() if nn_p is not None else None, _capi.stream_for(real.device)), "seg_surface_metrics")


def _surface_ws(lib, shape, device):
    nbytes = lib.seg_surface_ws_bytes(*shape)
    lib.check(nbytes, "seg_surface_ws_bytes")
    return aligned_empty(nbytes, device)


def _spacing_zyx(voxel_spacing):
    sp = [float(v) for v in voxel_spacing]
    if len(sp) != 3:
        raise ValueError("voxel_spacing must be (x, y, z)")
    return sp[::-1]                      # model/metric.py:47: the spacing comes as (x, y, z), the array axes are (z, y, x)


class Seg_Metirc3d():
    """The reference's class (model/metric.py:11-142) with its constructor and methods; surfaces, nearest distances and counts are computed on the device.

    real_mask / pred_mask: (D, H, W) numpy arrays or torch tensors of bool or integer dtype, read as `!= 0`.  A numpy array is uploaded to `device`
    (default "cuda"); a tensor is used where it lives.  voxel_spacing is (x, y, z) and is applied reversed, as in the reference.  The constructor
    enqueues one seg_surface_metrics call and reads its 16 numbers back (one synchronisation); ValueError when either mask has no voxel (the reference
    raises ValueError there too, from a broadcast).  The per-point arrays are downloaded on first access; until the object goes away it holds the call's
    device workspace (about 24 bytes per voxel).

    get_RVD is computed in signed arithmetic: it returns what the reference returns for bool or signed masks.  With unsigned-integer masks the
    reference's `pred.sum() - real.sum()` wraps around when the prediction is the smaller mask (7.9e16 for a uint8 pair) - that is not reproduced."""

    def __init__(self, real_mask, pred_mask, voxel_spacing, device=None):
        self.real_mask = real_mask
        self.pred_mask = pred_mask
        self.voxel_sapcing = voxel_spacing
        real = _labels_u8(real_mask, device, True)
        pred = _labels_u8(pred_mask, device, True)
        if real.dim() != 3 or real.shape != pred.shape or real.device != pred.device:
            raise ValueError("real_mask and pred_mask must be (D, H, W) volumes of one shape on one device")
        self._zyx = _spacing_zyx(voxel_spacing)
        self._shape = tuple(real.shape)
        dev = real.device
        lib = _capi.lib_for(dev)
        self._ws = _surface_ws(lib, self._shape, dev)
        v = real.numel()
        self._nn = (torch.empty(v, dtype=torch.float32, device=dev), torch.empty(v, dtype=torch.float32, device=dev))
        out16 = torch.empty(16, dtype=torch.float64, device=dev)
        _surface_call(lib, real, pred, -1, self._zyx, self._ws, out16, self._nn[0], self._nn[1])
        self._out = out16.cpu().numpy()                # the one synchronisation
        self._r, self._p, self._inter, self._union, self._nsr, self._nsp = (int(x) for x in self._out[:6])
        if self._r == 0 or self._p == 0:
            raise ValueError("Seg_Metirc3d: %s has no voxel" % ("real_mask" if self._r == 0 else "pred_mask"))
        self._cache = {}

    # ---- per-point results, downloaded on first access
    def _nn_host(self, side):
        key = ("nn", side)
        if key not in self._cache:
            self._cache[key] = self._nn[side][:(self._nsp if side else self._nsr)].cpu().numpy().astype(np.float64)
        return self._cache[key]

    def _pts_host(self, side):
        key = ("pts", side)
        if key not in self._cache:
            d, h, w = self._shape
            off = (4 * d * h * w + 255) // 256 * 256 * side            # include/segengine.h: where the call leaves the two index lists
            n = self._nsp if side else self._nsr
            idx = self._ws[off:off + 4 * n].view(torch.int32).cpu().numpy().astype(np.int64)
            self._cache[("idx", side)] = idx
            zyx = np.stack([idx // (h * w), idx // w % h, idx % w], axis=1)
            self._cache[key] = zyx * np.array(self._zyx).reshape(1, 3)
        return self._cache[key]

    def _surface_indices(self, side):
        """packed linear indices (z*H + y)*W + x of the surface voxels, raster order (int64)"""
        self._pts_host(side)
        return self._cache[("idx", side)]

    real2pred_nn = property(lambda self: self._nn_host(0))
    pred2real_nn = property(lambda self: self._nn_host(1))
    real_mask_surface_pts = property(lambda self: self._pts_host(0))
    pred_mask_surface_pts = property(lambda self: self._pts_host(1))

    # ---- overlap (model/metric.py:68-118), from the integer counts
    def get_dice_coefficient(self):
        return 2 * self._inter / (self._r + self._p), 2 * self._inter, self._r + self._p

    def get_jaccard_index(self):
        return self._inter / self._union

    def get_VOE(self):
        return 1 - self.get_jaccard_index()

    def get_RVD(self):
        return float(self._p - self._r) / float(self._r)

    def get_FNR(self):
        return (self._r - self._inter) / self._union

    def get_FPR(self):
        return (self._p - self._inter) / self._union

    # ---- surface distance (model/metric.py:121-142), from the device-side sums
    def get_ASSD(self):
        return float(self._out[6] + self._out[7]) / (self._nsr + self._nsp)

    def get_RMSD(self):
        return math.sqrt(float(self._out[8] + self._out[9]) / (self._nsr + self._nsp))

    def get_MSD(self):
        return float(max(self._out[10], self._out[11]))


def surface_metrics(real_labels, pred_labels, voxel_spacing, classes, device=None):
    """The nine numbers of Seg_Metirc3d for every (sample, class) of two label volumes (N, D, H, W): one seg_surface_metrics call per pair enqueued on the
    current stream, ONE synchronisation, dict of (N, K) float64 arrays keyed by SURFACE_METRICS.  A class with no voxel in either volume gives NaN in that
    entry (no exception): the form a validation loop over a multi-class data set calls."""
    real = _labels_u8(real_labels, device, False)
    pred = _labels_u8(pred_labels, device, False)
    if real.dim() != 4 or real.shape != pred.shape or real.device != pred.device:
        raise ValueError("real_labels and pred_labels must be (N, D, H, W) volumes of one shape on one device")
    classes = [int(c) for c in classes]
    zyx = _spacing_zyx(voxel_spacing)
    dev = real.device
    lib = _capi.lib_for(dev)
    n, k = real.shape[0], len(classes)
    ws = _surface_ws(lib, tuple(real.shape[1:]), dev)          # the calls run one after the other on the stream: one workspace serves them all
    out = torch.empty((n, k, 16), dtype=torch.float64, device=dev)
    for i in range(n):
        for j, c in enumerate(classes):
            _surface_call(lib, real[i], pred[i], c, zyx, ws, out[i, j])
    o = out.cpu().numpy()
    r, p, inter, union, nsurf = o[..., 0], o[..., 1], o[..., 2], o[..., 3], o[..., 4] + o[..., 5]
    with np.errstate(divide="ignore", invalid="ignore"):
        res = {"dice": 2 * inter / (r + p), "jaccard": inter / union, "VOE": 1 - inter / union, "RVD": (p - r) / r, "FNR": (r - inter) / union,
               "FPR": (p - inter) / union, "ASSD": (o[..., 6] + o[..., 7]) / nsurf, "RMSD": np.sqrt((o[..., 8] + o[..., 9]) / nsurf),
               "MSD": np.maximum(o[..., 10], o[..., 11])}
    empty = (r == 0) | (p == 0)
    return {name: np.where(empty, np.nan, res[name]) for name in SURFACE_METRICS}


def calc_accuracy(input, target):
    """model/metric.py:240-243 as written, on the tensors' device: `sum(input == target) / input.size(0)`.  The reference's binary wrappers call it with
    an (N, 1) tensor of thresholded probabilities and (N,) labels: the comparison BROADCASTS to (N, N) and the count of equal pairs is divided by N, so the
    value is N x (the agreement rate of all pairs), not the accuracy - reproduced, not repaired (the multi-class form compares (N,) with (N,))."""
    n = input.size(0)
    return torch.sum(input == target).sum().float() / n
