"""`dataprocess.AugData` boundary: Segmenation_Aug (dataprocess/AugData.py:6-38) with the transform itself on the device (csrc/augment2d.hip).

The reference composes albumentations steps - horizontal flip, vertical flip, one of motion / median / box blur, shift-scale-rotate, brightness and
contrast - and runs them per image on the host, offline.  Here the parameters of a sample are drawn on the host (`draw_transform2d`: 16 values of the
global `np.random.random()`, always) and a whole batch - image channels and label together, every sample on its own branch - goes through ONE launch
(`transform_batch2d`), so the same object also runs inside the training loop (`DevicePrefetcher(..., augment=gen)`, `model.augment = gen`).

What is computed is the contract written down at seg_augment2d in include/segengine.h.  It is NOT pinned to albumentations / cv2: neither is
installed where this package is built and tested, so the reference pipeline cannot be executed to record outputs, and its draw order and its uint8
fixed-point interpolation differ between its own versions.  The oracle of the tests (tests/aug2d_oracle.py) is a float64 numpy restatement of that
contract, not a golden file.

One deliberate deviation: float batches are NOT clipped by default.  albumentations clips a float image to [0, 1] after brightness / contrast, which
would destroy z-scored inputs; pass clip=(lo, hi) to get a clip.  The offline tool (uint8 images) uses brightness_scale 255 and clip (0, 255)."""
import math
import os

import numpy as np
import torch

from . import _capi
from .augment import _LABEL_TYPE, _read_csv_rows

__all__ = ["Segmenation_Aug", "draw_transform2d", "make_params2d", "pack_params2d", "transform_batch2d", "affine_matrix2d", "motion_kernel",
           "PARAM_DOUBLES", "BORDER_MODES", "DRAWS_PER_SAMPLE"]

PARAM_DOUBLES = 64                     # SEG_AUGMENT2D_PARAM_DOUBLES
DRAWS_PER_SAMPLE = 16
BORDER_MODES = {"nearest": 0, "constant": 1, "reflect": 2, "wrap": 3, "mirror": 4}
_SUPPORTED = ("mirror", "nearest", "constant")
BLUR_NONE, BLUR_WEIGHTS, BLUR_MEDIAN = 0, 1, 2


def _check_border_mode(mode):
    if mode not in BORDER_MODES:
        raise ValueError("unknown border_mode %r" % (mode,))
    if mode not in _SUPPORTED:
        raise NotImplementedError("border_mode %r is not implemented on the device; supported: 'mirror', 'nearest' and 'constant'" % (mode,))


# ---- parameters (host) ------------------------------------------------------------------------------------------------------------------------------
def affine_matrix2d(angle_deg, scale, dx, dy, size):
    """The 2x3 matrix M the kernel reads, rows (sy, sx) over columns (y, x, 1): the INVERSE of shift o rotate o scale about the centre
    ((w-1)/2, (h-1)/2) of an image of size (h, w), in double.  Forward: p' = scale * R(angle) (p - c) + c + (dx, dy) with p = (x, y) and
    R = [[cos, -sin], [sin, cos]]."""
    h, w = (int(v) for v in size)
    cx, cy = (w - 1) / 2.0, (h - 1) / 2.0
    a = math.radians(float(angle_deg))
    ic, is_ = math.cos(a) / float(scale), math.sin(a) / float(scale)
    tx, ty = cx + float(dx), cy + float(dy)
    return np.array([[ic, -is_, cy - ic * ty + is_ * tx],
                     [is_, ic, cx - ic * tx - is_ * ty]], dtype=np.float64)


def _bresenham(x0, y0, x1, y1):
    """the pixels of the segment (x0, y0) - (x1, y1), both end points included, 8-connected; integers only"""
    dx, dy = abs(x1 - x0), -abs(y1 - y0)
    sx, sy = (1 if x0 < x1 else -1), (1 if y0 < y1 else -1)
    err = dx + dy
    pts = []
    while True:
        pts.append((x0, y0))
        if x0 == x1 and y0 == y1:
            return pts
        e2 = 2 * err
        if e2 >= dy:
            err += dy
            x0 += sx
        if e2 <= dx:
            err += dx
            y0 += sy


def motion_kernel(k, p0, p1):
    """k x k weights of a motion blur: the Bresenham line between the integer end points p0 = (x0, y0) and p1 = (x1, y1) in [0, k-1]^2, each of its
    `count` pixels 1/count.  Coincident points: p1 is replaced by its reflection through the centre (k-1-x1, k-1-y1); when that is still p0 (both are the
    centre) the line is the centre row (0, k//2) - (k-1, k//2)."""
    (x0, y0), (x1, y1) = (int(v) for v in p0), (int(v) for v in p1)
    if (x0, y0) == (x1, y1):
        x1, y1 = k - 1 - x1, k - 1 - y1
    if (x0, y0) == (x1, y1):
        x0, y0, x1, y1 = 0, k // 2, k - 1, k // 2
    pts = _bresenham(x0, y0, x1, y1)
    ker = np.zeros((k, k), dtype=np.float64)
    for x, y in pts:
        ker[y, x] = 1.0 / len(pts)
    return ker


def make_params2d(matrix=None, hflip=False, vflip=False, blur=BLUR_NONE, kernel=None, alpha=1.0, beta=0.0, clip=None):
    """One parameter block (PARAM_DOUBLES float64) from given values.  matrix: a (2, 3) M (`affine_matrix2d`) or None for no warp; blur: 0 none,
    1 the k x k `kernel` (k 3, 5 or 7), 2 the 3 x 3 median; clip: None or (lo, hi)."""
    p = np.zeros(PARAM_DOUBLES, dtype=np.float64)
    p[0:6] = (1.0, 0.0, 0.0, 0.0, 1.0, 0.0)
    if matrix is not None:
        m = np.asarray(matrix, dtype=np.float64)
        if m.shape != (2, 3):
            raise ValueError("a 2-D transform is a (2, 3) matrix, got %s" % (m.shape,))
        p[0:6] = m.reshape(6)
        p[7] = 1.0
    p[6] = (1 if hflip else 0) + (2 if vflip else 0)
    p[8] = int(blur)
    if int(blur) == BLUR_WEIGHTS:
        ker = np.asarray(kernel, dtype=np.float64)
        if ker.ndim != 2 or ker.shape[0] != ker.shape[1] or ker.shape[0] not in (3, 5, 7):
            raise ValueError("a blur kernel is k x k with k 3, 5 or 7, got %s" % (ker.shape,))
        p[9] = ker.shape[0]
        flat = ker.reshape(-1)
        p[16:16 + min(flat.size, 48)] = flat[:48]
        if flat.size == 49:                # 16 + 49 is one more than the block holds: the last weight of a 7 x 7 kernel lives in slot 15
            p[15] = flat[48]
    p[10], p[11] = float(alpha), float(beta)
    if clip is not None:
        p[12], p[13], p[14] = 1.0, float(clip[0]), float(clip[1])
    return p


def draw_transform2d(aug, size):
    """One draw of `aug` (a Segmenation_Aug) for an image of size (h, w): one PARAM_DOUBLES block.  ALWAYS consumes exactly 16 values u1..u16 of the
    global np.random.random(), whichever steps they switch on, so a seeded run is reproducible and the 17th value is what the caller sees next:
       u1   horizontal flip when u1 < hflip_p                      u2   vertical flip when u2 < vflip_p
       u3   a blur when u3 < blur_p; then t = u3 / blur_p in [0, 1) picks motion / median / box by the cumulative normalised inner weights
       u4   motion k = (3, 5, 7)[min(int(3*u4), 2)]                u5..u8   motion end points x0, y0, x1, y1 = min(int(k*u), k-1)  (`motion_kernel`)
       u9   shift-scale-rotate when u9 < affine_p                  u10  angle = (2*u10 - 1) * rotate_limit degrees
       u11  scale = 1 + (2*u11 - 1) * scale_limit                  u12  dx = (2*u12 - 1) * shift_limit * w      u13  dy = (2*u13 - 1) * shift_limit * h
       u14  brightness / contrast when u14 < brightness_contrast_p
       u15  alpha = 1 + (2*u15 - 1) * contrast_limit               u16  beta = (2*u16 - 1) * brightness_limit * brightness_scale
    The box blur is 3 x 3 with weights 1/9.  M = `affine_matrix2d`.  clip is set on every sample when the generator has one."""
    h, w = (int(v) for v in size)
    u = [np.random.random() for _ in range(DRAWS_PER_SAMPLE)]
    blur, kernel = BLUR_NONE, None
    if u[2] < aug.blur_p:
        t = u[2] / aug.blur_p
        total = float(aug.motion_weight + aug.median_weight + aug.box_weight)
        if total > 0:
            if t * total < aug.motion_weight:
                k = (3, 5, 7)[min(int(3 * u[3]), 2)]
                x0, y0, x1, y1 = (min(int(k * v), k - 1) for v in u[4:8])
                blur, kernel = BLUR_WEIGHTS, motion_kernel(k, (x0, y0), (x1, y1))
            elif t * total < aug.motion_weight + aug.median_weight:
                blur = BLUR_MEDIAN
            else:
                blur, kernel = BLUR_WEIGHTS, np.full((3, 3), 1.0 / 9.0)
    matrix = None
    if u[8] < aug.affine_p:
        matrix = affine_matrix2d((2 * u[9] - 1) * aug.rotate_limit, 1 + (2 * u[10] - 1) * aug.scale_limit, (2 * u[11] - 1) * aug.shift_limit * w,
                                 (2 * u[12] - 1) * aug.shift_limit * h, (h, w))
    alpha, beta = 1.0, 0.0
    if u[13] < aug.brightness_contrast_p:
        alpha = 1 + (2 * u[14] - 1) * aug.contrast_limit
        beta = (2 * u[15] - 1) * aug.brightness_limit * aug.brightness_scale
    return make_params2d(matrix, u[0] < aug.hflip_p, u[1] < aug.vflip_p, blur, kernel, alpha, beta, aug.clip)


def pack_params2d(blocks, out=None):
    """parameter blocks (`draw_transform2d` / `make_params2d`) -> the (N, PARAM_DOUBLES) float64 array seg_augment2d reads (written into `out` if given)"""
    b = np.asarray(blocks, dtype=np.float64)
    if b.ndim == 1:
        b = b[None]
    if b.ndim != 2 or b.shape[1] != PARAM_DOUBLES:
        raise ValueError("a parameter block has %d doubles, got %s" % (PARAM_DOUBLES, b.shape))
    if out is None:
        return np.ascontiguousarray(b)
    out[:] = b
    return out


# ---- the launch ---------------------------------------------------------------------------------------------------------------------------------------
def _layout2d(x, layout):
    if x.dim() != 4:
        raise ValueError("a 2-D batch is (N, C, H, W) ['th'] or (N, H, W, C) ['tf'], got %s" % (tuple(x.shape),))
    if layout == "th":
        n, c, h, w = x.shape
        return n, c, h, w, h * w, 1
    if layout == "tf":
        n, h, w, c = x.shape
        return n, c, h, w, 1, c
    raise ValueError('layout should be "tf" (channel last) or "th" (channel first), got %r' % (layout,))


def transform_batch2d(x, params, label=None, layout="th", border_mode="mirror", cval=0.0, label_cval=0.0, params_dev=None):
    """The building block on device tensors: x float32 batch in `layout`, params the (N, PARAM_DOUBLES) float64 numpy array (`pack_params2d`), label
    None or a uint8 / int64 / float32 batch (N, H, W).  One launch for the whole batch.  A batch of ONE image with N > 1 parameter blocks gives the N
    variants of that image (and of its label) without copies of the source.  params_dev: the array already on the device (a non-blocking upload from
    pinned memory), else it is uploaded here.  Returns (out, label_out); label_out is None without a label."""
    _check_border_mode(border_mode)
    if x.dtype != torch.float32:
        raise TypeError("images must be float32, got %s" % x.dtype)
    x = x.contiguous()
    nx, c, h, w, xs_c, xs_v = _layout2d(x, layout)
    params = np.ascontiguousarray(params, dtype=np.float64)
    if params.ndim != 2 or params.shape[1] != PARAM_DOUBLES or (nx != 1 and params.shape[0] != nx):
        raise ValueError("params must be (%d, %d), got %s" % (nx, PARAM_DOUBLES, params.shape))
    n = params.shape[0]
    xs_n = c * h * w if nx == n else 0
    dev = x.device
    lib = _capi.lib_for(dev)
    lab = lab_out = None
    lt = 0
    if label is not None:
        if label.dtype not in _LABEL_TYPE:
            raise TypeError("labels must be uint8, int64 or float32 on the device, got %s" % label.dtype)
        if label.device != dev:
            raise ValueError("image and label must live on one device")
        lab = label.contiguous()
        if lab.numel() != nx * h * w:
            raise ValueError("label %s does not lie on the grid of image %s" % (tuple(lab.shape), tuple(x.shape)))
        lt = _LABEL_TYPE[lab.dtype]
        lab_out = torch.empty((n,) + tuple(lab.shape[1:]), dtype=lab.dtype, device=dev)
    out = torch.empty((n,) + tuple(x.shape[1:]), dtype=torch.float32, device=dev)
    lib.check(lib.seg_augment2d_ws_bytes(n), "seg_augment2d_ws_bytes")          # (no workspace today)
    if params_dev is None:
        params_dev = torch.from_numpy(params).to(dev)
    lib.check(lib.seg_augment2d(x.data_ptr(), out.data_ptr(), n, c, h, w, xs_n, xs_c, xs_v, lab.data_ptr() if lab is not None else None,
                                lab_out.data_ptr() if lab is not None else None, lt, params.ctypes.data, params_dev.data_ptr(),
                                BORDER_MODES[border_mode], float(cval), float(label_cval), None, _capi.stream_for(dev)), "seg_augment2d")
    return out, lab_out


# ---- the reference's class ----------------------------------------------------------------------------------------------------------------------------
class Segmenation_Aug(object):
    """The reference's class (its spelling), with the settings of its Compose as keyword defaults: flips p 0.5 each; the blur group p 0.2 with inner
    weights motion 0.2 / median 0.1 / box 0.1 (normalised); shift 0.0625, scale 0.2, rotate 45 degrees, p 0.2; brightness 0.3, contrast 0.3, p 0.2; the
    border mirrored without the edge pixel.  brightness_scale: what a brightness fraction is multiplied with - 1.0 for float input (albumentations'
    float convention), 255 on the uint8 offline path.  clip: None (float batches are not clipped, see the module docstring) or (lo, hi)."""

    PARAM_DOUBLES = PARAM_DOUBLES
    ndim = 2

    def __init__(self, hflip_p=0.5, vflip_p=0.5, blur_p=0.2, motion_weight=0.2, median_weight=0.1, box_weight=0.1, shift_limit=0.0625,
                 scale_limit=0.2, rotate_limit=45, affine_p=0.2, brightness_limit=0.3, contrast_limit=0.3, brightness_contrast_p=0.2,
                 border_mode="mirror", cval=0.0, label_cval=0.0, brightness_scale=1.0, clip=None, device=None):
        for name, p in (("hflip_p", hflip_p), ("vflip_p", vflip_p), ("blur_p", blur_p), ("affine_p", affine_p),
                        ("brightness_contrast_p", brightness_contrast_p)):
            if not 0.0 <= p <= 1.0:
                raise ValueError("%s must be a probability, got %r" % (name, p))
        if min(motion_weight, median_weight, box_weight) < 0:
            raise ValueError("the inner blur weights must not be negative")
        if not 0.0 <= scale_limit < 1.0:
            raise ValueError("scale_limit must be in [0, 1), got %r" % (scale_limit,))
        if clip is not None and not float(clip[0]) <= float(clip[1]):
            raise ValueError("clip must be (lo, hi) with lo <= hi, got %r" % (clip,))
        _check_border_mode(border_mode)
        self.hflip_p, self.vflip_p, self.blur_p = hflip_p, vflip_p, blur_p
        self.motion_weight, self.median_weight, self.box_weight = motion_weight, median_weight, box_weight
        self.shift_limit, self.scale_limit, self.rotate_limit, self.affine_p = shift_limit, scale_limit, rotate_limit, affine_p
        self.brightness_limit, self.contrast_limit, self.brightness_contrast_p = brightness_limit, contrast_limit, brightness_contrast_p
        self.border_mode, self.cval, self.label_cval = border_mode, cval, label_cval
        self.brightness_scale = brightness_scale
        self.clip = None if clip is None else (float(clip[0]), float(clip[1]))
        self.device = device

    def augment_batch(self, x, y=None, layout="th", params_buffer=None):
        """A 2-D batch of device tensors - x (N, C, H, W) ['th'] or (N, H, W, C) ['tf'], y None or (N, H, W) - through one draw per sample (in sample
        order) and one launch: what the training loop sees.  params_buffer: a pinned float64 (N, PARAM_DOUBLES) tensor to stage the parameters in
        (uploaded without blocking).  A batch that is not 2-D raises ValueError."""
        n, _, h, w, _, _ = _layout2d(x, layout)
        out = params_buffer.numpy() if params_buffer is not None else None
        params = pack_params2d([draw_transform2d(self, (h, w)) for _ in range(n)], out=out)
        pd = params_buffer.to(x.device, non_blocking=True) if params_buffer is not None else None
        return transform_batch2d(x, params, y, layout, self.border_mode, self.cval, self.label_cval, params_dev=pd)

    def __ImageMaskTransform(self, imagedata, index, number):
        from .model import _io
        dev = torch.device(self.device if self.device is not None else "cuda")
        src_image = np.ascontiguousarray(_io.imread_color(imagedata[0]))                     # (H, W, 3) uint8
        src_mask = np.ascontiguousarray(_io.imread_gray(imagedata[1]))                       # (H, W) uint8
        x = torch.from_numpy(src_image.astype(np.float32))[None].to(dev)                     # uploaded once: the launch reads it `number` times
        y = torch.from_numpy(src_mask.astype(np.uint8))[None].to(dev)
        params = pack_params2d([draw_transform2d(self.__offline, src_mask.shape[:2]) for _ in range(number)])
        out, lab = transform_batch2d(x, params, y, "tf", self.border_mode, self.cval, self.label_cval)
        images = torch.round(out).to(torch.uint8).cpu().numpy()                                # (clipped to [0, 255] in the launch)
        masks = lab.cpu().numpy()
        for i in range(number):
            _io.imwrite(self.aug_path + '/Image/' + str(index) + '_' + str(i) + '.bmp', images[i])
            _io.imwrite(self.aug_path + '/Mask/' + str(index) + '_' + str(i) + '.bmp', masks[i])

    def DataAugmentation(self, filepath, number=100, aug_path=None):
        """AugData.py:31-38: every csv row is (image path, mask path); the image is read as 3 channels, the mask as grey, and `number` variants of the pair
        are written as <aug_path>/Image/<row>_<i>.bmp and <aug_path>/Mask/<row>_<i>.bmp, i = 0 .. number-1.  The variants of a row come from ONE launch
        over the uploaded pair, with brightness_scale 255 and a clip to [0, 255], rounded to nearest and stored as uint8."""
        data = _read_csv_rows(filepath)
        self.aug_path = aug_path
        self.__offline = Segmenation_Aug(**dict(self._settings(), brightness_scale=255.0, clip=(0.0, 255.0)))
        for sub in ('/Image/', '/Mask/'):
            os.makedirs(aug_path + sub, exist_ok=True)
        for index in range(len(data)):
            self.__ImageMaskTransform(data[index], index, number)

    def _settings(self):
        names = ("hflip_p", "vflip_p", "blur_p", "motion_weight", "median_weight", "box_weight", "shift_limit", "scale_limit", "rotate_limit",
                 "affine_p", "brightness_limit", "contrast_limit", "brightness_contrast_p", "border_mode", "cval", "label_cval", "brightness_scale",
                 "clip", "device")
        return {k: getattr(self, k) for k in names}
