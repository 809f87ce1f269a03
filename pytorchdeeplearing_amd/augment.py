"""`dataprocess.Augmentation` boundary: ImageDataGenerator3D (dataprocess/Augmentation/images_masks_3dtransform.py:63-368) and DataAug3D
(dataprocess/Augmentation/ImageAugmentation.py:26-75) with the transform itself on the device (csrc/augment.hip).

The reference runs scipy.ndimage.affine_transform(order=0) per channel on the host and therefore multiplies the data set on disk, offline.  Here the
parameters are drawn on the host from the global `np.random` in the reference's order (`draw_transform`: same matrix bit for bit, same generator state
afterwards) and a whole batch - image channels and label together - goes through ONE gather launch (`transform_batch`), so the same generator also runs
inside the training loop (`DevicePrefetcher(..., augment=gen)`, `model.augment = gen`).  order=0 copies input values: the results equal the reference's
exactly (tests/test_augment.py, tests/golden/augment3d.npz).

Fill modes 'nearest' and 'constant'; 'reflect' / 'wrap' and the samplewise / featurewise / ZCA options raise NotImplementedError (the reference has no
`fit`, the last two cannot work there either).  Images are float32 (what the reference's `flow` hands to the transform); labels uint8, int64 or float32 on
the device - numpy labels of other integer / bool dtypes travel through one of those and come back in their own dtype."""
import csv
import os
import threading

import numpy as np
import torch

from . import _capi
from .engine import aligned_empty

__all__ = ["ImageDataGenerator3D", "NumpyArrayIterator", "DataAug3D", "draw_transform", "apply_transform", "transform_batch", "pack_params",
           "PARAM_DOUBLES", "FILL_MODES"]

PARAM_DOUBLES = 24                     # SEG_AUGMENT_PARAM_DOUBLES
FILL_MODES = {"nearest": 0, "constant": 1, "reflect": 2, "wrap": 3}
_SUPPORTED = ("nearest", "constant")
_LABEL_TYPE = {torch.uint8: 0, torch.int64: 2, torch.float32: 3}


def _check_fill_mode(fill_mode):
    if fill_mode not in FILL_MODES:
        raise ValueError("unknown fill_mode %r" % (fill_mode,))
    if fill_mode not in _SUPPORTED:
        raise NotImplementedError("fill_mode %r is not implemented on the device; supported: 'nearest' and 'constant'" % (fill_mode,))


# ---- parameters (host) ------------------------------------------------------------------------------------------------------------------------------
def draw_transform(gen, shape):
    """One draw of `gen.random_transform` (images_masks_3dtransform.py:187-269) for a sample with extents shape[:3] and shape[3] channels (1 when the
    shape has three entries), from the global np.random, in the reference's order: three rotations (if rotation_range), the height / width / depth
    shifts (each if set), ONE uniform(lo, hi, 3) for the zoom (unless both bounds are 1), one uniform per channel (if channel_shift_range != 0), one
    random() per enabled flip in the order horizontal (axis 1), vertical (axis 0), depth (axis 2).
    Returns (matrix, flips, shifts): the centred transform Rx.Ry.Rz.T.Z as a (3, 4) float64 array (bit-equal to the reference's), the flips of axes
    (0, 1, 2) as three bools, the channel shifts as a float64 array (None when channel_shift_range == 0)."""
    n0, n1, n2 = (int(v) for v in shape[:3])
    channels = int(shape[3]) if len(shape) > 3 else 1
    uni = np.random.uniform
    if gen.rotation_range:
        tx_, ty_, tz_ = (np.pi / 180 * uni(-gen.rotation_range, gen.rotation_range) for _ in range(3))
    else:
        tx_ = ty_ = tz_ = 0
    rx = np.array([[1, 0, 0, 0], [0, np.cos(tx_), -np.sin(tx_), 0], [0, np.sin(tx_), np.cos(tx_), 0], [0, 0, 0, 1]])
    ry = np.array([[np.cos(ty_), 0, np.sin(ty_), 0], [0, 1, 0, 0], [-np.sin(ty_), 0, np.cos(ty_), 0], [0, 0, 0, 1]])
    rz = np.array([[np.cos(tz_), -np.sin(tz_), 0, 0], [np.sin(tz_), np.cos(tz_), 0, 0], [0, 0, 1, 0], [0, 0, 0, 1]])
    s0 = uni(-gen.height_shift_range, gen.height_shift_range) * n0 if gen.height_shift_range else 0
    s1 = uni(-gen.width_shift_range, gen.width_shift_range) * n1 if gen.width_shift_range else 0
    s2 = uni(-gen.depth_shift_range, gen.depth_shift_range) * n2 if gen.depth_shift_range else 0
    shift = np.array([[1, 0, 0, s0], [0, 1, 0, s1], [0, 0, 1, s2], [0, 0, 0, 1]])
    if gen.zoom_range[0] == 1 and gen.zoom_range[1] == 1:
        z0, z1, z2 = 1, 1, 1
    else:
        z0, z1, z2 = uni(gen.zoom_range[0], gen.zoom_range[1], 3)
    zoom = np.array([[z0, 0, 0, 0], [0, z1, 0, 0], [0, 0, z2, 0], [0, 0, 0, 1]])
    m = np.dot(np.dot(rx, ry), rz)
    m = np.dot(np.dot(m, shift), zoom)
    o0, o1, o2 = float(n0) / 2 + 0.5, float(n1) / 2 + 0.5, float(n2) / 2 + 0.5          # transform_matrix_offset_center
    to = np.array([[1, 0, 0, o0], [0, 1, 0, o1], [0, 0, 1, o2], [0, 0, 0, 1]])
    back = np.array([[1, 0, 0, -o0], [0, 1, 0, -o1], [0, 0, 1, -o2], [0, 0, 0, 1]])
    m = np.dot(np.dot(to, m), back)
    shifts = None
    if gen.channel_shift_range != 0:
        shifts = np.array([uni(-gen.channel_shift_range, gen.channel_shift_range) for _ in range(channels)], dtype=np.float64)
    f1 = bool(gen.horizontal_flip and np.random.random() < 0.5)
    f0 = bool(gen.vertical_flip and np.random.random() < 0.5)
    f2 = bool(gen.depth_flip and np.random.random() < 0.5)
    return np.ascontiguousarray(m[:3, :], dtype=np.float64), (f0, f1, f2), shifts


def pack_params(matrices, flips=None, shifts=None, out=None):
    """(N, 3, 4) matrices [+ (N, 3) flips of axes 0, 1, 2] [+ (N, C) channel shifts] -> the (N, PARAM_DOUBLES) float64 block seg_augment3d reads"""
    m = np.asarray(matrices, dtype=np.float64)
    if m.ndim == 2:
        m = m[None]
    m = m[:, :3, :]
    if m.shape[1:] != (3, 4):
        raise ValueError("a transform is a (3, 4) or (4, 4) matrix, got %s" % (np.asarray(matrices).shape,))
    n = m.shape[0]
    p = np.zeros((n, PARAM_DOUBLES), dtype=np.float64) if out is None else out
    p[:] = 0.0
    p[:, 0:9] = m[:, :, :3].reshape(n, 9)
    p[:, 9:12] = m[:, :, 3]
    if flips is not None:
        f = np.broadcast_to(np.asarray(flips, dtype=bool).reshape(-1, 3), (n, 3))
        p[:, 12] = f[:, 0] * 1 + f[:, 1] * 2 + f[:, 2] * 4
    if shifts is not None:
        s = np.asarray(shifts, dtype=np.float64)
        s = np.broadcast_to(s.reshape(-1, s.shape[-1]), (n, s.shape[-1]))
        if s.shape[1] > 8:
            raise ValueError("a channel shift needs at most 8 channels")
        p[:, 16:16 + s.shape[1]] = s
    return p


# ---- the launch ---------------------------------------------------------------------------------------------------------------------------------------
def _layout(x, layout):
    if x.dim() != 5:
        raise ValueError("a batch is (N, C, n0, n1, n2) ['th'] or (N, n0, n1, n2, C) ['tf'], got %s" % (tuple(x.shape),))
    if layout == "th":
        n, c, n0, n1, n2 = x.shape
        return n, c, (n0, n1, n2), n0 * n1 * n2, 1
    if layout == "tf":
        n, n0, n1, n2, c = x.shape
        return n, c, (n0, n1, n2), 1, c
    raise ValueError('layout should be "tf" (channel last) or "th" (channel first), got %r' % (layout,))


def transform_batch(x, params, label=None, layout="th", fill_mode="nearest", cval=0.0, label_cval=None, rescale=None, channel_shift=False,
                    params_dev=None):
    """The building block on device tensors: x float32 batch in `layout`, params the (N, PARAM_DOUBLES) float64 numpy block (`pack_params`), label None or
    a uint8 / int64 / float32 batch on the same grid without a channel axis (or shaped like x).  One gather launch for the whole batch; with
    channel_shift the in-place clip(x + u_c, min, max) pass follows.  rescale multiplies the image last (`standardize`).  params_dev: the block already
    on the device (a non-blocking upload from pinned memory), else it is uploaded here.  Returns (out, label_out); label_out is None without a label."""
    _check_fill_mode(fill_mode)
    if x.dtype != torch.float32:
        raise TypeError("images must be float32, got %s" % x.dtype)
    x = x.contiguous()
    n, c, ext, xs_c, xs_v = _layout(x, layout)
    v = ext[0] * ext[1] * ext[2]
    params = np.ascontiguousarray(params, dtype=np.float64)
    if params.shape != (n, PARAM_DOUBLES):
        raise ValueError("params must be (%d, %d), got %s" % (n, PARAM_DOUBLES, params.shape))
    dev = x.device
    lib = _capi.lib_for(dev)
    lab = lab_out = None
    lt, lc = 0, 1
    if label is not None:
        if label.dtype not in _LABEL_TYPE:
            raise TypeError("labels must be uint8, int64 or float32 on the device, got %s" % label.dtype)
        if label.device != dev:
            raise ValueError("image and label must live on one device")
        lab = label.contiguous()
        if lab.numel() == n * v:
            lc = 1
        elif tuple(lab.shape) == tuple(x.shape):
            lc = c
        else:
            raise ValueError("label %s does not lie on the grid of image %s" % (tuple(lab.shape), tuple(x.shape)))
        lt = _LABEL_TYPE[lab.dtype]
        lab_out = torch.empty_like(lab)
    out = torch.empty_like(x)
    nbytes = lib.seg_augment3d_ws_bytes(n)
    lib.check(nbytes, "seg_augment3d_ws_bytes")
    ws = aligned_empty(nbytes, dev)
    if params_dev is None:
        params_dev = torch.from_numpy(params).to(dev)
    stream = _capi.stream_for(dev)
    scale = float(rescale) if rescale else 0.0
    lib.check(lib.seg_augment3d(x.data_ptr(), out.data_ptr(), n, c, ext[0], ext[1], ext[2], xs_c, xs_v,
                                lab.data_ptr() if lab is not None else None, lab_out.data_ptr() if lab is not None else None, lt, lc,
                                params.ctypes.data, params_dev.data_ptr(), FILL_MODES[fill_mode], float(cval),
                                float(cval if label_cval is None else label_cval), scale, 1 if channel_shift else 0, ws.data_ptr(), stream),
              "seg_augment3d")
    if channel_shift:
        lib.check(lib.seg_augment3d_shift(out.data_ptr(), n, c, ext[0], ext[1], ext[2], xs_c, xs_v, params_dev.data_ptr(), scale, ws.data_ptr(), stream),
                  "seg_augment3d_shift")
    return out, lab_out


def _rescale_(x, rescale):
    """x *= (float)rescale in place on the device (the rescale-only form of the shift pass)"""
    lib = _capi.lib_for(x.device)
    if not x.is_contiguous() or x.dtype != torch.float32:
        raise TypeError("standardize needs a contiguous float32 tensor")
    n = x.numel()
    if n:
        lib.check(lib.seg_augment3d_shift(x.data_ptr(), 1, 1, 1, 1, n, n, 1, None, float(rescale), None, _capi.stream_for(x.device)),
                  "seg_augment3d_shift")
    return x


def _host(a, dtype):
    """contiguous array of `dtype` torch may wrap (a read-only array is copied)"""
    a = np.ascontiguousarray(a, dtype=dtype)
    return a if a.flags.writeable else a.copy()


def _image_in(x, device):
    """numpy / tensor image -> (float32 tensor on the device, function that brings a result back to the caller's kind)"""
    if isinstance(x, np.ndarray):
        t = torch.from_numpy(_host(x, np.float32)).to(device if device is not None else "cuda")
        return t, lambda r: r.cpu().numpy()
    return x, lambda r: r


def _label_in(y, device):
    if isinstance(y, np.ndarray):
        kind = y.dtype.kind
        if kind == "b" or y.dtype == np.uint8:
            via = np.uint8
        elif kind in "iu":
            via = np.int64
        elif y.dtype in (np.float32, np.float16):
            via = np.float32
        else:
            raise TypeError("label arrays must be bool, integer, float16 or float32, got %s" % y.dtype)
        t = torch.from_numpy(_host(y, via)).to(device if device is not None else "cuda")
        return t, lambda r, dt=y.dtype: r.cpu().numpy().astype(dt, copy=False)
    if y.dtype == torch.bool:
        return y.view(torch.uint8), lambda r: r.view(torch.bool)
    return y, lambda r: r


def apply_transform(x, matrix, flips=(False, False, False), fill_mode="nearest", cval=0.0, label=None, label_cval=None, channel_shift=None, rescale=None,
                    layout="tf", device=None):
    """The deterministic building block: `apply_transform` of the reference (images_masks_3dtransform.py:43-53) for image and label together, followed by
    what `random_transform` / `standardize` do with given draws - the channel shift (values u_c), the flips of axes (0, 1, 2) and the rescale.

    x: one sample (n0, n1, n2, C) or a batch (N, n0, n1, n2, C) in layout 'tf'; (C, n0, n1, n2) / (N, C, n0, n1, n2) in layout 'th'.  matrix: (3, 4) /
    (4, 4), or one per sample.  label: on the same grid, shaped like x or without the channel axis; it gets label_cval (default cval) outside in mode
    'constant'.  numpy in, numpy out (uploaded to `device`, default "cuda"; float32 image); a device tensor in, a device tensor out.
    Returns the image, or (image, label) when a label is given."""
    xt, x_back = _image_in(x, device)
    single = xt.dim() == 4
    if single:
        xt = xt[None]
    n, c, ext, _, _ = _layout(xt, layout)
    params = pack_params(np.broadcast_to(np.asarray(matrix, dtype=np.float64)[..., :3, :], (n, 3, 4)), flips,
                         None if channel_shift is None else channel_shift)
    lt = l_back = None
    if label is not None:
        lt, l_back = _label_in(label, xt.device)
        if single:
            lt = lt[None]
    out, lab = transform_batch(xt, params, lt, layout, fill_mode, cval, label_cval, rescale, channel_shift is not None)
    if single:
        out = out[0]
        lab = lab[0] if lab is not None else None
    if label is None:
        return x_back(out)
    return x_back(out), l_back(lab)


# ---- the reference's classes ------------------------------------------------------------------------------------------------------------------------
class ImageDataGenerator3D(object):
    """The reference's generator (images_masks_3dtransform.py:63-269) with its constructor; see the module docstring for what is not implemented.
    Axes of a sample (n0, n1, n2, C): rows ("height", vertical flip), columns ("width", horizontal flip), depth.  fill_mode and cval apply to image AND
    label, as in the reference; an integer label type must be able to hold cval in mode 'constant'."""

    def __init__(self, featurewise_center=False, samplewise_center=False, featurewise_std_normalization=False, samplewise_std_normalization=False,
                 zca_whitening=False, rotation_range=0., width_shift_range=0., height_shift_range=0., depth_shift_range=0., zoom_range=0.,
                 channel_shift_range=0., fill_mode='nearest', cval=0., horizontal_flip=False, vertical_flip=False, depth_flip=False, rescale=None,
                 preprocessing_function=None, dim_ordering='tf'):
        for name, on in (("featurewise_center", featurewise_center), ("samplewise_center", samplewise_center),
                         ("featurewise_std_normalization", featurewise_std_normalization),
                         ("samplewise_std_normalization", samplewise_std_normalization), ("zca_whitening", zca_whitening)):
            if on:
                raise NotImplementedError("%s is not implemented (the reference has no fit(): its featurewise / ZCA options cannot run either)" % name)
        self.featurewise_center = self.samplewise_center = False
        self.featurewise_std_normalization = self.samplewise_std_normalization = self.zca_whitening = False
        self.rotation_range = rotation_range
        self.width_shift_range = width_shift_range
        self.height_shift_range = height_shift_range
        self.depth_shift_range = depth_shift_range
        self.channel_shift_range = channel_shift_range
        _check_fill_mode(fill_mode)
        self.fill_mode = fill_mode
        self.cval = cval
        self.horizontal_flip = horizontal_flip
        self.vertical_flip = vertical_flip
        self.depth_flip = depth_flip
        self.rescale = rescale
        self.preprocessing_function = preprocessing_function
        if dim_ordering not in {'tf', 'th'}:
            raise ValueError('dim_ordering should be "tf" (channel after row and column) or "th" (channel before row and column). Received arg: ',
                             dim_ordering)
        self.dim_ordering = dim_ordering
        self.mean = self.std = self.principal_components = None
        self.channel_axis, self.row_axis, self.col_axis, self.depth_axis = 4, 1, 2, 3        # (the reference sets them for 'tf' only and uses them always)
        if np.isscalar(zoom_range):
            self.zoom_range = [1 - zoom_range, 1 + zoom_range]
        elif len(zoom_range) == 2:
            self.zoom_range = [zoom_range[0], zoom_range[1]]
        else:
            raise ValueError('zoom_range should be a float or a tuple or list of two floats. Received arg: ', zoom_range)

    def flow(self, X, y=None, batch_size=32, shuffle=True, seed=None, device=None):
        return NumpyArrayIterator(X, y, self, batch_size=batch_size, shuffle=shuffle, seed=seed, dim_ordering=self.dim_ordering, device=device)

    def standardize(self, x):
        """x *= rescale, in place, as the reference does for a float32 sample (numpy: on the host; device tensor: on the device)"""
        if self.rescale:
            if isinstance(x, np.ndarray):
                x *= float(self.rescale)
            else:
                _rescale_(x, self.rescale)
        return x

    def random_transform(self, x, y, device=None):
        """one channel-last sample x (n0, n1, n2, C) and its label y (shaped like x, or without the channel axis) through one random draw"""
        matrix, flips, shifts = draw_transform(self, tuple(x.shape))
        return apply_transform(x, matrix, flips, self.fill_mode, self.cval, label=y, channel_shift=shifts, layout="tf", device=device)

    def augment_batch(self, x, y=None, layout="th", params_buffer=None):
        """A batch of device tensors through one draw per sample (in sample order) and one launch, the rescale included: what `flow` yields and what the
        training loop sees.  params_buffer: a pinned float64 (N, PARAM_DOUBLES) tensor to stage the parameters in (uploaded without blocking)."""
        n, c, ext, _, _ = _layout(x, layout)
        draws = [draw_transform(self, ext + (c,)) for _ in range(n)]
        shift = self.channel_shift_range != 0
        out = params_buffer.numpy() if params_buffer is not None else None
        params = pack_params(np.stack([d[0] for d in draws]), np.array([d[1] for d in draws]), np.stack([d[2] for d in draws]) if shift else None, out=out)
        pd = params_buffer.to(x.device, non_blocking=True) if params_buffer is not None else None
        return transform_batch(x, params, y, layout, self.fill_mode, self.cval, None, self.rescale, shift, params_dev=pd)


class NumpyArrayIterator(object):
    """`ImageDataGenerator3D.flow` (images_masks_3dtransform.py:272-368): the reference's index logic (seed + batches seen before every batch, a
    permutation at batch 0, the short last batch) and float64 numpy batches; every batch is uploaded, transformed in one launch and read back."""

    def __init__(self, x, y, image_data_generator, batch_size=32, shuffle=False, seed=None, dim_ordering='tf', device=None):
        if y is None:
            raise ValueError('flow() transforms images and masks together: y is needed')
        if len(x) != len(y):
            raise ValueError('X (images tensor) and y (labels) should have the same length. Found: X.shape = %s, y.shape = %s' %
                             (np.asarray(x).shape, np.asarray(y).shape))
        self.x = np.asarray(x, dtype=np.float32)
        if self.x.ndim != 5:
            raise ValueError('Input data in `NumpyArrayIterator` should have rank 5. You passed an array with shape', self.x.shape)
        channels_axis = 4 if dim_ordering == 'tf' else 1
        if self.x.shape[channels_axis] not in {1, 3, 4}:
            raise ValueError('NumpyArrayIterator expects 1, 3 or 4 channels on axis %d, got an array with shape %s' % (channels_axis, self.x.shape))
        self.y = np.asarray(y)
        self.image_data_generator = image_data_generator
        self.dim_ordering = dim_ordering
        self.device = torch.device(device if device is not None else "cuda")
        self.n, self.batch_size, self.shuffle = self.x.shape[0], batch_size, shuffle
        self.batch_index = 0
        self.total_batches_seen = 0
        self.lock = threading.Lock()
        self.index_generator = self._flow_index(self.n, batch_size, shuffle, seed)

    def reset(self):
        self.batch_index = 0

    def _flow_index(self, n, batch_size, shuffle, seed):
        self.reset()
        while 1:
            if seed is not None:
                np.random.seed(seed + self.total_batches_seen)
            if self.batch_index == 0:
                index_array = np.random.permutation(n) if shuffle else np.arange(n)
            current_index = (self.batch_index * batch_size) % n
            if n >= current_index + batch_size:
                current_batch_size = batch_size
                self.batch_index += 1
            else:
                current_batch_size = n - current_index
                self.batch_index = 0
            self.total_batches_seen += 1
            yield index_array[current_index: current_index + current_batch_size], current_index, current_batch_size

    def __iter__(self):
        return self

    def __next__(self):
        return self.next()

    def next(self):
        with self.lock:
            index_array, _, _ = next(self.index_generator)
        # the reference transforms the mask as float32 too (label.astype(np.float32)); samples are channel-last whatever dim_ordering says, as there
        xb = torch.from_numpy(self.x[index_array]).to(self.device)
        yb = torch.from_numpy(self.y[index_array].astype(np.float32)).to(self.device)
        xo, yo = self.image_data_generator.augment_batch(xb, yb, layout="tf")
        return xo.cpu().numpy().astype(np.float64), yo.cpu().numpy().astype(np.float64)


def _read_csv_rows(path):
    """the rows of a csv file without its header line, as pandas.read_csv(path).iloc[:, :].values gives them"""
    try:
        import pandas as pd
    except ImportError:
        with open(path, newline="") as f:
            return [row for row in list(csv.reader(f))[1:] if row]
    return pd.read_csv(path).iloc[:, :].values


class DataAug3D(object):
    """transform Image and Mask together (ImageAugmentation.py:26-75): reads the (image.npy, mask.npy) pairs of a csv file and writes `number` augmented
    pairs per row as <aug_path>Image/<row>_<i>.npy (float64) and <aug_path>Mask/<row>_<i>.npy (uint8), i = 1 .. number."""

    def __init__(self, rotation=5, width_shift=0.01, height_shift=0.01, depth_shift=0.01, zoom_range=0.01, rescale=1.1, horizontal_flip=True,
                 vertical_flip=False, depth_flip=False, device=None):
        self.device = device
        self.__datagen = ImageDataGenerator3D(rotation_range=rotation, width_shift_range=width_shift, height_shift_range=height_shift,
                                              depth_shift_range=depth_shift, zoom_range=zoom_range, rescale=rescale, horizontal_flip=horizontal_flip,
                                              vertical_flip=vertical_flip, depth_flip=depth_flip, fill_mode='nearest')

    def __ImageMaskTranform(self, images_path, index, number):
        image = np.load(images_path[0])
        mask = np.load(images_path[1])
        shape = tuple(image.shape[:3])
        srcimage = image.reshape((1,) + shape + (1,))
        srcmask = mask.reshape((1,) + tuple(mask.shape[:3]) + (1,))
        i = 0
        for batchx, batchy in self.__datagen.flow(srcimage, srcmask, device=self.device):
            i += 1
            np.save(self.aug_path + 'Image/' + str(index) + '_' + str(i) + ".npy", batchx[0].reshape(shape))
            np.save(self.aug_path + 'Mask/' + str(index) + '_' + str(i) + ".npy", batchy[0].reshape(mask.shape[:3]).astype('uint8'))
            if i > number - 1:
                break

    def DataAugmentation(self, filepathX, number=100, aug_path=None):
        data = _read_csv_rows(filepathX)
        self.aug_path = aug_path
        for sub in ('Image/', 'Mask/'):
            os.makedirs(os.path.dirname(aug_path + sub), exist_ok=True)
        for index in range(len(data)):
            self.__ImageMaskTranform(data[index], index, number)
