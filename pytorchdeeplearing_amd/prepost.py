"""Device-side pre/post-processing either side of `predict`: the SimpleITK resampling, the two
intensity normalisations and the sliding-window crop / stitch of the reference's `inference` / `inference_patch`
(model/modelVNet.py:678-698, model/modelUnet.py:684-763, dataprocess/utils.py:99-204), as HIP kernels behind the C-ABI
(`seg_op_resample3d`, `seg_op_normalize_*`, `seg_op_gather_patches`, `seg_op_stitch_mask`), and sliding-window inference with
blended class probabilities (`seg_op_gather_windows`, `seg_op_blend_windows`, `seg_op_blend_finalize`).  Volumes are (D, H, W)
torch tensors on the engine's device; no CPU fallback (a CPU tensor raises unless the test-only checker is injected)."""
import numpy as np
import torch

from . import _capi
from .engine import aligned_empty

LINEAR, NEAREST = 0, 1


def _vol(t):
    assert t.dim() == 3, "expected a (D, H, W) volume"
    return t.contiguous()


def resample3d(vol, out_size, step=None, mode=LINEAR):
    """ITK ResampleImageFilter with the identity transform (dataprocess/utils.py:99-145).  out_size = (D, H, W) of the
    result; step = continuous-index step per axis (output spacing / input spacing); default = in_size / out_size, which
    is `resize_image_itkwithsize`.  float32 volumes (linear or nearest) or uint8 masks (nearest)."""
    vol = _vol(vol)
    if vol.dtype not in (torch.float32, torch.uint8):
        vol = vol.float()
    out_size = tuple(int(s) for s in out_size)
    if step is None:
        step = tuple(float(i) / float(o) for i, o in zip(vol.shape, out_size))
    lib = _capi.lib_for(vol.device)
    out = torch.empty(out_size, dtype=vol.dtype, device=vol.device)
    lib.check(lib.seg_op_resample3d(vol.data_ptr(), out.data_ptr(), 0 if vol.dtype == torch.float32 else 1, *vol.shape, *out_size,
                                    float(step[0]), float(step[1]), float(step[2]), int(mode), _capi.stream_for(vol.device)),
              "seg_op_resample3d")
    return out


def spacing_resample_size(in_size, new_spacing, origin_spacing):
    """`resize_image_itk` (dataprocess/utils.py:123-145): newSize = (originSize / (newSpacing / originSpacing)).astype(int);
    returns (out_size, step) per axis in the order the sizes are given."""
    factor = np.array(new_spacing, float) / np.array(origin_spacing, float)
    new_size = (np.array(in_size) / factor).astype(int)
    return tuple(int(s) for s in new_size), tuple(float(f) for f in factor)


def _ws(device):
    lib = _capi.lib_for(device)
    return lib, aligned_empty(lib.seg_op_normalize_ws_bytes(), device)


def normalize_meanstd(vol, lower=None, upper=None):
    """ConvertitkTrunctedValue(image, upper, lower, 'meanstd') (dataprocess/utils.py:148-179)."""
    x = vol.float().contiguous()
    lib, ws = _ws(x.device)
    out = torch.empty_like(x)
    clip = lower is not None and upper is not None
    lib.check(lib.seg_op_normalize_meanstd(x.data_ptr(), out.data_ptr(), x.numel(), 1 if clip else 0, float(lower if clip else 0.0),
                                           float(upper if clip else 0.0), ws.data_ptr(), _capi.stream_for(x.device)), "seg_op_normalize_meanstd")
    return out


def normalize_percentile(vol, bottom=95, down=5):
    """normalize(slice, bottom=95, down=5) (dataprocess/utils.py:182-204)."""
    x = vol.float().contiguous()
    lib, ws = _ws(x.device)
    out = torch.empty_like(x)
    lib.check(lib.seg_op_normalize_percentile(x.data_ptr(), out.data_ptr(), x.numel(), float(down), float(bottom), ws.data_ptr(),
                                              _capi.stream_for(x.device)), "seg_op_normalize_percentile")
    return out


def patch_origins(vol_shape, patch_shape):
    """Window origins of the reference's sliding loop, statement by statement (model/modelUnet.py:718-743).  The loop
    variables already advance in half-patch steps and are then multiplied by the patch size once more, so every window
    after the first is clamped to the far border: the set of windows is {0, size - patch} per axis.  Reproduced as is."""
    D, H, W = (int(s) for s in vol_shape)
    pd, ph, pw = (int(s) for s in patch_shape)
    if pd > D or ph > H or pw > W:
        raise ValueError("inference_patch: the resampled volume %s is smaller than the network patch %s" % ((D, H, W), (pd, ph, pw)))
    seen, out = set(), []
    for z in range(0, D, pd // 2):
        for y in range(0, H, ph // 2):
            for x in range(0, W, pw // 2):
                x_min, x_max = x * pw, (x + 1) * pw
                if x_max > W:
                    x_max, x_min = W, W - pw
                y_min, y_max = y * ph, (y + 1) * ph
                if y_max > H:
                    y_max, y_min = H, H - ph
                z_min, z_max = z * pd, (z + 1) * pd
                if z_max > D:
                    z_max, z_min = D, D - pd
                o = (z_min, y_min, x_min)
                if o not in seen:            # the stitch is idempotent (|=), repeated windows add nothing
                    seen.add(o)
                    out.append(o)
    return out


def gather_patches(vol, origins, patch_shape):
    """(D,H,W) float32 volume + int32 origins (nb, 3) on the device -> (nb, 1, pd, ph, pw) network batch."""
    vol = _vol(vol.float())
    lib = _capi.lib_for(vol.device)
    nb = origins.shape[0]
    out = torch.empty((nb, 1) + tuple(patch_shape), dtype=torch.float32, device=vol.device)
    lib.check(lib.seg_op_gather_patches(vol.data_ptr(), *vol.shape, origins.data_ptr(), nb, *patch_shape, out.data_ptr(),
                                        _capi.stream_for(vol.device)), "seg_op_gather_patches")
    return out


def stitch_mask(masks, origins, out):
    """out[window] = 1 where the window's uint8 mask is non-zero (`out_mask += patch; out_mask[out_mask != 0] = 1`)."""
    masks = masks.contiguous()
    assert masks.dtype == torch.uint8 and out.dtype == torch.uint8 and out.is_contiguous()
    lib = _capi.lib_for(out.device)
    nb = origins.shape[0]
    pshape = tuple(masks.shape[-3:])
    lib.check(lib.seg_op_stitch_mask(masks.data_ptr(), origins.data_ptr(), nb, *pshape, out.data_ptr(), *out.shape,
                                     _capi.stream_for(out.device)), "seg_op_stitch_mask")
    return out


# ---- sliding-window inference with blended probabilities (csrc/sliding.hip); no counterpart in the reference ----

def _axis_starts(n, p, overlap):
    if n <= p:
        return [0]
    step = max(1, int(p * (1.0 - overlap)))
    starts = list(range(0, n - p + 1, step))
    if starts[-1] != n - p:
        starts.append(n - p)
    return starts


def window_origins(vol_shape, patch_shape, overlap=0.5):
    """Origins (z, y, x) of overlapping windows that cover the volume, z-major with x fastest.  Per axis: the single start 0 when the
    volume is not larger than the patch (the window then overhangs and `gather_windows` pads it); otherwise 0, step, 2 * step, ... while
    the window fits, step = max(1, int(patch * (1 - overlap))), plus the start that ends on the far border when the last one does not."""
    if not 0.0 <= overlap < 1.0:
        raise ValueError("overlap must lie in [0, 1), got %r" % (overlap,))
    if len(vol_shape) != 3 or len(patch_shape) != 3:
        raise ValueError("window_origins expects (D, H, W) shapes")
    zs, ys, xs = (_axis_starts(int(n), int(p), float(overlap)) for n, p in zip(vol_shape, patch_shape))
    return [(z, y, x) for z in zs for y in ys for x in xs]


def importance_1d(p, mode="gaussian"):
    """fp32 importance weights along one patch axis: "constant" = ones; "gaussian" = exp(-(i - (p - 1) / 2)^2 / (2 * (0.125 * p)^2)) divided
    by its maximum and floored at 1e-3 (so the weight sum of a covered voxel is never 0).  The blend weight of a window voxel is the product
    of the three axes' values."""
    p = int(p)
    if mode == "constant":
        return np.ones(p, np.float32)
    if mode != "gaussian":
        raise ValueError("blend must be 'constant' or 'gaussian', got %r" % (mode,))
    i = np.arange(p, dtype=np.float64)
    g = np.exp(-(i - (p - 1) / 2.0) ** 2 / (2.0 * (0.125 * p) ** 2))
    return np.maximum(g / g.max(), 1e-3).astype(np.float32)


def _entries(entries, device):
    """window entries {z, y, x, flipbits} as a contiguous int32 (nb, 4) tensor on `device`"""
    e = torch.as_tensor(entries, dtype=torch.int32).to(device).contiguous()
    if e.dim() != 2 or e.shape[1] != 4 or e.shape[0] < 1:
        raise RuntimeError("window entries must be a non-empty (nb, 4) list of {z, y, x, flipbits}")
    return e


def gather_windows(vol, entries, patch_shape, pad_value=0.0):
    """(D, H, W) float32 volume + int32 entries (nb, 4) {z, y, x, flipbits} on the device -> (nb, 1, pd, ph, pw) network batch; bit 0 / 1 / 2
    of flipbits mirrors the window along z / y / x, voxels outside the volume read `pad_value`."""
    vol = _vol(vol.float())
    e = _entries(entries, vol.device)
    lib = _capi.lib_for(vol.device)
    patch_shape = tuple(int(s) for s in patch_shape)
    out = torch.empty((e.shape[0], 1) + patch_shape, dtype=torch.float32, device=vol.device)
    lib.check(lib.seg_op_gather_windows(vol.data_ptr(), *vol.shape, e.data_ptr(), e.shape[0], *patch_shape, float(pad_value), out.data_ptr(),
                                        _capi.stream_for(vol.device)), "seg_op_gather_windows")
    return out


def _f32c(t, device):
    return torch.as_tensor(t, dtype=torch.float32).to(device).contiguous()


def blend_windows(probs, entries, weights, acc, wsum, box=None):
    """acc (C, D, H, W) += w * probs, wsum (D, H, W) += w for the windows of one batch, un-mirrored back into the volume, w = wz[i] * wy[j] * wx[k]
    (`weights` = the three 1-D importance vectors).  probs: (nb, C, pd, ph, pw) fp32.  `box` = ((z0, y0, x0), (z1, y1, x1)), half-open, the voxels
    the launch covers: it must hold every window of the batch (default: the whole volume; `sliding_window_predict` passes the windows' bounding box).
    Deterministic: windows are added in entry order."""
    if probs.dim() != 5 or acc.dim() != 4 or wsum.dim() != 3 or tuple(acc.shape[1:]) != tuple(wsum.shape) or probs.shape[1] != acc.shape[0]:
        raise RuntimeError("blend_windows: expected probs (nb, C, pd, ph, pw), acc (C, D, H, W) and wsum (D, H, W), got %s, %s, %s"
                           % (tuple(probs.shape), tuple(acc.shape), tuple(wsum.shape)))
    if acc.dtype != torch.float32 or wsum.dtype != torch.float32 or not acc.is_contiguous() or not wsum.is_contiguous():
        raise RuntimeError("blend_windows: acc and wsum must be contiguous float32 tensors")
    dev = acc.device
    probs = _f32c(probs, dev)
    e = _entries(entries, dev)
    nb, c, pd, ph, pw = probs.shape
    w3 = [_f32c(w, dev) for w in weights]
    if e.shape[0] != nb or [w.numel() for w in w3] != [pd, ph, pw]:
        raise RuntimeError("blend_windows: %d entries and importance vectors of %s elements for probs %s"
                           % (e.shape[0], [w.numel() for w in w3], tuple(probs.shape)))
    lo, hi = box if box is not None else ((0, 0, 0), tuple(wsum.shape))
    I3 = _capi.C.c_int * 3
    lib = _capi.lib_for(dev)
    lib.check(lib.seg_op_blend_windows(probs.data_ptr(), e.data_ptr(), nb, c, pd, ph, pw, w3[0].data_ptr(), w3[1].data_ptr(), w3[2].data_ptr(),
                                       I3(*(int(v) for v in lo)), I3(*(int(v) for v in hi)), acc.data_ptr(), wsum.data_ptr(), *wsum.shape,
                                       _capi.stream_for(dev)), "seg_op_blend_windows")
    return acc, wsum


def blend_finalize(acc, wsum, threshold=0.5, scale=1, return_probs=False):
    """blended field -> uint8 mask (D, H, W): C == 1: (acc / wsum > threshold) * scale, C > 1: first arg-max over the classes; with
    return_probs also acc / wsum as (C, D, H, W) fp32.  A voxel no window reached (wsum == 0) gives mask 0 and probability 0."""
    if acc.dim() != 4 or tuple(acc.shape[1:]) != tuple(wsum.shape) or acc.dtype != torch.float32 or wsum.dtype != torch.float32:
        raise RuntimeError("blend_finalize: expected float32 acc (C, D, H, W) and wsum (D, H, W), got %s, %s" % (tuple(acc.shape), tuple(wsum.shape)))
    acc, wsum = acc.contiguous(), wsum.contiguous()
    lib = _capi.lib_for(acc.device)
    mask = torch.empty(wsum.shape, dtype=torch.uint8, device=acc.device)
    probs = torch.empty_like(acc) if return_probs else None
    lib.check(lib.seg_op_blend_finalize(acc.data_ptr(), wsum.data_ptr(), acc.shape[0], wsum.numel(), float(threshold), int(scale), mask.data_ptr(),
                                        probs.data_ptr() if return_probs else None, _capi.stream_for(acc.device)), "seg_op_blend_finalize")
    return (mask, probs) if return_probs else mask


def sliding_window_predict(fn, vol, patch, num_class, batch_size=1, overlap=0.5, blend="gaussian", mirror_axes=(), threshold=0.5, scale=1,
                           return_probs=False):
    """Whole-volume prediction from a patch network.  vol: device fp32 (D, H, W); fn: device batch (B, 1, pd, ph, pw) -> class probabilities
    (B, C, pd, ph, pw) fp32.  The entry list is every `window_origins` origin x every subset of `mirror_axes` (0 = z, 1 = y, 2 = x); it runs in
    batches of `batch_size` through gather_windows -> fn -> blend_windows (fn always sees `batch_size` windows when there are more entries than
    that), then blend_finalize: the uint8 mask (D, H, W), with return_probs also the blended probabilities (C, D, H, W).  A 2-D image is
    D = pd = 1."""
    vol = _vol(vol.float())
    patch = tuple(int(s) for s in patch)
    axes = sorted(set(int(a) for a in mirror_axes))
    if any(a not in (0, 1, 2) for a in axes):
        raise ValueError("mirror_axes must be a subset of (0, 1, 2)")
    flips = [sum(1 << a for k, a in enumerate(axes) if s >> k & 1) for s in range(1 << len(axes))]
    entries = [o + (f,) for o in window_origins(vol.shape, patch, overlap) for f in flips]
    weights = [torch.from_numpy(importance_1d(p, blend)).to(vol.device) for p in patch]
    acc = torch.zeros((int(num_class),) + tuple(vol.shape), dtype=torch.float32, device=vol.device)
    wsum = torch.zeros(tuple(vol.shape), dtype=torch.float32, device=vol.device)
    bs = max(1, int(batch_size))
    for s in range(0, len(entries), bs):
        chunk = entries[s:s + bs]
        # a short last batch is filled up with repeats of its last window, so that fn sees ONE batch size (an engine behind fn plans per batch
        # shape); only the first len(chunk) answers are blended
        fed = chunk + [chunk[-1]] * (bs - len(chunk) if len(entries) > bs else 0)
        e = torch.tensor(fed, dtype=torch.int32).to(vol.device)
        probs = fn(gather_windows(vol, e, patch))
        if tuple(probs.shape) != (len(fed), int(num_class)) + patch:
            raise RuntimeError("sliding_window_predict: fn returned %s for a batch of %s" % (tuple(probs.shape), (len(fed), int(num_class)) + patch))
        lo = tuple(min(c[a] for c in chunk) for a in range(3))
        hi = tuple(min(max(c[a] for c in chunk) + patch[a], vol.shape[a]) for a in range(3))
        blend_windows(probs[:len(chunk)], e[:len(chunk)], weights, acc, wsum, (lo, hi))
    return blend_finalize(acc, wsum, threshold, scale, return_probs)


# ---- mask post-processing (dataprocess/utils.py:7-96): connected components and binary morphology, csrc/postproc.hip ----

CC_STATS = 32                # int32 per sample: K, foreground voxels, largest size, its label, its first voxel, its box (6), the foreground box (6), zeros
KEEP_LARGEST, MIN_SIZE = 0, 1
MORPH_OPS = {"dilate": 0, "erode": 1, "open": 2, "close": 3}
SE_SHAPES = {"ball": 0, "box": 1, "cross": 2}
_pp_ws = {}                  # (device, stream) -> the largest workspace asked for so far


def _pp_workspace(device, nbytes):
    key = (str(device), _capi.stream_for(device).value)
    ws = _pp_ws.get(key)
    if ws is None or ws.numel() < nbytes:
        ws = _pp_ws[key] = aligned_empty(nbytes, device)
    return ws


def _pp_mask(mask):
    """device uint8 (D, H, W) or (N, D, H, W) -> (contiguous tensor, (n, d, h, w))"""
    if not torch.is_tensor(mask) or mask.dtype != torch.uint8 or mask.dim() not in (3, 4):
        raise TypeError("expected a uint8 tensor (D, H, W) or (N, D, H, W)")
    mask = mask.contiguous()
    return mask, ((1,) + tuple(mask.shape) if mask.dim() == 3 else tuple(mask.shape))


def _pp_out(mask, out):
    if out is None:
        return torch.empty_like(mask)
    if out.dtype != torch.uint8 or out.shape != mask.shape or out.device != mask.device or not out.is_contiguous():
        raise ValueError("out must be a contiguous uint8 tensor of the mask's shape on its device")
    return out


def _pp_cls(cls):
    return -1 if cls is None else int(cls)


def connected_components(mask, connectivity=1, cls=None, labels=True):
    """Components of the voxels equal to `cls` (None: non-zero) per sample; connectivity 1 = faces, 3 = fully connected.  Returns (labels int32 of the
    mask's shape, numbered 1..K like scipy.ndimage.label; stats int32 (N, 32), see seg_cc_label in include/segengine.h)."""
    mask, nd = _pp_mask(mask)
    lib = _capi.lib_for(mask.device)
    nbytes = lib.seg_cc_ws_bytes(*nd)
    lib.check(nbytes, "seg_cc_ws_bytes")
    ws = _pp_workspace(mask.device, nbytes)
    lab = torch.empty(mask.shape, dtype=torch.int32, device=mask.device) if labels else None
    stats = torch.empty((nd[0], CC_STATS), dtype=torch.int32, device=mask.device)
    lib.check(lib.seg_cc_label(mask.data_ptr(), *nd, _pp_cls(cls), int(connectivity), ws.data_ptr(), lab.data_ptr() if labels else None,
                               stats.data_ptr(), _capi.stream_for(mask.device)), "seg_cc_label")
    return lab, stats


def _cc_filter(mask, mode, min_voxels, connectivity, cls, out):
    mask, nd = _pp_mask(mask)
    out = _pp_out(mask, out)
    lib = _capi.lib_for(mask.device)
    nbytes = lib.seg_cc_ws_bytes(*nd)
    lib.check(nbytes, "seg_cc_ws_bytes")
    ws = _pp_workspace(mask.device, nbytes)
    lib.check(lib.seg_cc_filter(mask.data_ptr(), out.data_ptr(), *nd, _pp_cls(cls), int(connectivity), mode, int(min_voxels), ws.data_ptr(), None,
                                _capi.stream_for(mask.device)), "seg_cc_filter")
    return out


def keep_largest_component(mask, connectivity=1, cls=None, out=None):
    """the input value on the largest component of every sample (ties: the first in raster order), 0 elsewhere; out may be mask"""
    return _cc_filter(mask, KEEP_LARGEST, 0, connectivity, cls, out)


def remove_small_components(mask, min_voxels, connectivity=1, cls=None, out=None):
    """the input value on the components of at least min_voxels voxels, 0 elsewhere; out may be mask"""
    return _cc_filter(mask, MIN_SIZE, min_voxels, connectivity, cls, out)


def foreground_bbox(mask, cls=None):
    """int32 (N, 6) (or (6,) for a (D, H, W) mask) on the device: inclusive z0 y0 x0 z1 y1 x1 of the foreground; {D, H, W, -1, -1, -1} when there is none"""
    _, stats = connected_components(mask, 1, cls, labels=False)
    box = stats[:, 11:17]
    return box[0] if mask.dim() == 3 else box


def binary_morphology(mask, op, radius, shape="ball", border=None, fg_value=1, cls=None, out=None):
    """dilate / erode / open / close of the voxels equal to `cls` (None: non-zero) with a ball, box or cross of `radius` (an int or (rz, ry, rx));
    border = the value outside the volume (None: 0 for a dilation, 1 for an erosion); result fg_value / 0.  scipy.ndimage.binary_dilation /
    binary_erosion with that structure and border_value; out may be mask."""
    mask, nd = _pp_mask(mask)
    out = _pp_out(mask, out)
    if op not in MORPH_OPS or shape not in SE_SHAPES:
        raise ValueError("op must be one of %s and shape one of %s" % (sorted(MORPH_OPS), sorted(SE_SHAPES)))
    r = (int(radius),) * 3 if np.isscalar(radius) else tuple(int(v) for v in radius)
    if len(r) != 3:
        raise ValueError("radius must be an int or (rz, ry, rx)")
    lib = _capi.lib_for(mask.device)
    nbytes = lib.seg_morph3d_ws_bytes(*nd)
    lib.check(nbytes, "seg_morph3d_ws_bytes")
    ws = _pp_workspace(mask.device, nbytes)
    lib.check(lib.seg_morph3d(mask.data_ptr(), out.data_ptr(), *nd, _pp_cls(cls), MORPH_OPS[op], SE_SHAPES[shape], *r, -1 if border is None else int(border),
                              int(fg_value), ws.data_ptr(), _capi.stream_for(mask.device)), "seg_morph3d")
    return out


# ---- exact Euclidean distance transform and the maps of the boundary loss, csrc/edt.hip ----

EDT_SQUARED, EDT_DISTANCE, EDT_SIGNED, EDT_BOUNDARY = 0, 1, 2, 3


def _edt_sampling(sampling, rank=3):
    """None, a scalar or one spacing per spatial axis -> (sz, sy, sx); a 2-D grid is the d = 1 volume"""
    if sampling is None:
        return (1.0, 1.0, 1.0)
    s = (float(sampling),) * rank if np.isscalar(sampling) else tuple(float(v) for v in sampling)
    if len(s) != rank:
        raise ValueError("sampling must be a scalar or one spacing per spatial axis (%d)" % rank)
    return (1.0,) * (3 - rank) + s


def _edt_call(lib, mask, nd, cls, sampling, mode, out_ptr, out_stride):
    nbytes = lib.seg_edt_ws_bytes(*nd)
    lib.check(nbytes, "seg_edt_ws_bytes")
    ws = _pp_workspace(mask.device, nbytes)
    lib.check(lib.seg_edt(mask.data_ptr(), *nd, cls, *sampling, mode, ws.data_ptr(), out_ptr, out_stride, _capi.stream_for(mask.device)), "seg_edt")


def _edt(mask, sampling, cls, mode, out):
    mask, nd = _pp_mask(mask)
    if out is None:
        out = torch.empty(mask.shape, dtype=torch.float32, device=mask.device)
    elif out.dtype != torch.float32 or out.shape != mask.shape or out.device != mask.device or not out.is_contiguous():
        raise ValueError("out must be a contiguous float32 tensor of the mask's shape on its device")
    _edt_call(_capi.lib_for(mask.device), mask, nd, _pp_cls(cls), _edt_sampling(sampling), mode, out.data_ptr(), nd[1] * nd[2] * nd[3])
    return out


def distance_transform_edt(mask, sampling=None, cls=None, squared=False, out=None):
    """scipy.ndimage.distance_transform_edt on the device: for every voxel equal to `cls` (None: non-zero) of a uint8 (D, H, W) or (N, D, H, W) tensor the
    exact Euclidean distance (squared=True: its square) to the nearest other voxel of the same sample, 0 elsewhere; `sampling` a scalar or (sz, sy, sx).
    float32 of the mask's shape.  A sample without any background voxel gives +inf everywhere (scipy leaves that case unspecified)."""
    return _edt(mask, sampling, cls, EDT_SQUARED if squared else EDT_DISTANCE, out)


def signed_distance_map(mask, sampling=None, cls=None, out=None):
    """+ distance to the foreground outside the mask, - distance to the background inside; all zero for a sample whose mask is empty or full"""
    return _edt(mask, sampling, cls, EDT_SIGNED, out)


def boundary_distance_maps(labels, num_class, sampling=None, out=None):
    """The maps of the boundary loss (Kervadec et al.), edt(~m) * [~m] - (edt(m) - 1) * [m] per class: labels (N, *spatial) with two or three spatial axes
    -> float32 (N, C, *spatial), C = num_class.  num_class == 1: one plane for labels != 0; otherwise plane k for labels == k, k = 0..C-1.  A plane whose
    mask is empty or full in a sample is zero there.  One seg_edt call per class on the current stream, written in place, no synchronisation."""
    if not torch.is_tensor(labels) or labels.dim() not in (3, 4) or labels.dtype.is_floating_point or labels.dtype.is_complex:
        raise TypeError("expected an integer label tensor (N, H, W) or (N, D, H, W)")
    num_class = int(num_class)
    if num_class < 1 or num_class > 256:
        raise ValueError("num_class must be 1..256")
    lab = labels if labels.dtype == torch.uint8 else labels.to(torch.uint8)
    lab = lab.contiguous()
    spatial = tuple(lab.shape[1:])
    nd = (lab.shape[0],) + (1,) * (3 - len(spatial)) + spatial
    v = nd[1] * nd[2] * nd[3]
    shape = (lab.shape[0], num_class) + spatial
    if out is None:
        out = torch.empty(shape, dtype=torch.float32, device=lab.device)
    elif out.dtype != torch.float32 or tuple(out.shape) != shape or out.device != lab.device or not out.is_contiguous():
        raise ValueError("out must be a contiguous float32 tensor (N, num_class, *spatial) on the labels' device")
    lib = _capi.lib_for(lab.device)
    sp = _edt_sampling(sampling, len(spatial))
    for k in range(num_class):
        _edt_call(lib, lab, nd, -1 if num_class == 1 else k, sp, EDT_BOUNDARY, out.data_ptr() + 4 * k * v, num_class * v)
    return out
