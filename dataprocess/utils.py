"""Pre/post-processing helpers the wrappers and scripts call (dataprocess/utils.py of the reference).  The resampling / normalisation helpers
(utils.py:99-233) are host-side; the mask cleaning (utils.py:7-96) runs on the device.  SimpleITK is optional in this image; the helpers that
need it import it lazily."""
import os

import numpy as np


def file_name_path(file_dir, dir=True, file=False):
    """sub-directories (dir=True) or files (file=True) of the first non-empty level (utils.py:221-233)."""
    for root, dirs, files in os.walk(file_dir):
        if len(dirs) and dir:
            print("sub_dirs:", dirs)
            return dirs
        if len(files) and file:
            print("files:", files)
            return files


def normalize(slice, bottom=95, down=5):
    """percentile clip + z-score over the non-zero voxels (utils.py:182-204; the `tmp == tmp.min() -> -9` line is
    commented out in the reference and is not applied).  Host-side numpy form; the wrappers use the device kernel
    (pytorchdeeplearing_amd.prepost.normalize_percentile)."""
    b, t = np.percentile(slice, bottom), np.percentile(slice, down)
    slice = np.clip(slice, t, b)
    image_nonzero = slice[np.nonzero(slice)]
    if np.std(slice) == 0 or np.std(image_nonzero) == 0:
        return slice
    return (slice - np.mean(image_nonzero)) / np.std(image_nonzero)


def _sitk():
    import SimpleITK as sitk
    return sitk


def resize_image_itkwithsize(itkimage, newSize, originSize, resamplemethod=None):
    """resample to a fixed grid size keeping the physical extent (utils.py:99-120)."""
    sitk = _sitk()
    resampler = sitk.ResampleImageFilter()
    originSize, newSize = np.array(originSize), np.array(newSize)
    factor = originSize / newSize
    newSpacing = np.array(itkimage.GetSpacing()) * factor
    resampler.SetReferenceImage(itkimage)
    resampler.SetOutputSpacing(newSpacing.tolist())
    resampler.SetSize(newSize.astype(int).tolist())
    resampler.SetTransform(sitk.Transform(3, sitk.sitkIdentity))
    resampler.SetInterpolator(sitk.sitkNearestNeighbor if resamplemethod is None else resamplemethod)
    out = resampler.Execute(itkimage)
    return sitk.GetArrayFromImage(out), out


def ConvertitkTrunctedValue(image, upper=200, lower=-200, normalize="maxmin"):
    """clip to [lower, upper] then max-min or mean-std normalise (utils.py:148-179)."""
    sitk = _sitk()
    arr = np.clip(sitk.GetArrayFromImage(image).astype(np.float64), lower, upper)
    if normalize == "maxmin":
        arr = (arr - arr.min()) / max(arr.max() - arr.min(), 1e-12)
    elif normalize == "meanstd":
        arr = (arr - arr.mean()) / max(arr.std(ddof=1), 1e-12)      # itk::NormalizeImageFilter: unbiased variance
    out = sitk.GetImageFromArray(arr.astype(np.float32))
    out.SetSpacing(image.GetSpacing()); out.SetOrigin(image.GetOrigin()); out.SetDirection(image.GetDirection())
    return out


# ---- mask cleaning (utils.py:7-96) on the device: pytorchdeeplearing_amd.prepost over csrc/postproc.hip ----

def _to_device_mask(image):
    """numpy array, device tensor or SimpleITK image -> (uint8 device tensor (D, H, W), kind, the original); host arrays go to the current device"""
    import torch
    if torch.is_tensor(image):
        return image, "tensor", image
    if isinstance(image, np.ndarray):
        return torch.from_numpy(np.ascontiguousarray(image)).to(_device()), "numpy", image
    sitk = _sitk()                                              # anything else has to be a SimpleITK image
    return torch.from_numpy(np.ascontiguousarray(sitk.GetArrayFromImage(image))).to(_device()), "sitk", image


MASK_DEVICE = None          # where host arrays are uploaded; None: the current GPU


def _device():
    import torch
    return MASK_DEVICE if MASK_DEVICE is not None else torch.device("cuda", torch.cuda.current_device())


def _volume(t):
    """(D, H, W) view of a 2-D or 3-D mask"""
    if t.dim() == 2:
        return t.unsqueeze(0)
    if t.dim() != 3:
        raise ValueError("expected a 2-D or 3-D mask")
    return t


def _from_device_mask(t, kind, like):
    if kind == "tensor":
        return t
    arr = t.cpu().numpy()
    if kind == "numpy":
        return arr
    sitk = _sitk()
    out = sitk.GetImageFromArray(arr)
    out.SetSpacing(like.GetSpacing()); out.SetDirection(like.GetDirection()); out.SetOrigin(like.GetOrigin())
    return out


def GetLargestConnectedCompont(binarysitk_image):
    """0/1 mask of the largest face-connected component of `image != 0` (utils.py:19-44: ConnectedComponent + the `maxsize < size` loop, which keeps
    the first of several largest components); uint8."""
    import torch
    from pytorchdeeplearing_amd import prepost
    t, kind, like = _to_device_mask(binarysitk_image)
    binary = (_volume(t) != 0).to(torch.uint8)
    return _from_device_mask(prepost.keep_largest_component(binary, out=binary).reshape(t.shape), kind, like)


def GetLargestConnectedCompontBoundingbox(binarysitk_image):
    """[xstart, ystart, zstart, xsize, ysize, zsize].  Despite its name the reference (utils.py:13-15) runs LabelShapeStatistics on the BINARY image and
    asks for label 1: the box of ALL voxels equal to 1, not of the largest component.  Restated as that: cls = 1, whole-foreground box."""
    import torch
    from pytorchdeeplearing_amd import prepost
    t, _, _ = _to_device_mask(binarysitk_image)
    box = prepost.foreground_bbox(_volume(t).to(torch.uint8), cls=1).cpu().numpy().astype(np.int64)
    if box[3] < 0:
        raise RuntimeError("GetLargestConnectedCompontBoundingbox: label 1 is not in the image")      # (LabelShapeStatistics raises too)
    z0, y0, x0, z1, y1, x1 = box
    if t.dim() == 2:
        return np.array([x0, y0, x1 - x0 + 1, y1 - y0 + 1])
    return np.array([x0, y0, z0, x1 - x0 + 1, y1 - y0 + 1, z1 - z0 + 1])


def MorphologicalOperation(sitk_maskimg, kernelsize, name='open'):
    """open / close / dilate / erode of `mask != 0` with SimpleITK's default kernel, a ball of radius `kernelsize` on every axis of extent above 1
    (utils.py:47-66); 0/1 uint8.  An unknown name returns None, as the reference does."""
    if name not in ("open", "close", "dilate", "erode"):
        return None
    import torch
    from pytorchdeeplearing_amd import prepost
    t, kind, like = _to_device_mask(sitk_maskimg)
    vol = (_volume(t) != 0).to(torch.uint8)
    radius = tuple(int(kernelsize) if s > 1 else 0 for s in vol.shape)
    out = prepost.binary_morphology(vol, name, radius, shape="ball")
    return _from_device_mask(out.reshape(t.shape), kind, like)


def getRangImageRange(image, index=0):
    """(first, last) position along axis `index` with a non-zero maximum, (0, 0) for an empty image (utils.py:69-96, including its indifference between
    "empty" and "only position 0")."""
    import torch
    if torch.is_tensor(image):
        flag = (image.movedim(index, 0).reshape(image.shape[index], -1).max(dim=1).values != 0).cpu().numpy()
    else:
        flag = np.max(np.moveaxis(np.asarray(image), index, 0).reshape(image.shape[index], -1), axis=1) != 0
    hit = np.flatnonzero(flag)
    return (int(hit[0]), int(hit[-1])) if len(hit) else (0, 0)
