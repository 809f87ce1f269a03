"""Float64 brute-force oracle of the Euclidean distance transform (csrc/edt.hip) and the test volumes of tests/test_edt.py / test_boundary_loss.py.
For every foreground voxel the minimum over ALL background voxels of the same sample of sum_a (delta_a * s_a)^2, chunked over the foreground; no scipy,
no separable pass, nothing shared with the kernels.  Results are computed once per (case, class, spacing, side) and handed out read-only."""
import numpy as np

UNIT = (1.0, 1.0, 1.0)
ANISO = (2.5, 0.78, 0.78)


def edt_sq(mask, sampling=UNIT):
    """mask bool (d, h, w) -> float64 (d, h, w): squared distance to the nearest False voxel on the True voxels (+inf when there is none), 0 elsewhere"""
    mask = np.asarray(mask, dtype=bool)
    out = np.zeros(mask.shape, dtype=np.float64)
    fg = np.argwhere(mask)
    bg = np.argwhere(~mask)
    if len(fg) == 0:
        return out
    if len(bg) == 0:
        out[mask] = np.inf
        return out
    s = np.asarray(sampling, dtype=np.float64).reshape(1, 1, 3)
    best = np.empty(len(fg), dtype=np.float64)
    step = max(1, (1 << 20) // len(bg))
    for i in range(0, len(fg), step):
        d = (fg[i:i + step, None, :] - bg[None, :, :]).astype(np.float64) * s
        best[i:i + step] = (d * d).sum(axis=2).min(axis=1)
    out[mask] = best
    return out


def fg_of(labels, cls):
    return labels != 0 if cls == -1 else labels == cls


_cache = {}


def batch_sq(name, cls=-1, sampling=UNIT, complement=False):
    """squared transform of every sample of case `name` (float64 (n, d, h, w), read-only); complement: of the background instead"""
    key = (name, cls, tuple(sampling), complement)
    if key not in _cache:
        m = fg_of(CASES[name], cls)
        r = np.stack([edt_sq(~s if complement else s, sampling) for s in m])
        r.setflags(write=False)
        _cache[key] = r
    return _cache[key]


def combined(name, cls, sampling, mode):
    """modes 2 (signed) and 3 (boundary) from the two one-sided distance maps, as include/segengine.h defines them; zero for a sample whose mask is empty
    or full"""
    m = fg_of(CASES[name], cls)
    din, dout = np.sqrt(batch_sq(name, cls, sampling)), np.sqrt(batch_sq(name, cls, sampling, complement=True))
    out = np.zeros(m.shape, dtype=np.float64)
    for s in range(len(m)):
        if m[s].any() and not m[s].all():
            out[s] = dout[s] * ~m[s] - ((din[s] - 1.0) if mode == 3 else din[s]) * m[s]
    return out


def boundary_maps(labels, num_class, sampling=UNIT):
    """prepost.boundary_distance_maps restated: labels (n, *spatial) -> float64 (n, C, *spatial)"""
    labels = np.asarray(labels)
    vol = labels.reshape((labels.shape[0],) + (1,) * (4 - labels.ndim) + labels.shape[1:])
    sp = (1.0,) * (4 - labels.ndim) + tuple(sampling)[-(labels.ndim - 1):]
    out = np.zeros((labels.shape[0], num_class) + vol.shape[1:], dtype=np.float64)
    for k in range(num_class):
        m = vol != 0 if num_class == 1 else vol == k
        for s in range(len(m)):
            if m[s].any() and not m[s].all():
                out[s, k] = np.sqrt(edt_sq(~m[s], sp)) * ~m[s] - (np.sqrt(edt_sq(m[s], sp)) - 1.0) * m[s]
    return out.reshape((labels.shape[0], num_class) + labels.shape[1:])


def _random(shape, p, seed):
    rng = np.random.default_rng(seed)
    return (rng.random(shape) < p).astype(np.uint8)


def _labels(n=2, shape=(6, 11, 70), seed=5):
    """label volumes with values {0, 1, 2, 3}: three boxes per sample with salt noise of other labels; class 3 is absent from sample 1"""
    rng = np.random.default_rng(seed)
    v = np.zeros((n,) + shape, dtype=np.uint8)
    for i in range(n):
        for c in (1, 2, 3):
            z0, y0, x0 = rng.integers(0, 3), rng.integers(0, 5), rng.integers(0, 40)
            v[i, z0:z0 + 3, y0:y0 + 5, x0 + 4 * c:x0 + 4 * c + 20] = c
        noise = rng.random(shape) < 0.03
        v[i][noise] = rng.integers(0, 4, size=int(noise.sum()))
    v[1][v[1] == 3] = 0
    return v


def _make_cases():
    c = {"tiny": _random((1, 5, 7, 9), 0.8, 11), "slab": _random((1, 3, 130, 67), 0.9, 12), "plane2d": _random((2, 1, 300, 70), 0.95, 13)}
    far_bg = np.ones((1, 12, 20, 70), dtype=np.uint8)
    far_bg[0, 11, 0, 69] = 0
    far_fg = np.zeros((1, 12, 20, 70), dtype=np.uint8)
    far_fg[0, 5, 9, 33] = 1
    full_empty = np.zeros((2, 4, 5, 70), dtype=np.uint8)
    full_empty[0] = 1
    c.update(far_bg=far_bg, far_fg=far_fg, labels=_labels(), full_empty=full_empty)
    for v in c.values():
        v.setflags(write=False)
    return c


CASES = _make_cases()
RANDOM = ("tiny", "slab", "plane2d")             # every sample of these must hold both kinds of voxel
# (case, cls) pairs the transform is checked on; full_empty has its own test
PAIRS = [("tiny", -1), ("slab", -1), ("plane2d", -1), ("far_bg", -1), ("far_fg", -1), ("labels", -1), ("labels", 0), ("labels", 2), ("labels", 3)]
