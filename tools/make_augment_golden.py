"""Writes tests/golden/augment3d.npz: what the LIVE reference generator (dataprocess/Augmentation/images_masks_3dtransform.py, loaded by file path from
the tree oracle.ref_loader points at) computes for the cases of tests/test_augment.py.  Numeric data only: seeded random inputs, constructor arguments,
seeds, the centred transform matrix / flips / channel shifts captured from inside `random_transform`, its outputs, `standardize` of the image, the next
np.random.random() after the draw, and the first three batches of one `flow`.

    python tools/make_augment_golden.py            (needs the reference tree, numpy and scipy)

The comparison in the tests is exact (order=0 copies input values), so it must never rest on the last bit of a double: for every captured matrix of a
random-angle case the coordinates cc = ((i0*A[a][0] + i1*A[a][1]) + i2*A[a][2]) + off[a] of all output voxels are recomputed here, and the script asserts
that no cc + 0.5 inside the volume lies within 1e-9 of an integer and that no cc lies within 1e-9 of 0 or n - 1 (the clamp / outside decision); the
smallest margin found is stored.  It also asserts that the numpy restatement of scipy's rule (`restate`) reproduces the reference's output, and that
each of the three flips occurs in one case and is absent in another.  Seeds that miss an assertion are simply replaced.

tests/test_augment.py::test_golden_file_is_what_the_live_reference_computes re-runs `reference_case` / `reference_flow` and compares with the file."""
import importlib.util
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUT = os.path.join(ROOT, "tests", "golden", "augment3d.npz")
MARGIN = 1e-9
FILL_IDS = {"nearest": 0, "constant": 1}
ARG_NAMES = ("rotation_range", "width_shift_range", "height_shift_range", "depth_shift_range", "zoom_lo", "zoom_hi", "channel_shift_range", "fill_mode",
             "cval", "horizontal_flip", "vertical_flip", "depth_flip", "rescale")

_AFFINE = dict(rotation_range=20, width_shift_range=0.1, height_shift_range=0.1, depth_shift_range=0.1, zoom_range=0.2, horizontal_flip=True,
               vertical_flip=True, depth_flip=True)
# (name, extents, channels, label dtype, constructor arguments, seed, random angles?)
CASES = (
    ("tiny_5x7x9", (5, 7, 9), 1, np.uint8, dict(_AFFINE, fill_mode="nearest"), 3, True),
    ("slab_3x130x67", (3, 130, 67), 1, np.uint8, dict(_AFFINE, fill_mode="nearest"), 4, True),
    ("const_6x10x33", (6, 10, 33), 1, np.int64, dict(_AFFINE, fill_mode="constant", cval=-3., width_shift_range=0.3, height_shift_range=0.3,
                                                      depth_shift_range=0.3), 5, True),
    ("ties_5x9x13", (5, 9, 13), 1, np.uint8, dict(zoom_range=(0.5, 0.5)), 6, False),
    ("shift_4x6x70x3", (4, 6, 70), 3, np.uint8, dict(_AFFINE, fill_mode="nearest", channel_shift_range=0.5, rescale=1.1), 11, True),
)
FLOW = dict(shape=(3, 4, 5, 6, 1), kwargs=dict(rotation_range=20, width_shift_range=0.1, height_shift_range=0.1, depth_shift_range=0.1, zoom_range=0.2,
                                              horizontal_flip=True, rescale=1.1), batch_size=2, seed=11, batches=3)


def load_reference():
    sys.path.insert(0, ROOT)
    from oracle import ref_loader
    path = os.path.join(ref_loader.REF, "dataprocess", "Augmentation", "images_masks_3dtransform.py")
    spec = importlib.util.spec_from_file_location("ref_images_masks_3dtransform", path)
    mod = importlib.util.module_from_spec(spec)
    sys.dont_write_bytecode = True
    spec.loader.exec_module(mod)
    return mod


def reference_available():
    sys.path.insert(0, ROOT)
    from oracle import ref_loader
    return os.path.isfile(os.path.join(ref_loader.REF, "dataprocess", "Augmentation", "images_masks_3dtransform.py"))


def make_inputs(shape, channels, label_dtype, seed):
    rng = np.random.default_rng(1000 + seed)
    x = rng.standard_normal(tuple(shape) + (channels,)).astype(np.float32)
    y = rng.integers(0, 4, size=tuple(shape) + (channels,)).astype(label_dtype)
    return x, y


def ctor_args(kwargs):
    z = kwargs.get("zoom_range", 0.)
    lo, hi = (1 - z, 1 + z) if np.isscalar(z) else z
    g = lambda k, d=0.: kwargs.get(k, d)
    return np.array([g("rotation_range"), g("width_shift_range"), g("height_shift_range"), g("depth_shift_range"), lo, hi, g("channel_shift_range"),
                     FILL_IDS[g("fill_mode", "nearest")], g("cval"), g("horizontal_flip", False), g("vertical_flip", False), g("depth_flip", False),
                     g("rescale", None) or 0.], dtype=np.float64)


class Capture:
    """records what the reference draws inside random_transform: the matrices handed to apply_transform, the flipped axes, every np.random.uniform result"""

    def __init__(self, mod):
        self.mod, self.matrices, self.flipped, self.uniforms = mod, [], [], []

    def __enter__(self):
        mod = self.mod
        self.saved = (mod.apply_transform, mod.flip_axis, np.random.uniform)
        ap, fl, un = self.saved

        def apply_transform(x, m, *a, **k):
            self.matrices.append(np.array(m, dtype=np.float64))
            return ap(x, m, *a, **k)

        def flip_axis(x, axis):
            self.flipped.append(axis)
            return fl(x, axis)

        def uniform(*a, **k):
            r = un(*a, **k)
            self.uniforms.append(r)
            return r

        mod.apply_transform, mod.flip_axis, np.random.uniform = apply_transform, flip_axis, uniform
        return self

    def __exit__(self, *exc):
        self.mod.apply_transform, self.mod.flip_axis, np.random.uniform = self.saved


def coordinates(matrix, shape):
    """cc[a] for every output voxel, in scipy's summation order, float64: (3, n0, n1, n2)"""
    i0, i1, i2 = np.meshgrid(*[np.arange(n, dtype=np.float64) for n in shape], indexing="ij")
    return np.stack([((i0 * matrix[a, 0] + i1 * matrix[a, 1]) + i2 * matrix[a, 2]) + matrix[a, 3] for a in range(3)])


def margin(matrix, shape):
    """smallest distance of a decision to its threshold: cc + 0.5 to an integer (inside the volume), cc to 0 and to n - 1"""
    cc = coordinates(matrix, shape)
    m = np.inf
    for a, n in enumerate(shape):
        c = cc[a]
        m = min(m, np.abs(c).min(), np.abs(c - (n - 1)).min())
        inside = c[(c > 0) & (c < n - 1)] + 0.5
        if inside.size:
            m = min(m, np.abs(inside - np.rint(inside)).min())
    return float(m)


def restate(vol, matrix, fill_mode, cval):
    """scipy.ndimage.affine_transform(vol, A, off, order=0, mode=fill_mode, cval=cval) for one (n0, n1, n2) volume, in numpy"""
    shape = vol.shape
    cc = coordinates(matrix, shape)
    outside = np.zeros(shape, dtype=bool)
    idx = []
    for a, n in enumerate(shape):
        c = cc[a]
        outside |= (c < 0) | (c > n - 1)
        idx.append(np.floor(np.clip(c, 0, n - 1) + 0.5).astype(np.int64))
    out = vol[idx[0], idx[1], idx[2]]
    if fill_mode == "constant":
        out = np.where(outside, np.asarray(cval).astype(vol.dtype), out)
    return out


def flip(a, flips):
    for axis in range(3):
        if flips[axis]:
            a = np.flip(a, axis)
    return np.ascontiguousarray(a)


def reference_case(mod, case):
    """one case through the live reference -> dict of arrays"""
    name, shape, channels, label_dtype, kwargs, seed, _ = case
    x, y = make_inputs(shape, channels, label_dtype, seed)
    gen = mod.ImageDataGenerator3D(**kwargs)
    with Capture(mod) as cap:
        np.random.seed(seed)
        xo, yo = gen.random_transform(x.copy(), y.copy())
        nxt = np.random.random()
    xs = gen.standardize(np.array(xo, copy=True))
    matrix = cap.matrices[0][:3, :]
    assert np.array_equal(cap.matrices[0], cap.matrices[1])
    flips = np.array([0 in cap.flipped, 1 in cap.flipped, 2 in cap.flipped])
    shifts = np.array(cap.uniforms[-channels:], dtype=np.float64) if kwargs.get("channel_shift_range", 0.) else np.zeros(0)
    res = {"x": x, "y": y, "args": ctor_args(kwargs), "seed": np.int64(seed), "matrix": matrix, "flips": flips, "shifts": shifts,
           "xo": np.ascontiguousarray(xo), "yo": np.ascontiguousarray(yo), "xs": np.ascontiguousarray(xs), "next": np.float64(nxt)}
    assert res["xo"].dtype == np.float32 and res["xs"].dtype == np.float32 and res["yo"].dtype == label_dtype
    if len(shifts):
        # how many voxels the clip of random_channel_shift moved back to the minimum / maximum (the reference's apply_transform alone, then the shift)
        t = mod.apply_transform(x.copy(), cap.matrices[0], 3, fill_mode=kwargs.get("fill_mode", "nearest"), cval=kwargs.get("cval", 0.))
        moved = t + shifts.astype(np.float32)
        res["clipped"] = np.array([(moved < t.min()).sum(), (moved > t.max()).sum()], dtype=np.int64)
    if kwargs.get("fill_mode") == "constant":
        # the label with cval 0 (the form a uint8 mask needs): the reference's own apply_transform with the captured matrix, then the flips
        y0 = mod.apply_transform(y.copy(), cap.matrices[0], 3, fill_mode="constant", cval=0.)
        res["yo_cval0"] = flip(y0, flips)
    return res


def reference_flow(mod):
    n = FLOW["shape"][0]
    rng = np.random.default_rng(77)
    x = rng.standard_normal(FLOW["shape"]).astype(np.float32)
    y = (rng.integers(0, 2, size=FLOW["shape"]) * 255).astype(np.uint8)
    gen = mod.ImageDataGenerator3D(**FLOW["kwargs"])
    res = {"flow_x": x, "flow_y": y, "flow_args": ctor_args(FLOW["kwargs"]), "flow_batch_size": np.int64(FLOW["batch_size"]),
           "flow_seed": np.int64(FLOW["seed"])}
    with Capture(mod) as cap:
        it = gen.flow(x, y, batch_size=FLOW["batch_size"], shuffle=True, seed=FLOW["seed"])
        for b in range(FLOW["batches"]):
            bx, by = next(it)
            assert bx.dtype == np.float64 and by.dtype == np.float64
            res["flow_bx%d" % b], res["flow_by%d" % b] = bx, by
    assert [len(res["flow_bx%d" % b]) for b in range(3)] == [2, 1, 2] and n == 3
    return res, cap.matrices


def check_case(case, res):
    """the numpy restatement reproduces the reference; returns the decision margin of the case"""
    name, shape, channels, label_dtype, kwargs, seed, random_angles = case
    mode, cval = kwargs.get("fill_mode", "nearest"), kwargs.get("cval", 0.)
    m = res["matrix"]
    want_y = np.stack([restate(res["y"][..., c], m, mode, cval) for c in range(channels)], axis=-1)
    assert np.array_equal(flip(want_y, res["flips"]), res["yo"]), name
    want_x = np.stack([restate(res["x"][..., c], m, mode, cval) for c in range(channels)], axis=-1)
    if len(res["shifts"]):
        # random_channel_shift: f32 add of the shift, clip at the extrema of the transformed sample; the case must clip at both ends
        lo, hi = want_x.min(), want_x.max()
        moved = want_x + res["shifts"].astype(np.float32)
        assert np.array_equal(res["clipped"], [(moved < lo).sum(), (moved > hi).sum()]) and res["clipped"].min() > 0, (name, res["clipped"])
        want_x = np.clip(moved, lo, hi)
    assert want_x.dtype == np.float32 and np.array_equal(flip(want_x, res["flips"]), res["xo"]), name
    mg = margin(m, shape)
    if random_angles:
        assert mg >= MARGIN, "%s: seed %d leaves a margin of %.3g; pick another seed" % (name, seed, mg)
    return mg


def main():
    mod = load_reference()
    out = {"names": np.array([c[0] for c in CASES]), "arg_names": np.array(ARG_NAMES)}
    margins, flips = [], []
    for i, case in enumerate(CASES):
        res = reference_case(mod, case)
        mg = check_case(case, res)
        if case[6]:
            margins.append(mg)
        flips.append(res["flips"])
        for k, v in res.items():
            out["c%d_%s" % (i, k)] = v
        print("%-16s seed %d flips %s margin %.3g next %.17g" % (case[0], case[5], res["flips"].astype(int), mg, res["next"]))
    flips = np.array(flips)
    assert flips.any(axis=0).all() and (~flips).any(axis=0).all(), "every flip must occur in one case and be absent in another:\n%s" % flips
    flow, matrices = reference_flow(mod)
    for m in matrices:
        mg = margin(m[:3, :], FLOW["shape"][1:4])
        assert mg >= MARGIN, "flow: seed %d leaves a margin of %.3g" % (FLOW["seed"], mg)
        margins.append(mg)
    out.update(flow)
    out["min_margin"] = np.float64(min(margins))
    print("smallest decision margin of the random-angle draws: %.3g" % min(margins))
    np.savez_compressed(OUT, **out)
    print(OUT, os.path.getsize(OUT), "bytes")


if __name__ == "__main__":
    main()
