"""ImageDataGenerator3D / DataAug3D (pytorchdeeplearing_amd/augment.py over csrc/augment.hip) against the reference generator
(dataprocess/Augmentation/images_masks_3dtransform.py, ImageAugmentation.py).

tests/golden/augment3d.npz holds what the live reference computes (tools/make_augment_golden.py): per case the seeded inputs, the constructor
arguments, the centred matrix / flips / channel shifts captured inside `random_transform`, its outputs, `standardize` of the image and the next
np.random.random() after the draw; and the first three batches of one `flow`.
  tiny_5x7x9      rotation 20, shifts 0.1, zoom 0.2, nearest: every extent below a wave, innermost extent no multiple of the store width
  slab_3x130x67   the same settings: many rows, W no multiple of 64; uint8 label
  const_6x10x33   constant, cval -3, shifts 0.3: many outside voxels, the outside half voxel at the edges; int64 label (cval -3) and uint8 label (cval 0)
  ties_5x9x13     zoom (0.5, 0.5) only: every coordinate exact, even source indices land on x.5 - floor(cc + 0.5), not round-half-even
  shift_4x6x70x3  three channels, channel shift 0.5 (clip at the extrema of the transformed sample), rescale 1.1; three-channel label

Tolerances: none.  order = 0 copies input values, the channel shift is one f32 add and two f32 comparisons, the rescale one f32 multiply: image and
label are compared with np.array_equal.  The generator script asserts that no rounding or clamp decision of a random-angle case lies within 1e-9 of its
threshold (`min_margin` in the file), so exactness does not rest on the last bit of a double."""
import os
import sys

import numpy as np
import pytest
import torch

from conftest import GOLDEN, ROOT

sys.path.insert(0, os.path.join(ROOT, "tools"))

NAMES = ("tiny_5x7x9", "slab_3x130x67", "const_6x10x33", "ties_5x9x13", "shift_4x6x70x3")
FILL = {0: "nearest", 1: "constant"}
_gold = None


def gold():
    global _gold
    if _gold is None:
        with np.load(os.path.join(GOLDEN, "augment3d.npz")) as z:
            _gold = {k: z[k] for k in z.files}
        assert tuple(_gold["names"]) == NAMES
        for v in _gold.values():
            v.setflags(write=False)
    return _gold


def case(i):
    g = gold()
    p = "c%d_" % i
    return {k[len(p):]: v for k, v in g.items() if k.startswith(p)}


def gen_kwargs(args):
    a = dict(zip(gold()["arg_names"], (float(v) for v in args)))
    return dict(rotation_range=a["rotation_range"], width_shift_range=a["width_shift_range"], height_shift_range=a["height_shift_range"],
                depth_shift_range=a["depth_shift_range"], zoom_range=(a["zoom_lo"], a["zoom_hi"]), channel_shift_range=a["channel_shift_range"],
                fill_mode=FILL[int(a["fill_mode"])], cval=a["cval"], horizontal_flip=bool(a["horizontal_flip"]), vertical_flip=bool(a["vertical_flip"]),
                depth_flip=bool(a["depth_flip"]), rescale=a["rescale"] or None)


def test_the_golden_file_covers_what_it_should():
    g = gold()
    assert g["min_margin"] >= 1e-9
    flips = np.array([case(i)["flips"] for i in range(len(NAMES))])
    assert flips.any(axis=0).all() and (~flips).any(axis=0).all()          # every flip occurs in one case and is absent in another
    assert case(2)["yo"].dtype == np.int64 and (case(2)["yo"] == -3).any() and (case(2)["xo"] == -3).any()
    assert len(case(4)["shifts"]) == 3 and case(4)["x"].shape == (4, 6, 70, 3)
    assert case(4)["clipped"].min() > 0                                   # the clip of the channel shift is active at both extrema


@pytest.mark.parametrize("i", range(5), ids=NAMES)
def test_apply_transform_matches_the_reference(dev, i):
    from pytorchdeeplearing_amd.augment import apply_transform
    c = case(i)
    kw = gen_kwargs(c["args"])
    shifts = c["shifts"] if len(c["shifts"]) else None
    flips = tuple(bool(f) for f in c["flips"])
    xo, yo = apply_transform(c["x"], c["matrix"], flips, kw["fill_mode"], kw["cval"], label=c["y"], channel_shift=shifts, device=dev)
    assert xo.dtype == np.float32 and yo.dtype == c["y"].dtype and xo.shape == c["x"].shape and yo.shape == c["y"].shape
    print(NAMES[i], "image mismatches", int((xo != c["xo"]).sum()), "label mismatches", int((yo != c["yo"]).sum()), "of", xo.size)
    assert np.array_equal(xo, c["xo"]) and np.array_equal(yo, c["yo"])
    # the rescale in the same call (gather pass, or the shift pass when a channel shift is set) = the reference's standardize
    xs = apply_transform(c["x"], c["matrix"], flips, kw["fill_mode"], kw["cval"], channel_shift=shifts, rescale=kw["rescale"], device=dev)
    assert np.array_equal(xs, c["xs"])
    # device tensors in, device tensors out; a label without the channel axis
    xt, yt = torch.from_numpy(c["x"].copy()).to(dev), torch.from_numpy(c["y"][..., 0].copy()).to(dev)
    xo_t, yo_t = apply_transform(xt, c["matrix"], flips, kw["fill_mode"], kw["cval"], label=yt, channel_shift=shifts)
    assert xo_t.device == xt.device and yo_t.dtype == yt.dtype
    assert np.array_equal(xo_t.cpu().numpy(), c["xo"]) and np.array_equal(yo_t.cpu().numpy(), c["yo"][..., 0])
    if "yo_cval0" in c:
        # a uint8 mask cannot hold cval -3: the call refuses it; with label_cval 0 it equals the reference's apply_transform(..., cval=0)
        y8 = c["y"].astype(np.uint8)
        with pytest.raises(RuntimeError, match="label_cval"):
            apply_transform(c["x"], c["matrix"], flips, "constant", kw["cval"], label=y8, device=dev)
        xo8, yo8 = apply_transform(c["x"], c["matrix"], flips, "constant", kw["cval"], label=y8, label_cval=0, device=dev)
        assert yo8.dtype == np.uint8 and np.array_equal(yo8, c["yo_cval0"].astype(np.uint8)) and np.array_equal(xo8, c["xo"])
        assert (c["yo_cval0"] != c["yo"]).any()


@pytest.mark.parametrize("i", range(5), ids=NAMES)
def test_generator_matches_the_reference(dev, i):
    from pytorchdeeplearing_amd.augment import ImageDataGenerator3D
    c = case(i)
    gen = ImageDataGenerator3D(**gen_kwargs(c["args"]))
    np.random.seed(int(c["seed"]))
    xo, yo = gen.random_transform(c["x"].copy(), c["y"].copy(), device=dev)
    assert np.random.random() == float(c["next"])
    assert np.array_equal(xo, c["xo"]) and np.array_equal(yo, c["yo"]) and yo.dtype == c["y"].dtype
    xs = gen.standardize(xo)
    assert xs is xo and xs.dtype == np.float32 and np.array_equal(xs, c["xs"])
    if gen.rescale:                                  # the device form of standardize: in place, one f32 multiply
        t = torch.from_numpy(c["xo"].copy()).to(dev)
        assert gen.standardize(t) is t and np.array_equal(t.cpu().numpy(), c["xs"])


@pytest.mark.parametrize("i", range(5), ids=NAMES)
def test_draw_transform_is_the_reference_draw(i):
    """host only: the matrix bit for bit, the flips, the channel shifts and the state of np.random afterwards"""
    from pytorchdeeplearing_amd.augment import ImageDataGenerator3D, draw_transform
    c = case(i)
    gen = ImageDataGenerator3D(**gen_kwargs(c["args"]))
    np.random.seed(int(c["seed"]))
    matrix, flips, shifts = draw_transform(gen, c["x"].shape)
    assert np.random.random() == float(c["next"])
    assert matrix.dtype == np.float64 and matrix.shape == (3, 4) and matrix.tobytes() == np.ascontiguousarray(c["matrix"]).tobytes()
    assert tuple(flips) == tuple(bool(f) for f in c["flips"])
    if len(c["shifts"]):
        assert shifts.tobytes() == c["shifts"].tobytes()
    else:
        assert shifts is None


def test_a_batch_in_one_launch_equals_the_single_calls_in_both_layouts(dev):
    from pytorchdeeplearing_amd.augment import ImageDataGenerator3D, apply_transform, draw_transform
    c = case(4)
    gen = ImageDataGenerator3D(**gen_kwargs(c["args"]))
    np.random.seed(123)
    m2, f2, s2 = draw_transform(gen, c["x"].shape)
    rng = np.random.default_rng(9)
    x = np.stack([c["x"], rng.standard_normal(c["x"].shape).astype(np.float32) * 3])
    y = np.stack([c["y"][..., 0], rng.integers(0, 200, size=c["y"].shape[:3]).astype(np.uint8)])
    ms, fs, ss = np.stack([c["matrix"], m2]), np.array([c["flips"], f2]), np.stack([c["shifts"], s2])
    assert not np.array_equal(ms[0], ms[1])
    for mode, cval in (("nearest", 0.), ("constant", 2.)):
        bx, by = apply_transform(x, ms, fs, mode, cval, label=y, channel_shift=ss, rescale=1.1, device=dev)
        for k in range(2):
            sx, sy = apply_transform(x[k], ms[k], fs[k], mode, cval, label=y[k], channel_shift=ss[k], rescale=1.1, device=dev)
            assert np.array_equal(bx[k], sx) and np.array_equal(by[k], sy)
        if mode == "nearest":
            assert np.array_equal(bx[0], c["xs"]) and np.array_equal(by[0], c["yo"][..., 0])
        # (N, C, D, H, W): the same values without a transpose pass
        tx, ty = apply_transform(np.ascontiguousarray(x.transpose(0, 4, 1, 2, 3)), ms, fs, mode, cval, label=y, channel_shift=ss, rescale=1.1, layout="th",
                                 device=dev)
        assert np.array_equal(tx.transpose(0, 2, 3, 4, 1), bx) and np.array_equal(ty, by)
        # without the channel shift (the rescale runs in the gather pass), int64 and float32 labels
        for dt in (np.int64, np.float32):
            gx, gy = apply_transform(np.ascontiguousarray(x.transpose(0, 4, 1, 2, 3)), ms, fs, mode, cval, label=y.astype(dt), rescale=1.1, layout="th",
                                     device=dev)
            assert gy.dtype == dt and np.array_equal(gy, by.astype(dt))
            if mode == "nearest":
                assert np.array_equal(gx[0].transpose(1, 2, 3, 0), c_no_shift(c, dev))


def c_no_shift(c, dev):
    from pytorchdeeplearing_amd.augment import apply_transform
    return apply_transform(c["x"], c["matrix"], tuple(bool(f) for f in c["flips"]), "nearest", 0., rescale=1.1, device=dev)


def test_flow_yields_the_reference_batches(dev):
    from pytorchdeeplearing_amd.augment import ImageDataGenerator3D
    g = gold()
    gen = ImageDataGenerator3D(**gen_kwargs(g["flow_args"]))
    it = gen.flow(g["flow_x"], g["flow_y"], batch_size=int(g["flow_batch_size"]), shuffle=True, seed=int(g["flow_seed"]), device=dev)
    for b in range(3):
        bx, by = next(it)
        assert bx.dtype == np.float64 and by.dtype == np.float64
        assert bx.shape == g["flow_bx%d" % b].shape and len(bx) == (2, 1, 2)[b]
        assert np.array_equal(bx, g["flow_bx%d" % b]) and np.array_equal(by, g["flow_by%d" % b])
    with pytest.raises(ValueError):
        gen.flow(g["flow_x"][..., 0], g["flow_y"], device=dev)
    with pytest.raises(ValueError):
        gen.flow(g["flow_x"], g["flow_y"][:2], device=dev)


def test_constructor_and_argument_errors(dev):
    from pytorchdeeplearing_amd import _capi
    from pytorchdeeplearing_amd.augment import PARAM_DOUBLES, ImageDataGenerator3D, apply_transform, pack_params
    for mode in ("reflect", "wrap"):
        with pytest.raises(NotImplementedError, match="'nearest' and 'constant'"):
            ImageDataGenerator3D(fill_mode=mode)
    for opt in ("featurewise_center", "samplewise_center", "featurewise_std_normalization", "samplewise_std_normalization", "zca_whitening"):
        with pytest.raises(NotImplementedError):
            ImageDataGenerator3D(**{opt: True})
    with pytest.raises(ValueError):
        ImageDataGenerator3D(zoom_range=(1, 2, 3))
    with pytest.raises(ValueError):
        ImageDataGenerator3D(dim_ordering="xy")
    assert ImageDataGenerator3D(zoom_range=0.25).zoom_range == [0.75, 1.25] and ImageDataGenerator3D(zoom_range=(0.5, 2)).zoom_range == [0.5, 2]
    # the C call: nothing is launched on a bad argument (out keeps its content)
    lib = _capi.lib_for(dev)
    c = case(0)
    x = torch.from_numpy(c["x"].copy()).to(dev)
    out = torch.full_like(x, -7.0)
    ws = torch.empty(int(lib.seg_augment3d_ws_bytes(1)) + 256, dtype=torch.uint8, device=dev)
    good = pack_params(c["matrix"])
    assert good.shape == (1, PARAM_DOUBLES) and lib.seg_augment3d_ws_bytes(1) >= 256 and lib.seg_augment3d_ws_bytes(0) < 0
    pd = torch.from_numpy(good).to(dev)
    st = _capi.stream_for(dev)

    def call(params, mode=0, ext=(5, 7, 9), cval=0.0):
        return lib.seg_augment3d(x.data_ptr(), out.data_ptr(), 1, 1, ext[0], ext[1], ext[2], 1, 1, None, None, 0, 1, params.ctypes.data, pd.data_ptr(),
                                 mode, cval, cval, 0.0, 0, ws.data_ptr(), st)
    for k, bad in ((0, np.nan), (8, np.inf), (11, -np.inf), (12, 9.0)):
        p = good.copy()
        p[0, k] = bad
        assert call(p) < 0 and b"seg_augment3d" in lib.seg_last_error()
    assert call(np.full_like(good, np.nan)) < 0 and b"non-finite" in lib.seg_last_error()
    for mode in (2, 3):
        assert call(good, mode=mode) < 0 and b"reflect and wrap" in lib.seg_last_error()
    assert call(good, ext=(2048, 2048, 513)) < 0 and b"2^31" in lib.seg_last_error()          # extent product above 2^31
    assert call(good, ext=(5, 0, 9)) < 0 and call(good, cval=np.nan) < 0
    assert np.all(out.cpu().numpy() == -7.0)
    assert call(good) == 0 and np.array_equal(out.cpu().numpy(), apply_transform(c["x"], c["matrix"], device=dev))
    with pytest.raises(TypeError):
        apply_transform(x.double(), c["matrix"])
    with pytest.raises(TypeError):
        apply_transform(c["x"], c["matrix"], label=c["y"].astype(np.float64), device=dev)


def test_cpu_tensors_raise_without_the_checker(monkeypatch):
    from pytorchdeeplearing_amd import _capi
    from pytorchdeeplearing_amd.augment import apply_transform
    monkeypatch.setattr(_capi, "lib_for", getattr(_capi, "product_lib_for", _capi.lib_for))
    with pytest.raises(RuntimeError, match="MI355X"):
        apply_transform(torch.zeros(2, 2, 2, 1), np.eye(4)[:3])


def test_shim_packages_and_the_model_attribute():
    import dataprocess.Augmentation as pkg
    from dataprocess.Augmentation.ImageAugmentation import DataAug3D
    from dataprocess.Augmentation.images_masks_3dtransform import ImageDataGenerator3D, NumpyArrayIterator  # noqa: F401
    from pytorchdeeplearing_amd import augment
    from pytorchdeeplearing_amd.model.seg_models import _SegModel
    assert DataAug3D is augment.DataAug3D is pkg.DataAug3D and ImageDataGenerator3D is augment.ImageDataGenerator3D
    assert _SegModel.augment is None


class _Batches:
    """a loader that hands out prepared batches (no sampler: the prefetcher iterates it with one reader thread)"""

    def __init__(self, batches):
        self.batches = batches

    def __len__(self):
        return len(self.batches)

    def __iter__(self):
        return iter(self.batches)


@pytest.mark.parametrize("label_dtype", [torch.uint8, torch.int64], ids=["u8", "i64"])
def test_prefetcher_augments_each_batch_with_the_draws_in_sample_order(dev, label_dtype):
    from pytorchdeeplearing_amd.augment import ImageDataGenerator3D, apply_transform, draw_transform
    from pytorchdeeplearing_amd.model.pipeline import DevicePrefetcher
    rng = np.random.default_rng(3)
    shape = (2, 2, 4, 6, 10)                                      # (N, C, D, H, W)
    batches = []
    for b in range(2):
        y = rng.integers(0, 3, size=(2, 4, 6, 10))
        if label_dtype == torch.int64:
            y[0, 0, 0, 0] = 300                                   # (ids that do not fit a byte keep int64 through the pipeline)
        batches.append({"image": torch.from_numpy(rng.standard_normal(shape).astype(np.float32)),
                        "label": torch.from_numpy(y).to(label_dtype)})
    gen = ImageDataGenerator3D(rotation_range=20, width_shift_range=0.1, height_shift_range=0.1, depth_shift_range=0.1, zoom_range=0.2,
                               channel_shift_range=0.3, horizontal_flip=True, depth_flip=True, rescale=1.1)
    plain = list(DevicePrefetcher(_Batches(batches), dev, binary=False))
    np.random.seed(21)
    got = list(DevicePrefetcher(_Batches(batches), dev, binary=False, augment=gen))
    after = np.random.random()
    np.random.seed(21)
    assert len(got) == 2
    for (px, py), (gx, gy), batch in zip(plain, got, batches):
        assert np.array_equal(px.cpu().numpy(), batch["image"].numpy()) and np.array_equal(py.cpu().numpy(), batch["label"].numpy())
        assert gx.device == px.device and gx.dtype == torch.float32 and gx.shape == px.shape and gy.dtype == label_dtype and gy.shape == py.shape
        for k in range(2):
            m, f, s = draw_transform(gen, (4, 6, 10, 2))
            wx, wy = apply_transform(batch["image"][k].numpy(), m, f, "nearest", 0., label=batch["label"][k].numpy(), channel_shift=s, rescale=1.1,
                                     layout="th", device=dev)
            assert np.array_equal(gx[k].cpu().numpy(), wx) and np.array_equal(gy[k].cpu().numpy(), wy)
            assert not np.array_equal(wx, batch["image"][k].numpy())
    assert np.random.random() == after


def test_dataaug3d_writes_the_reference_files(dev, tmp_path):
    from pytorchdeeplearing_amd.augment import DataAug3D
    rng = np.random.default_rng(5)
    rows = []
    for r in range(2):
        img, msk = tmp_path / ("img%d.npy" % r), tmp_path / ("msk%d.npy" % r)
        np.save(img, rng.standard_normal((4, 6, 10)).astype(np.float32))
        np.save(msk, ((rng.random((4, 6, 10)) < 0.4) * 255).astype(np.uint8))
        rows.append("%s,%s" % (img, msk))
    csv_path = tmp_path / "train.csv"
    csv_path.write_text("Image,Mask\n" + "\n".join(rows) + "\n")
    out = str(tmp_path / "aug") + os.sep
    np.random.seed(2)
    DataAug3D(device=dev).DataAugmentation(str(csv_path), number=2, aug_path=out)
    assert sorted(os.listdir(out + "Image")) == sorted(os.listdir(out + "Mask")) == ["0_1.npy", "0_2.npy", "1_1.npy", "1_2.npy"]
    src = np.load(tmp_path / "img0.npy")
    for name in os.listdir(out + "Image"):
        im, mk = np.load(out + "Image/" + name), np.load(out + "Mask/" + name)
        assert im.shape == (4, 6, 10) and im.dtype == np.float64 and mk.shape == (4, 6, 10) and mk.dtype == np.uint8
        assert set(np.unique(mk)) <= {0, 255}
    # every written value is an input value times (float)1.1 (order 0 copies, the default rescale multiplies)
    assert np.isin(np.load(out + "Image/0_1.npy").astype(np.float32), src * np.float32(1.1)).all()


def test_golden_file_is_what_the_live_reference_computes():
    import make_augment_golden as mk
    if not mk.reference_available():
        pytest.skip("reference tree not present")
    mod = mk.load_reference()
    g = gold()
    assert tuple(c[0] for c in mk.CASES) == NAMES
    for i, c in enumerate(mk.CASES):
        res = mk.reference_case(mod, c)
        assert mk.check_case(c, res) >= (1e-9 if c[6] else 0.0)
        assert set(res) == set(case(i))
        for k, v in res.items():
            assert np.asarray(v).tobytes() == np.ascontiguousarray(case(i)[k]).tobytes() and np.asarray(v).dtype == case(i)[k].dtype, (c[0], k)
    flow, _ = mk.reference_flow(mod)
    for k, v in flow.items():
        assert np.array_equal(v, g[k]), k
