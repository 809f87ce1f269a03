"""seg_edt (csrc/edt.hip) and its prepost wrappers against tests/edt_oracle.py, the float64 brute force over all background voxels.  Unit spacing is checked
for EQUALITY (the computation is integer); the anisotropic spacing to 1e-5 relative: index differences are exact, the spacings are rounded to f32, a few
f32 products and additions give about 6 * 2^-24 on d^2 (half of it after the root), and the separable passes add at most one rounding per axis - the
derivation tests/test_surface_metric.py uses for the same arithmetic."""
import numpy as np
import pytest
import torch

import edt_oracle as oracle
from edt_oracle import ANISO, CASES, PAIRS, UNIT

SQUARED, DISTANCE, SIGNED, BOUNDARY = 0, 1, 2, 3
IDS = ["%s-cls%d" % p for p in PAIRS]


def edt(dev, vol, cls=-1, sampling=UNIT, mode=DISTANCE):
    """one seg_edt call through the C-ABI on the shared workspace cache; the output is pre-filled with NaN, so an element left out shows"""
    from pytorchdeeplearing_amd import _capi, prepost
    lib = _capi.lib_for(dev)
    t = torch.from_numpy(np.array(vol)).to(dev)                   # (a copy: the cases are read-only)
    n, d, h, w = vol.shape
    out = torch.full(vol.shape, float("nan"), dtype=torch.float32, device=dev)
    nbytes = lib.seg_edt_ws_bytes(n, d, h, w)
    lib.check(nbytes, "seg_edt_ws_bytes")
    ws = prepost._pp_workspace(dev, nbytes)
    lib.check(lib.seg_edt(t.data_ptr(), n, d, h, w, cls, *sampling, mode, ws.data_ptr(), out.data_ptr(), d * h * w, _capi.stream_for(dev)), "seg_edt")
    return out.cpu().numpy()


def close_to_oracle(got, ref):
    """f32 result against the float64 oracle of a signed / boundary map with unit spacing: one f32 rounding of the root (2^-24 relative, absolute once the
    1 is taken off) and one of the result"""
    np.testing.assert_allclose(got, ref, rtol=0, atol=2.0 ** -23 * max(1.0, np.abs(ref).max()))
    return True


def check_both_kinds(name, cls):
    m = oracle.fg_of(CASES[name], cls)
    if name in oracle.RANDOM:
        for s in m:
            assert s.any() and not s.all(), name


def scipy_sq(name, cls, sampling):
    """scipy's squared transform of the samples that have a background voxel (its result without one is unspecified), or None without scipy"""
    try:
        from scipy import ndimage
    except ImportError:
        return None
    m = oracle.fg_of(CASES[name], cls)
    return [ndimage.distance_transform_edt(s, sampling=sampling) ** 2 if not s.all() else None for s in m]


@pytest.mark.parametrize("name,cls", PAIRS, ids=IDS)
def test_unit_spacing_is_exact(dev, name, cls):
    check_both_kinds(name, cls)
    want = oracle.batch_sq(name, cls)
    assert np.array_equal(want, np.rint(want))
    sp = scipy_sq(name, cls, UNIT)
    if sp is not None:
        for s, ref in enumerate(sp):
            if ref is not None:
                assert np.array_equal(np.rint(ref), want[s]) and np.abs(ref - want[s]).max() < 1e-9
    got = edt(dev, CASES[name], cls, UNIT, SQUARED)
    assert got.dtype == np.float32 and np.array_equal(got, want.astype(np.float32))
    got = edt(dev, CASES[name], cls, UNIT, DISTANCE)
    assert np.array_equal(np.rint(got.astype(np.float64) ** 2), want)


@pytest.mark.parametrize("name,cls", PAIRS, ids=IDS)
def test_anisotropic_spacing(dev, name, cls):
    check_both_kinds(name, cls)
    want = oracle.batch_sq(name, cls, ANISO)
    sp = scipy_sq(name, cls, ANISO)
    if sp is not None:
        for s, ref in enumerate(sp):
            if ref is not None:
                np.testing.assert_allclose(ref, want[s], rtol=1e-12, atol=0)
    for mode, ref in ((SQUARED, want), (DISTANCE, np.sqrt(want))):
        got = edt(dev, CASES[name], cls, ANISO, mode).astype(np.float64)
        nz = ref > 0
        dev_rel = float(np.max(np.abs(got[nz] - ref[nz]) / ref[nz])) if nz.any() else 0.0
        print("edt %s cls %d mode %d: largest relative deviation %.3g" % (name, cls, mode, dev_rel))
        np.testing.assert_allclose(got, ref, rtol=1e-5, atol=0)


def complement_volume(name, cls):
    """uint8 volume whose non-zero voxels are the background of (case, cls)"""
    return (~oracle.fg_of(CASES[name], cls)).astype(np.uint8)


@pytest.mark.parametrize("name,cls", PAIRS, ids=IDS)
def test_signed_and_boundary_modes(dev, name, cls):
    """modes 2 / 3 = the combination of the two one-sided distance maps: exactly that of two mode-1 calls with unit spacing, to 1e-5 of the oracle's
    otherwise (mode 3 with an absolute allowance of 1e-5 * max |phi|: its `- 1` cancels)"""
    check_both_kinds(name, cls)
    m = oracle.fg_of(CASES[name], cls)
    din = edt(dev, CASES[name], cls, UNIT, DISTANCE)
    dout = edt(dev, complement_volume(name, cls), -1, UNIT, DISTANCE)
    boundary = np.array([s.any() and not s.all() for s in m]).reshape(-1, 1, 1, 1)
    one = np.float32(1)
    for mode in (SIGNED, BOUNDARY):
        inside = din - one if mode == BOUNDARY else din
        with np.errstate(invalid="ignore"):
            want = np.where(boundary, np.where(m, -inside, dout), np.float32(0))
        got = edt(dev, CASES[name], cls, UNIT, mode)
        assert np.array_equal(got, want), (name, cls, mode)
        close_to_oracle(got, oracle.combined(name, cls, UNIT, mode))
        ref = oracle.combined(name, cls, ANISO, mode)
        got = edt(dev, CASES[name], cls, ANISO, mode).astype(np.float64)
        np.testing.assert_allclose(got, ref, rtol=1e-5, atol=1e-5 * np.abs(ref).max() if mode == BOUNDARY else 0)
    if (name, cls) == ("labels", 3):
        assert not m[1].any() and not np.any(edt(dev, CASES[name], cls, UNIT, BOUNDARY)[1])


def test_samples_without_a_boundary(dev):
    vol = CASES["full_empty"]
    assert vol[0].all() and not vol[1].any()
    for sampling in (UNIT, ANISO):
        for mode in (SQUARED, DISTANCE):
            got = edt(dev, vol, -1, sampling, mode)
            assert np.all(np.isposinf(got[0])) and np.all(got[1] == 0)
        for mode in (SIGNED, BOUNDARY):
            got = edt(dev, vol, -1, sampling, mode)
            assert np.all(got == 0) and not np.isnan(got).any()
    for mode in (SIGNED, BOUNDARY):
        assert np.all(edt(dev, CASES["labels"], 3, UNIT, mode)[1] == 0)


def test_out_stride_writes_class_planes_in_place(dev):
    from pytorchdeeplearing_amd import _capi, prepost
    vol = CASES["labels"]
    n, d, h, w = vol.shape
    v = d * h * w
    lib = _capi.lib_for(dev)
    t = torch.from_numpy(vol.copy()).to(dev)
    sentinel = -12345.0
    out = torch.full((n, 3, v + 5), sentinel, dtype=torch.float32, device=dev)      # 5 floats of slack behind every plane
    ws = prepost._pp_workspace(dev, lib.seg_edt_ws_bytes(n, d, h, w))
    classes = (1, 2, 3)
    for k, cls in enumerate(classes):
        lib.check(lib.seg_edt(t.data_ptr(), n, d, h, w, cls, *UNIT, DISTANCE, ws.data_ptr(), out.data_ptr() + 4 * k * (v + 5), 3 * (v + 5),
                              _capi.stream_for(dev)), "seg_edt")
    got = out.cpu().numpy()
    for k, cls in enumerate(classes):
        assert np.array_equal(got[:, k, :v].reshape(vol.shape), edt(dev, vol, cls, UNIT, DISTANCE))
    assert np.all(got[:, :, v:] == sentinel)
    # the (2, 3, v) tensor of the issue: dense planes
    out = torch.full((n, 3, v), sentinel, dtype=torch.float32, device=dev)
    lib.check(lib.seg_edt(t.data_ptr(), n, d, h, w, 2, *UNIT, DISTANCE, ws.data_ptr(), out.data_ptr() + 4 * v, 3 * v, _capi.stream_for(dev)), "seg_edt")
    got = out.cpu().numpy()
    assert np.all(got[:, 0] == sentinel) and np.all(got[:, 2] == sentinel)
    assert np.array_equal(got[:, 1].reshape(vol.shape), edt(dev, vol, 2, UNIT, DISTANCE))


def test_repeatable_and_no_stale_workspace(dev):
    """slab, tiny, slab on the one cached workspace: the second slab result is the first, bit for bit, and tiny is right in between"""
    for sampling, mode in ((UNIT, SQUARED), (ANISO, BOUNDARY)):
        a = edt(dev, CASES["slab"], -1, sampling, mode)
        t = edt(dev, CASES["tiny"], -1, sampling, mode)
        b = edt(dev, CASES["slab"], -1, sampling, mode)
        assert a.tobytes() == b.tobytes()
        assert t.tobytes() == edt(dev, CASES["tiny"], -1, sampling, mode).tobytes()
    assert np.array_equal(edt(dev, CASES["tiny"], -1, UNIT, SQUARED), oracle.batch_sq("tiny").astype(np.float32))


def test_argument_errors_launch_nothing(dev):
    from pytorchdeeplearing_amd import _capi, prepost
    lib = _capi.lib_for(dev)
    n, d, h, w = 1, 3, 4, 5
    v = d * h * w
    t = torch.ones((n, d, h, w), dtype=torch.uint8, device=dev)
    t[0, 1, 2, 3] = 0
    out = torch.full((v,), 7.0, dtype=torch.float32, device=dev)
    ws = prepost._pp_workspace(dev, lib.seg_edt_ws_bytes(2, 8, 8, 8))
    good = dict(labels=t.data_ptr(), n=n, d=d, h=h, w=w, cls=-1, sz=1.0, sy=1.0, sx=1.0, mode=DISTANCE, ws=ws.data_ptr(), out=out.data_ptr(), stride=v)

    def call(**kw):
        a = dict(good, **kw)
        return lib.seg_edt(a["labels"], a["n"], a["d"], a["h"], a["w"], a["cls"], a["sz"], a["sy"], a["sx"], a["mode"], a["ws"], a["out"], a["stride"],
                           _capi.stream_for(dev))

    bad = [dict(d=0), dict(h=0), dict(w=0), dict(d=2049), dict(h=2049), dict(w=2049), dict(n=0), dict(n=65536), dict(sz=0.0), dict(sy=-1.0),
           dict(sx=float("nan")), dict(sy=float("inf")), dict(mode=4), dict(mode=-1), dict(stride=v - 1), dict(cls=256), dict(cls=-2),
           dict(labels=None), dict(ws=None), dict(out=None), dict(d=2048, h=2048, w=512)]
    for kw in bad:
        rc = call(**kw)
        assert rc < 0, kw
        with pytest.raises(RuntimeError, match="seg_edt"):
            lib.check(rc, "seg_edt")
        assert lib.seg_last_error().decode().startswith("seg_edt"), kw
    for kw in (dict(d=0), dict(w=2049), dict(n=0), dict(n=65536), dict(d=2048, h=2048, w=512)):
        a = dict(good, **kw)
        assert lib.seg_edt_ws_bytes(a["n"], a["d"], a["h"], a["w"]) < 0
    assert np.all(out.cpu().numpy() == 7.0)
    lib.check(call(), "seg_edt")                                  # and the good call is one
    got = out.cpu().numpy().reshape(d, h, w)
    assert got[1, 2, 3] == 0 and got[1, 2, 2] == 1 and got[0, 0, 0] == np.float32(np.sqrt(1 + 4 + 9))


def test_prepost_wrappers(dev):
    from pytorchdeeplearing_amd import _capi, prepost
    vol = CASES["labels"]
    t4 = torch.from_numpy(vol.copy()).to(dev)
    want = np.sqrt(oracle.batch_sq("labels", -1))
    got = prepost.distance_transform_edt(t4)
    assert got.dtype == torch.float32 and tuple(got.shape) == vol.shape and got.device == t4.device
    np.testing.assert_allclose(got.cpu().numpy(), want, rtol=1e-6, atol=0)
    got3 = prepost.distance_transform_edt(t4[1])                  # (D, H, W)
    assert tuple(got3.shape) == vol.shape[1:] and torch.equal(got3, got[1])
    sq = prepost.distance_transform_edt(t4, cls=2, squared=True)
    assert np.array_equal(sq.cpu().numpy(), oracle.batch_sq("labels", 2).astype(np.float32))
    an = prepost.distance_transform_edt(t4, sampling=ANISO)
    np.testing.assert_allclose(an.cpu().numpy(), np.sqrt(oracle.batch_sq("labels", -1, ANISO)), rtol=1e-5, atol=0)
    sc = prepost.distance_transform_edt(t4, sampling=2.0)         # a scalar spacing scales the map
    np.testing.assert_allclose(sc.cpu().numpy(), 2.0 * want, rtol=1e-6, atol=0)
    buf = torch.empty(vol.shape, dtype=torch.float32, device=dev)
    assert prepost.distance_transform_edt(t4, out=buf) is buf and torch.equal(buf, got)
    sd = prepost.signed_distance_map(t4, cls=2, out=buf)
    assert sd is buf and close_to_oracle(sd.cpu().numpy(), oracle.combined("labels", 2, UNIT, SIGNED))
    # the maps of the boundary loss: 3-D labels with four classes, one class, and a 2-D batch run as d = 1
    maps = prepost.boundary_distance_maps(t4, 4)
    assert tuple(maps.shape) == (2, 4) + vol.shape[1:] and maps.dtype == torch.float32
    for k in range(4):
        close_to_oracle(maps[:, k].cpu().numpy(), oracle.combined("labels", k, UNIT, BOUNDARY))
    one = prepost.boundary_distance_maps(t4.to(torch.int64), 1)
    assert tuple(one.shape) == (2, 1) + vol.shape[1:]
    close_to_oracle(one[:, 0].cpu().numpy(), oracle.combined("labels", -1, UNIT, BOUNDARY))
    flat = torch.from_numpy(CASES["plane2d"][:, 0].copy()).to(dev)
    m2 = prepost.boundary_distance_maps(flat, 1, sampling=(0.78, 0.78))
    assert tuple(m2.shape) == (2, 1, 300, 70)
    ref = oracle.combined("plane2d", -1, (1.0, 0.78, 0.78), BOUNDARY)[:, 0]
    np.testing.assert_allclose(m2[:, 0].cpu().numpy(), ref, rtol=1e-5, atol=1e-5 * np.abs(ref).max())
    mbuf = torch.empty((2, 4) + vol.shape[1:], dtype=torch.float32, device=dev)
    assert prepost.boundary_distance_maps(t4, 4, out=mbuf) is mbuf and torch.equal(mbuf, maps)
    # what must raise
    with pytest.raises(TypeError):
        prepost.distance_transform_edt(t4.float())
    with pytest.raises(TypeError):
        prepost.distance_transform_edt(t4[0, 0])
    with pytest.raises(ValueError):
        prepost.distance_transform_edt(t4, out=torch.empty(vol.shape, dtype=torch.float64, device=dev))
    with pytest.raises(ValueError):
        prepost.distance_transform_edt(t4, out=torch.empty(vol.shape[1:], dtype=torch.float32, device=dev))
    with pytest.raises(ValueError):
        prepost.distance_transform_edt(t4, sampling=(1.0, 2.0))
    with pytest.raises(RuntimeError):
        prepost.distance_transform_edt(t4, sampling=(1.0, 0.0, 1.0))
    with pytest.raises(TypeError):
        prepost.boundary_distance_maps(t4.float(), 4)
    with pytest.raises(ValueError):
        prepost.boundary_distance_maps(t4, 4, out=torch.empty((2, 3) + vol.shape[1:], dtype=torch.float32, device=dev))
    with pytest.raises(RuntimeError):                             # CPU tensors raise outside the checker
        getattr(_capi, "product_lib_for", _capi.lib_for)(torch.device("cpu"))
