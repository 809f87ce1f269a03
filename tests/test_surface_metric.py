"""Seg_Metirc3d / surface_metrics (pytorchdeeplearing_amd/metric.py over csrc/surface.hip) against the reference class (model/metric.py:11-142).

tests/golden/surface_metric.npz holds what the live reference computes for four pairs of bool masks (tools/make_surface_golden.py) with spacing
(1, 1, 1) and (0.78, 0.78, 2.5); surface points real / pred:
  tiny_5x7x9     176 / 127     every extent below one wave, masks touch the volume faces, less than one LDS tile, one workgroup in the scan
  slab_3x130x67  15512 / 4939  W no multiple of 64, every voxel has an out-of-volume neighbour along z; many tiles, counts no multiple of the tile or of
                               the queries per thread, the target list split over workgroups and combined with atomicMin
  blob_12x20x70  2492 / 2822   an interior blob against salt noise
  voxel_4x5x6    1 / 96        one query point against the shell of the full volume (ASSD 2.676301764188125, MSD 4.123105625617661)

Tolerances.  Surface lists and the overlap counts are integers: exact (the six overlap metrics to 1e-12 relative, the Python arithmetic is the
reference's).  Unit spacing: every d^2 is an integer below 2^24, the f32 minimum is exact: round(nn^2) == round(nn_ref^2), a condition.  Anisotropic
spacing: rtol 1e-5 - the differences are exact integers, the spacings are rounded to f32 (2^-24), three products and two additions follow: at most
about 6 * 2^-24 = 4e-7 relative on d^2, half of it after the root, the sums are f64; 1e-5 leaves a factor of about 25 for the checker's libm."""
import os
import sys

import numpy as np
import pytest
import torch

import conftest
from conftest import GOLDEN, ROOT

sys.path.insert(0, os.path.join(ROOT, "tools"))

NAMES = ("tiny_5x7x9", "slab_3x130x67", "blob_12x20x70", "voxel_4x5x6")
METRICS = ("dice", "jaccard", "VOE", "RVD", "FNR", "FPR", "ASSD", "RMSD", "MSD")
_gold = None


def gold():
    global _gold
    if _gold is None:
        with np.load(os.path.join(GOLDEN, "surface_metric.npz")) as z:
            _gold = {k: z[k] for k in z.files}
        assert tuple(_gold["names"]) == NAMES
    return _gold


def masks(i):
    g = gold()
    shape = tuple(int(v) for v in g["c%d_shape" % i])
    n = int(np.prod(shape))
    return tuple(np.unpackbits(g["c%d_%s" % (i, s)])[:n].astype(bool).reshape(shape) for s in ("real", "pred"))


def spacing(j):
    return tuple(float(v) for v in gold()["spacings"][j])


def nine(m):
    return np.array([m.get_dice_coefficient()[0], m.get_jaccard_index(), m.get_VOE(), m.get_RVD(), m.get_FNR(), m.get_FPR(), m.get_ASSD(), m.get_RMSD(),
                     m.get_MSD()], dtype=np.float64)


def raw_call(dev, real, pred, cls, sp=(1.0, 1.0, 1.0)):
    """seg_surface_metrics through the C-ABI on uint8 volumes -> (out16, nn r2p, nn p2r) as numpy"""
    from pytorchdeeplearing_amd import _capi, metric
    r = torch.from_numpy(np.ascontiguousarray(real, dtype=np.uint8)).to(dev)
    p = torch.from_numpy(np.ascontiguousarray(pred, dtype=np.uint8)).to(dev)
    lib = _capi.lib_for(dev)
    ws = metric._surface_ws(lib, tuple(r.shape), dev)
    out = torch.empty(16, dtype=torch.float64, device=dev)
    nn = [torch.empty(r.numel(), dtype=torch.float32, device=dev) for _ in range(2)]
    metric._surface_call(lib, r, p, cls, sp[::-1], ws, out, nn[0], nn[1])
    o = out.cpu().numpy()
    return o, nn[0][:int(o[4])].cpu().numpy(), nn[1][:int(o[5])].cpu().numpy()


def label_volumes(n=2, shape=(6, 11, 70), seed=5):
    """label volumes with values {0, 1, 2, 3}: three boxes per sample with salt noise of other labels; class 3 is absent from sample 1 of `pred`"""
    rng = np.random.default_rng(seed)
    vols = []
    for side in range(2):
        v = np.zeros((n,) + shape, dtype=np.uint8)
        for i in range(n):
            for c in (1, 2, 3):
                z0, y0, x0 = rng.integers(0, 3), rng.integers(0, 5), rng.integers(0, 40)
                v[i, z0:z0 + 3, y0:y0 + 5, x0 + 4 * c:x0 + 4 * c + 20] = c
            noise = rng.random(shape) < 0.03
            v[i][noise] = rng.integers(0, 4, size=int(noise.sum()))
        vols.append(v)
    vols[1][1][vols[1][1] == 3] = 0
    return vols


@pytest.mark.parametrize("j", [0, 1], ids=["unit", "aniso"])
@pytest.mark.parametrize("i", range(4), ids=NAMES)
def test_matches_the_reference_class(dev, i, j):
    from pytorchdeeplearing_amd.metric import Seg_Metirc3d
    g = gold()
    real, pred = masks(i)
    sp = spacing(j)
    m = Seg_Metirc3d(real, pred, sp, device=dev)
    d, h, w = real.shape
    zyx = np.array(sp[::-1]).reshape(1, 3)
    for side, pts in (("real", m.real_mask_surface_pts), ("pred", m.pred_mask_surface_pts)):
        ref_idx = g["c%d_surf_%s" % (i, side)].astype(np.int64)
        assert pts.shape == (len(ref_idx), 3) and pts.dtype == np.float64
        np.testing.assert_array_equal(m._surface_indices(side == "pred"), ref_idx)          # same count, same order
        np.testing.assert_allclose(pts, np.stack([ref_idx // (h * w), ref_idx // w % h, ref_idx % w], axis=1) * zyx, rtol=1e-15)
    want = g["c%d_s%d_values" % (i, j)]
    got = nine(m)
    print(NAMES[i], sp, "rel. deviation of the nine values:", np.abs(got - want) / np.maximum(np.abs(want), 1e-300))
    np.testing.assert_allclose(got[:6], want[:6], rtol=1e-12, atol=0)
    dice, num, den = m.get_dice_coefficient()
    assert dice == num / den and num == 2 * int((real & pred).sum()) and den == int(real.sum()) + int(pred.sum())
    for name, nn in (("nn_r2p", m.real2pred_nn), ("nn_p2r", m.pred2real_nn)):
        ref = g["c%d_s%d_%s" % (i, j, name)]
        assert nn.shape == ref.shape
        if j == 0:
            np.testing.assert_array_equal(np.rint(nn ** 2), np.rint(ref ** 2))
        else:
            np.testing.assert_allclose(nn, ref, rtol=1e-5, atol=0)
    np.testing.assert_allclose(got[6:], want[6:], rtol=1e-5, atol=0)
    if i == 3 and j == 0:
        np.testing.assert_allclose([m.get_ASSD(), m.get_MSD()], [2.676301764188125, 4.123105625617661], rtol=1e-5, atol=0)


@pytest.mark.parametrize("i", [1, 2], ids=[NAMES[1], NAMES[2]])
def test_two_calls_agree_bit_for_bit(dev, i):
    real, pred = masks(i)
    a = raw_call(dev, real, pred, -1, spacing(1))
    b = raw_call(dev, real, pred, -1, spacing(1))
    for x, y in zip(a, b):
        assert x.tobytes() == y.tobytes()
    assert a[0][4] == len(gold()["c%d_surf_real" % i]) and np.all(a[0][12:] == 0)


def test_class_selector_equals_the_binary_call_on_that_class(dev):
    real, pred = label_volumes()
    for c in (0, 1, 2, 3):
        a = raw_call(dev, real[0], pred[0], c, spacing(1))
        b = raw_call(dev, (real[0] == c), (pred[0] == c), -1, spacing(1))
        assert a[0][4] > 0 and a[0][5] > 0
        for x, y in zip(a, b):
            assert x.tobytes() == y.tobytes()


def test_batched_form_equals_the_pairs_and_gives_nan_for_an_absent_class(dev):
    from pytorchdeeplearing_amd.metric import SURFACE_METRICS, Seg_Metirc3d, surface_metrics
    real, pred = label_volumes()
    classes = [1, 2, 3]
    sp = spacing(1)
    res = surface_metrics(real, pred, sp, classes, device=dev)
    assert tuple(res) == SURFACE_METRICS == METRICS
    res_t = surface_metrics(torch.from_numpy(real).to(dev), torch.from_numpy(pred.astype(np.int64)).to(dev), sp, [3])
    for name in METRICS:
        assert res[name].shape == (2, 3) and res[name].dtype == np.float64
        assert res[name][:, 2:].tobytes() == res_t[name].tobytes()
    for n in range(2):
        for k, c in enumerate(classes):
            got = np.array([res[name][n, k] for name in METRICS])
            if n == 1 and c == 3:
                assert np.all(np.isnan(got))
                continue
            want = nine(Seg_Metirc3d(real[n] == c, pred[n] == c, sp, device=dev))
            np.testing.assert_allclose(got, want, rtol=1e-15, atol=0)


def test_numpy_and_torch_bool_and_uint8_inputs_give_the_same_numbers(dev):
    from pytorchdeeplearing_amd.metric import Seg_Metirc3d
    real, pred = masks(0)
    sp = spacing(1)
    base = Seg_Metirc3d(real, pred, sp, device=dev)
    want = nine(base)
    assert want[3] < 0                   # RVD: the prediction is the smaller mask; signed arithmetic for every input dtype
    np.testing.assert_allclose(want[3], gold()["c0_s1_values"][3], rtol=1e-12)
    variants = [(real.astype(np.uint8) * 255, pred.astype(np.uint8)), (real.astype(np.int64), pred.astype(np.int32) * 7),
                (torch.from_numpy(real).to(dev), torch.from_numpy(pred).to(dev)),
                (torch.from_numpy(real.astype(np.uint8) * 3).to(dev), torch.from_numpy(pred.astype(np.int64)).to(dev))]
    for r, p in variants:
        m = Seg_Metirc3d(r, p, sp, device=dev)
        assert nine(m).tobytes() == want.tobytes()
        assert m.real2pred_nn.tobytes() == base.real2pred_nn.tobytes() and m.pred2real_nn.tobytes() == base.pred2real_nn.tobytes()
    with pytest.raises(TypeError):
        Seg_Metirc3d(real.astype(np.float32), pred, sp, device=dev)


def test_empty_masks_and_bad_arguments(dev):
    from pytorchdeeplearing_amd import _capi
    from pytorchdeeplearing_amd.metric import Seg_Metirc3d
    real, pred = masks(0)
    none = np.zeros_like(real)
    for r, p in ((none, pred), (real, none), (none, none)):
        with pytest.raises(ValueError):
            Seg_Metirc3d(r, p, (1, 1, 1), device=dev)
    # the call itself runs to completion on an empty side: counts right, distance fields NaN
    o, nn_r, nn_p = raw_call(dev, none, pred, -1)
    ref_surf = len(gold()["c0_surf_pred"])
    assert list(o[:6]) == [0, pred.sum(), 0, pred.sum(), 0, ref_surf] and np.all(np.isnan(o[6:12])) and np.all(o[12:] == 0)
    assert len(nn_r) == 0 and len(nn_p) == ref_surf
    o = raw_call(dev, real, none, -1)[0]
    assert list(o[:6]) == [real.sum(), 0, 0, real.sum(), len(gold()["c0_surf_real"]), 0] and np.all(np.isnan(o[6:12]))
    # argument checks: nothing is launched (out16 keeps its content)
    lib = _capi.lib_for(dev)
    r = torch.from_numpy(real.astype(np.uint8)).to(dev)
    p = torch.from_numpy(pred.astype(np.uint8)).to(dev)
    ws = torch.empty(int(lib.seg_surface_ws_bytes(5, 7, 9)) + 256, dtype=torch.uint8, device=dev)
    out = torch.full((16,), -7.0, dtype=torch.float64, device=dev)
    st = _capi.stream_for(dev)
    bad = [(None, p.data_ptr(), 5, 7, 9, ws.data_ptr(), out.data_ptr()), (r.data_ptr(), None, 5, 7, 9, ws.data_ptr(), out.data_ptr()),
           (r.data_ptr(), p.data_ptr(), 5, 7, 9, None, out.data_ptr()), (r.data_ptr(), p.data_ptr(), 5, 7, 9, ws.data_ptr(), None),
           (r.data_ptr(), p.data_ptr(), 0, 7, 9, ws.data_ptr(), out.data_ptr()), (r.data_ptr(), p.data_ptr(), 5, 0, 9, ws.data_ptr(), out.data_ptr()),
           (r.data_ptr(), p.data_ptr(), 5, 7, 0, ws.data_ptr(), out.data_ptr()), (r.data_ptr(), p.data_ptr(), 5, 7, 2049, ws.data_ptr(), out.data_ptr())]
    for a, b, d, h, w, wsp, op in bad:
        rc = lib.seg_surface_metrics(a, b, d, h, w, -1, 1.0, 1.0, 1.0, wsp, op, None, None, st)
        assert rc != 0 and b"seg_surface_metrics" in lib.seg_last_error()
    assert lib.seg_surface_ws_bytes(0, 7, 9) < 0 and lib.seg_surface_ws_bytes(2048, 2048, 2048) < 0
    assert np.all(out.cpu().numpy() == -7.0)
    # worst case (every voxel a surface voxel): four uint32 per voxel fit the workspace
    assert lib.seg_surface_ws_bytes(5, 7, 9) >= 16 * 5 * 7 * 9


def test_checkerboard_fills_the_worst_case_workspace(dev):
    """every voxel of a checkerboard is a surface voxel of one of the two sides: the lists the workspace is sized for"""
    z, y, x = np.meshgrid(np.arange(4), np.arange(6), np.arange(66), indexing="ij")
    board = (z + y + x) % 2 == 0
    o, nn_r, nn_p = raw_call(dev, board, ~board, -1)
    n = board.size
    assert list(o[:6]) == [n // 2, n // 2, 0, n, n // 2, n // 2]
    assert np.all(nn_r == 1.0) and np.all(nn_p == 1.0) and o[6] == n // 2 and o[10] == 1.0


def test_golden_file_is_what_the_live_reference_computes():
    from oracle import ref_loader
    if not ref_loader.available():
        pytest.skip("reference tree not present")
    import make_surface_golden as mk
    ref_metric = ref_loader.load()[2]
    g = gold()
    cases = mk.make_cases()
    assert tuple(c[0] for c in cases) == NAMES
    for i, (name, real, pred) in enumerate(cases):
        r, p = masks(i)
        assert np.array_equal(r, real) and np.array_equal(p, pred), name
        for j in range(2):
            res = mk.reference_results(ref_metric, r, p, spacing(j))
            np.testing.assert_array_equal(res["surf_real"], g["c%d_surf_real" % i])
            np.testing.assert_array_equal(res["surf_pred"], g["c%d_surf_pred" % i])
            np.testing.assert_allclose(res["values"], g["c%d_s%d_values" % (i, j)], rtol=1e-12, atol=0)
            np.testing.assert_allclose(res["nn_r2p"], g["c%d_s%d_nn_r2p" % (i, j)], rtol=1e-15, atol=0)
            np.testing.assert_allclose(res["nn_p2r"], g["c%d_s%d_nn_p2r" % (i, j)], rtol=1e-15, atol=0)
