"""Mask post-processing (pytorchdeeplearing_amd/prepost.py over csrc/postproc.hip; the shims in dataprocess/utils.py) against scipy.ndimage.

tests/golden/postproc.npz holds what scipy computes (tools/make_postproc_golden.py): masks, label volumes and the 32 statistics per sample for faces /
fully connected labelling, and the SHA-256 + voxel count of every morphology result.  Where scipy can be imported the same comparisons also run against
the live functions.  Everything is integer: every comparison is exact.

  tiny 5x7x9          every extent below one wave and one word; the mask touches all faces           K 11 / 1
  slab 3x130x67       W no multiple of 64 (padding bits), many workgroup seams in y                  K 478 / 2, top sizes 12376, 27
  noise 12x20x70      many roots per wave for the size aggregation                                   K 796 / 4
  sparse 9x33x129     W = 2 words + 1 bit; a scan over thousands of roots                            K 2404 / 15
  plane 1x40x200      2-D, 4- and 8-connectivity                                                     K 404 / 18
  batch 2x6x11x70     samples must not join; per-sample statistics (largest 64 and 65)               K 336, 366 / 4, 6
  serpentine 4x9x70   one component of 1416 voxels whose label crosses every seam along a path far longer than any extent
  tiles 19x23x150     p = .4, faces: every extent above the unit's tile (a 64-voxel word; 256 consecutive words per workgroup, 2.7 rows of z) and no
                      multiple of it
"""
import functools
import hashlib
import os
import sys

import numpy as np
import pytest
import torch

import conftest
from conftest import GOLDEN, ROOT

sys.path.insert(0, os.path.join(ROOT, "tools"))
import make_postproc_golden as mk          # noqa: E402  (case list, structuring elements; scipy only inside its *_ref functions)

try:
    from scipy import ndimage              # noqa: F401
    HAVE_SCIPY = True
except ImportError:
    HAVE_SCIPY = False

CC_CASES = mk.CC_CASES
_gold = None


def gold():
    global _gold
    if _gold is None:
        with np.load(os.path.join(GOLDEN, "postproc.npz")) as z:
            _gold = {k: z[k] for k in z.files}
        _gold["morph"] = {k: (s, int(c)) for k, s, c in zip(_gold["morph_keys"], _gold["morph_sha256"], _gold["morph_count"])}
    return _gold


def mask_of(name):
    g = gold()
    shape = tuple(int(v) for v in g[name + "_shape"])
    return np.unpackbits(g[name + "_mask"])[:int(np.prod(shape))].astype(bool).reshape(shape)


def up(arr, dev):
    return torch.from_numpy(np.array(arr, dtype=np.uint8)).to(dev)          # a copy: in-place calls on the checker must not reach the caller's array


def PP():
    from pytorchdeeplearing_amd import prepost
    return prepost


def label_call(dev, mask, conn=1, cls=None):
    lab, stats = PP().connected_components(up(mask, dev), conn, cls)
    return lab.cpu().numpy(), stats.cpu().numpy()


def ref_labels(name, conn):
    g = gold()
    return g["%s_lab%d" % (name, conn)].astype(np.int32), g["%s_stats%d" % (name, conn)]


def conns(name):
    return (1,) if name == "tiles" else (1, 3)


@pytest.mark.parametrize("name", CC_CASES)
def test_labels_and_stats_equal_scipy(dev, name):
    mask = mask_of(name)
    for conn in conns(name):
        want_lab, want_stats = ref_labels(name, conn)
        lab, stats = label_call(dev, mask, conn)
        assert lab.dtype == np.int32 and stats.dtype == np.int32 and stats.shape == (len(mk.samples(mask)), 32)
        print(name, conn, "K", stats[:, 0], "largest", stats[:, 2], "label", stats[:, 3])
        assert np.array_equal(lab, want_lab.reshape(mask.shape)), (name, conn)
        assert np.array_equal(stats, want_stats), (name, conn, stats[:, :17], want_stats[:, :17])
        if HAVE_SCIPY:
            for i, vol in enumerate(mk.samples(mask)):
                live, k = mk.label_ref(vol, conn)
                assert np.array_equal(mk.samples(lab)[i], live)
                assert np.array_equal(stats[i], mk.stats_ref(vol, live, k))


@pytest.mark.parametrize("name", CC_CASES)
def test_keep_largest_and_remove_small(dev, name):
    mask = mask_of(name)
    values = np.where(mask, 200, 0).astype(np.uint8)                         # the input VALUE survives, not a 1
    for conn in conns(name):
        lab, stats = ref_labels(name, conn)
        lab = lab.reshape((-1,) + mask.shape[-3:])
        big = np.stack([lab[i] == stats[i][3] for i in range(len(lab))]).reshape(mask.shape) & mask
        got = PP().keep_largest_component(up(values, dev), conn).cpu().numpy()
        assert np.array_equal(got, np.where(big, 200, 0))
        for min_voxels in (2, 10):
            keep = np.stack([np.isin(lab[i], 1 + np.flatnonzero(np.bincount(lab[i].ravel())[1:] >= min_voxels)) for i in range(len(lab))])
            got = PP().remove_small_components(up(values, dev), min_voxels, conn).cpu().numpy()
            assert np.array_equal(got, np.where(keep.reshape(mask.shape) & mask, 200, 0)), (name, conn, min_voxels)
    # in place
    t = up(values, dev)
    assert PP().keep_largest_component(t, 1, out=t) is t
    lab, stats = ref_labels(name, 1)
    lab = lab.reshape((-1,) + mask.shape[-3:])
    big = np.stack([lab[i] == stats[i][3] for i in range(len(lab))]).reshape(mask.shape) & mask
    assert np.array_equal(t.cpu().numpy(), np.where(big, 200, 0))
    t = up(values, dev)
    PP().remove_small_components(t, 10, 1, out=t)
    keep = np.stack([np.isin(lab[i], 1 + np.flatnonzero(np.bincount(lab[i].ravel())[1:] >= 10)) for i in range(len(lab))])
    assert np.array_equal(t.cpu().numpy(), np.where(keep.reshape(mask.shape) & mask, 200, 0))


def label_volume():
    """values 0..2 in 6x11x70 (the sum of two halves of the noise case); class 3 is absent"""
    m = mask_of("noise")
    return m[0:6, :11].astype(np.uint8) + m[6:12, :11].astype(np.uint8)


def test_cls_selects_one_value_and_an_absent_class_is_empty(dev):
    vol = label_volume()
    assert set(np.unique(vol)) == {0, 1, 2}
    for c in (0, 1, 2):
        lab, stats = label_call(dev, vol, 1, cls=c)
        lab_b, stats_b = label_call(dev, vol == c, 1)                         # the binary call on that class
        assert stats[0][0] > 1 and np.array_equal(lab, lab_b) and np.array_equal(stats, stats_b)
        kept = PP().keep_largest_component(up(vol, dev), 1, cls=c).cpu().numpy()
        assert np.array_equal(kept, np.where(lab == stats[0][3], c, 0))
        if HAVE_SCIPY:
            live, k = mk.label_ref(vol == c, 1)
            assert np.array_equal(lab, live) and np.array_equal(stats[0], mk.stats_ref(vol == c, live, k))
    lab, stats = label_call(dev, vol, 1, cls=3)
    assert not lab.any() and list(stats[0][:17]) == [0, 0, 0, 0, -1, 6, 11, 70, -1, -1, -1, 6, 11, 70, -1, -1, -1] and not stats[0][17:].any()
    assert not PP().keep_largest_component(up(vol, dev), 1, cls=3).cpu().numpy().any()


def test_all_zero_all_one_and_single_voxel(dev):
    shape = (3, 5, 66)
    lab, stats = label_call(dev, np.zeros(shape, bool))
    assert not lab.any() and list(stats[0][:17]) == [0, 0, 0, 0, -1, 3, 5, 66, -1, -1, -1, 3, 5, 66, -1, -1, -1]
    assert not PP().keep_largest_component(up(np.zeros(shape, bool), dev)).cpu().numpy().any()
    for conn in (1, 3):
        lab, stats = label_call(dev, np.ones(shape, bool), conn)
        assert (lab == 1).all() and list(stats[0][:17]) == [1, 990, 990, 1, 0, 0, 0, 0, 2, 4, 65, 0, 0, 0, 2, 4, 65]
    one = np.zeros(shape, bool)
    one[2, 3, 64] = True
    lab, stats = label_call(dev, one, 3)
    idx = (2 * 5 + 3) * 66 + 64
    assert lab.ravel()[idx] == 1 and lab.sum() == 1 and list(stats[0][:17]) == [1, 1, 1, 1, idx, 2, 3, 64, 2, 3, 64, 2, 3, 64, 2, 3, 64]
    assert np.array_equal(PP().foreground_bbox(up(one, dev)).cpu().numpy(), [2, 3, 64, 2, 3, 64])


def test_tie_goes_to_the_first_component_in_raster_order(dev):
    mask = mask_of("tie")
    want_lab, want_stats = ref_labels("tie", 1)
    lab, stats = label_call(dev, mask)
    assert np.array_equal(lab, want_lab) and np.array_equal(stats, want_stats)
    assert list(stats[0][:5]) == [2, 4, 2, 1, (0 * 4 + 1) * 10 + 3]
    assert np.array_equal(PP().keep_largest_component(up(mask, dev)).cpu().numpy().astype(bool), want_lab == 1)


@pytest.mark.parametrize("name", ["slab", "batch"])
def test_two_calls_agree_bit_for_bit(dev, name):
    a = label_call(dev, mask_of(name), 1)
    b = label_call(dev, mask_of(name), 1)
    assert a[0].tobytes() == b[0].tobytes() and a[1].tobytes() == b[1].tobytes()


def test_component_error_codes(dev):
    from pytorchdeeplearing_amd import _capi
    lib = _capi.lib_for(dev)
    m = up(mask_of("tiny"), dev)
    ws = torch.empty(int(lib.seg_cc_ws_bytes(1, 5, 7, 9)) + 256, dtype=torch.uint8, device=dev)
    lab = torch.full((5, 7, 9), -7, dtype=torch.int32, device=dev)
    stats = torch.full((32,), -7, dtype=torch.int32, device=dev)
    st = _capi.stream_for(dev)
    ok = (m.data_ptr(), 1, 5, 7, 9, -1, 1, ws.data_ptr(), lab.data_ptr(), stats.data_ptr())
    bad = {"connectivity 2": {6: 2}, "null mask": {0: None}, "null ws": {7: None}, "null stats": {9: None}, "d = 0": {2: 0}, "w = 2049": {4: 2049},
           "n = 0": {1: 0}, "cls 256": {5: 256}}
    for what, change in bad.items():
        args = list(ok)
        for k, v in change.items():
            args[k] = v
        assert lib.seg_cc_label(*args, st) != 0 and b"seg_cc_label" in lib.seg_last_error(), what
    assert lib.seg_cc_filter(m.data_ptr(), m.data_ptr(), 1, 5, 7, 9, -1, 2, 0, 0, ws.data_ptr(), None, st) != 0
    assert lib.seg_cc_filter(m.data_ptr(), None, 1, 5, 7, 9, -1, 1, 0, 0, ws.data_ptr(), None, st) != 0
    assert lib.seg_cc_filter(m.data_ptr(), m.data_ptr(), 1, 5, 7, 9, -1, 1, 7, 0, ws.data_ptr(), None, st) != 0
    assert lib.seg_cc_ws_bytes(1, 0, 7, 9) < 0 and lib.seg_cc_ws_bytes(2, 2048, 2048, 512) < 0
    assert (lab.cpu().numpy() == -7).all() and (stats.cpu().numpy() == -7).all()          # nothing was launched
    with pytest.raises(RuntimeError):
        PP().connected_components(m, connectivity=2)
    with pytest.raises(RuntimeError):                                                     # CPU tensors raise outside the checker
        getattr(_capi, "product_lib_for", _capi.lib_for)(torch.device("cpu"))


# ---- morphology ----------------------------------------------------------------------------------------------------------------------------------------

def morph_call(dev, mask, op, shape, radii, border, **kw):
    return PP().binary_morphology(up(mask, dev), op, radii, shape=shape, border=border, **kw).cpu().numpy()


def check_morph(dev, case, op, shape, radii, border):
    mask = mask_of(case)
    got = morph_call(dev, mask, op, shape, radii, border)
    assert got.dtype == np.uint8 and got.shape == mask.shape and got.max() <= 1
    sha, count = gold()["morph"][mk.morph_key(case, op, shape, radii, border)]
    where = (case, op, shape, radii, border)
    if HAVE_SCIPY:
        want = mk.morph_ref(mask, op, mk.structure(shape, radii)[0], border)
        assert np.array_equal(got.astype(bool), want), (where, int(got.sum()), int(want.sum()), np.argwhere(got.astype(bool) != want)[:5])
    assert int(got.sum()) == count, where
    assert hashlib.sha256(np.packbits(got.astype(bool)).tobytes()).hexdigest() == sha, where


@pytest.mark.parametrize("se", mk.MORPH_SES, ids=["%s%d%d%d" % ((s,) + r) for s, r in mk.MORPH_SES])
@pytest.mark.parametrize("case", mk.MORPH_CASES)
def test_dilate_and_erode_equal_scipy(dev, case, se):
    for op in ("dilate", "erode"):
        for border in (0, 1):
            check_morph(dev, case, op, se[0], se[1], border)


@pytest.mark.parametrize("case", mk.MORPH_CASES)
def test_open_and_close_equal_scipy(dev, case):
    for op in ("open", "close"):
        for r in (1, 2):
            check_morph(dev, case, op, "ball", (r, r, r), None)


@pytest.mark.parametrize("case", ["carry64", "carry65"])
def test_carries_across_words_and_the_padding_bits(dev, case):
    """voxels at x = 0, 63 and 64 only, widened by 31: the carries between the words, and (border 1 against border 0) the padding bits of the last word,
    which must read as the border and never leak into the volume"""
    for shape, radii in mk.CARRY_SES:
        for op in ("dilate", "erode"):
            for border in (0, 1):
                check_morph(dev, case, op, shape, radii, border)
    mask = mask_of(case)
    w = mask.shape[2]
    got = morph_call(dev, mask, "dilate", "box", (0, 0, 31), 0).astype(bool)
    want = np.zeros(w, bool)
    for x in (0, 63, 64):
        if x < w:
            want[max(0, x - 31):x + 32] = True
    assert np.array_equal(got, np.broadcast_to(want, mask.shape))


def test_morphology_values_defaults_in_place_and_errors(dev):
    mask = mask_of("slab")
    base = morph_call(dev, mask, "dilate", "ball", 1, 0)
    assert np.array_equal(morph_call(dev, mask, "dilate", "ball", (1, 1, 1), None), base)                 # default border of a dilation: 0
    assert np.array_equal(morph_call(dev, mask, "erode", "ball", 1, None), morph_call(dev, mask, "erode", "ball", 1, 1))
    assert np.array_equal(morph_call(dev, mask, "dilate", "ball", 1, 0, fg_value=255), base * 255)
    vol = np.where(mask, 2, 1).astype(np.uint8)
    assert np.array_equal(PP().binary_morphology(up(vol, dev), "dilate", 1, border=0, cls=2).cpu().numpy(), base)
    t = up(mask, dev)
    assert PP().binary_morphology(t, "dilate", 1, border=0, out=t) is t and np.array_equal(t.cpu().numpy(), base)
    assert np.array_equal(morph_call(dev, mask, "dilate", "ball", 0, 0), mask)                            # a single voxel: the identity
    with pytest.raises(RuntimeError, match="radii"):
        morph_call(dev, mask, "dilate", "ball", 32, 0)
    with pytest.raises(RuntimeError, match="border"):
        morph_call(dev, mask, "open", "ball", 1, 0)
    with pytest.raises(ValueError):
        morph_call(dev, mask, "thicken", "ball", 1, 0)
    with pytest.raises(TypeError):
        PP().binary_morphology(torch.zeros((3, 4, 5), dtype=torch.float32, device=dev), "dilate", 1)
    from pytorchdeeplearing_amd import _capi
    lib = _capi.lib_for(dev)
    assert lib.seg_morph3d_ws_bytes(1, 3, 0, 5) < 0
    assert lib.seg_morph3d(None, t.data_ptr(), 1, 3, 130, 67, -1, 0, 0, 1, 1, 1, -1, 1, t.data_ptr(), _capi.stream_for(dev)) != 0


# ---- the reference's helper names (dataprocess/utils.py) -----------------------------------------------------------------------------------------------

@pytest.fixture
def utils(dev, monkeypatch):
    from dataprocess import utils as U
    monkeypatch.setattr(U, "MASK_DEVICE", dev)
    return U


@pytest.mark.skipif(not HAVE_SCIPY, reason="restated with scipy")
def test_reference_helpers_on_numpy_arrays(dev, utils):
    from scipy import ndimage
    mask = mask_of("noise")
    image = np.where(mask, 7, 0).astype(np.int16)
    # GetLargestConnectedCompont: ConnectedComponent (faces) + the first largest label -> 0 / 1
    lab, k = ndimage.label(image != 0)
    sizes = np.bincount(lab.ravel())[1:]
    got = utils.GetLargestConnectedCompont(image)
    assert isinstance(got, np.ndarray) and got.shape == image.shape
    assert np.array_equal(got, (lab == 1 + int(np.argmax(sizes))).astype(np.uint8))
    # MorphologicalOperation: ball of radius k on every axis, erosion with the border as foreground
    for name in ("open", "close", "dilate", "erode"):
        want = mk.morph_ref(image != 0, name, mk.structure("ball", (2, 2, 2))[0])
        assert np.array_equal(utils.MorphologicalOperation(image, 2, name), want.astype(np.uint8)), name
    assert utils.MorphologicalOperation(image, 2, "skeleton") is None
    plane = mask_of("plane")[0]                                            # a 2-D image: the ball is a disc
    want = ndimage.binary_dilation(plane, structure=mk.structure("ball", (0, 2, 2))[0][0])
    assert np.array_equal(utils.MorphologicalOperation(plane.astype(np.uint8), 2, "dilate"), want.astype(np.uint8))
    # a device tensor comes back as a device tensor
    t = utils.GetLargestConnectedCompont(up(image != 0, dev))
    assert torch.is_tensor(t) and t.device.type == dev.type and np.array_equal(t.cpu().numpy(), got)
    # getRangImageRange
    vol = np.zeros((6, 7, 8), np.float32)
    assert all(utils.getRangImageRange(vol, i) == (0, 0) for i in range(3))
    vol[2:5, 1:3, 6] = 3.0
    assert [utils.getRangImageRange(vol, i) for i in range(3)] == [(2, 4), (1, 2), (6, 6)]
    assert utils.getRangImageRange(torch.from_numpy(vol), 0) == (2, 4)


def test_bounding_box_is_the_box_of_all_voxels_equal_to_one(dev, utils):
    """utils.py:13-15 runs LabelShapeStatistics on the binary image and asks for label 1: all voxels equal to 1, not the largest component"""
    vol = np.zeros((8, 9, 70), np.uint8)
    vol[1:4, 2:6, 3:30] = 1                      # the largest component
    vol[6, 7, 66:69] = 1                         # a speck far away: it widens the box
    vol[0, 0, 0] = 2                             # another value: no part of label 1
    box = utils.GetLargestConnectedCompontBoundingbox(vol)
    assert list(box) == [3, 2, 1, 66, 6, 6]      # [xstart, ystart, zstart, xsize, ysize, zsize]
    _, stats = label_call(dev, vol, 1, cls=1)
    assert list(stats[0][5:11]) == [1, 2, 3, 3, 5, 29] and list(stats[0][11:17]) == [1, 2, 3, 6, 7, 68]


# ---- the model wrappers' postprocess hook ----------------------------------------------------------------------------------------------------------------

@pytest.mark.skipif(not HAVE_SCIPY, reason="the cleaned mask is restated with scipy")
def test_wrapper_postprocess_hook(dev, monkeypatch):
    """postprocess = None: inference / inference_patch return what they return with the attribute unset; with keep_largest_component the result is the same
    mask cleaned by scipy"""
    conftest.checker_slow(dev, "UNet3d inference chains take ~40 s on the host checker")
    import model
    from scipy import ndimage
    from oracle import seg_oracle as seg
    monkeypatch.setenv("SEGENGINE_DTYPE", "f32")
    m = model.BinaryUNet3dModel(image_depth=16, image_height=16, image_width=16, image_channel=1, numclass=1, batch_size=3, use_cuda=dev.type == "cuda")
    m.model.load_state_dict(seg.perturb_params(seg.init_params("unet", 3, 1, 1, seed=0), seed=7))
    rs = np.random.RandomState(11)
    arr = (rs.randn(20, 22, 24) * 100.0).astype(np.float32)
    arr[:, :5] = 0.0
    ct = (-1024.0 + 224.0 * rs.rand(20, 24, 28)).astype(np.float32)
    assert type(m).postprocess is None and "postprocess" not in vars(m)
    plain = m.inference(arr, newSize=(16, 16, 16))
    plain_patch = m.inference_patch(ct, newSpacing=(0.8, 0.8, 0.8), spacing=(1.0, 1.0, 1.0))
    m.postprocess = None
    assert np.array_equal(m.inference(arr, newSize=(16, 16, 16)), plain)
    m.postprocess = functools.partial(PP().keep_largest_component)
    for got, base in ((m.inference(arr, newSize=(16, 16, 16)), plain),
                      (m.inference_patch(ct, newSpacing=(0.8, 0.8, 0.8), spacing=(1.0, 1.0, 1.0)), plain_patch)):
        lab, k = ndimage.label(base != 0)
        assert k > 1 and got.dtype == base.dtype                     # the hook has something to remove
        assert np.array_equal(got, np.where(lab == 1 + int(np.argmax(np.bincount(lab.ravel())[1:])), base, 0))
    m.postprocess = lambda t: t.float()
    with pytest.raises(TypeError):
        m.inference(arr, newSize=(16, 16, 16))
