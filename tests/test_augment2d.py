"""seg_augment2d (csrc/augment2d.hip) and its host side (pytorchdeeplearing_amd/augment2d.py) against tests/aug2d_oracle.py, the float64 restatement of
the contract in include/segengine.h.  The contract is this project's own definition, not albumentations / cv2 (neither can run here).

Every shape case runs SUITE - six parameter blocks, one sample each, in ONE launch: flipped copy, median, box blur, warp + tone, motion blur + warp,
median + warp - so every branch of the kernel meets every shape.
  tiny_5x7        c = 1: below a wave, w no multiple of the store width
  chlast_9x70x3   channel-last, three channels, w above 64 and no multiple of 4
  rows_130x67     many rows, several workgroups; uint8 label
  line_1x33, col_33x1   the mirror (and the median's clamp) on an axis of one pixel
  far             scale 0.05 + a shift of several image sizes: the mirror folds over many periods; all three border modes; int64 label with
                  label_cval -3 and uint8 label with 0 under mode constant
  ties_8x12       scale exactly 0.5, no rotation: coordinates land on x.5 - the label follows floor(c + 0.5), not round-half-even
  mixed_batch     blur {none, box 3, median, motion 7} x warp {off, on} in one launch = the eight single launches, bit for bit

Tolerances.  Labels: equal.  Images on the copy-only path (blur none or median, no warp, alpha 1, beta 0, no clip): equal.  Images on the arithmetic
paths: |out - oracle| <= 80 * 2^-24 * (max|x| + |beta|) - derived, not measured: a value passes at most 49 f32 accumulations with non-negative weights
summing to 1, three interpolations and one multiply-add with |alpha| <= 1.3; a wrong tap or fold is an O(1) error on the random inputs.
The oracle's decision margin (no floor of a coordinate within 1e-9 of an integer unless the coordinate is exact) is asserted for every compared
sample, so a tap does not hang on the last bit of a double."""
import numpy as np
import pytest
import torch

import aug2d_oracle as oracle

TOL = 80 * 2.0 ** -24
BORDER = {"nearest": oracle.NEAREST, "constant": oracle.CONSTANT, "mirror": oracle.MIRROR}


def a2():
    from pytorchdeeplearing_amd import augment2d
    return augment2d


def suite(h, w, angle=17.0):
    m = a2()
    return [m.make_params2d(hflip=True),
            m.make_params2d(hflip=True, vflip=True, blur=2),
            m.make_params2d(vflip=True, blur=1, kernel=np.full((3, 3), 1 / 9)),
            m.make_params2d(m.affine_matrix2d(angle, 1.1, 0.04 * w, -0.05 * h, (h, w)), alpha=1.2, beta=0.1),
            m.make_params2d(m.affine_matrix2d(-2 * angle + 1, 0.85, -0.03 * w, 0.02 * h, (h, w)), vflip=True, blur=1,
                            kernel=m.motion_kernel(5, (0, 1), (4, 2))),
            m.make_params2d(m.affine_matrix2d(angle / 3, 1.0, 0.3, 0.7, (h, w)), hflip=True, blur=2, alpha=0.8, beta=-0.2)]


def is_copy(p):
    return p[7] == 0 and p[8] in (0, 2) and p[10] == 1 and p[11] == 0 and p[12] == 0


def launch(dev, x, params, label=None, layout="th", border="mirror", cval=0.0, label_cval=0):
    """x numpy in `layout`, label numpy (N, H, W) or None -> numpy results of one launch"""
    out, lab = a2().transform_batch2d(torch.from_numpy(x).to(dev), np.stack(params), None if label is None else torch.from_numpy(label).to(dev),
                                      layout, border, cval, label_cval)
    return out.cpu().numpy(), None if lab is None else lab.cpu().numpy()


def check(name, x_th, params, out_th, label=None, label_out=None, border="mirror", cval=0.0, label_cval=0):
    """every sample of a launch against the oracle; x_th / out_th are (N, C, H, W) (x_th may hold one source for all)"""
    for s, p in enumerate(params):
        src = x_th[s if len(x_th) > 1 else 0]
        lsrc = None if label is None else label[s if len(label) > 1 else 0]
        want, lwant, margin = oracle.apply(src, p, lsrc, BORDER[border], cval, label_cval)
        err = float(np.abs(out_th[s] - want).max())
        bound = TOL * (float(np.abs(src).max()) + abs(p[11]))
        print(name, "sample", s, "margin", margin, "max err", err, "bound", bound)
        assert margin >= 1e-9
        if is_copy(p):
            assert np.array_equal(out_th[s], want.astype(np.float32))
        else:
            assert err <= bound
        if label is not None:
            assert label_out[s].dtype == label.dtype and np.array_equal(label_out[s], lwant)


SHAPES = {"tiny_5x7": (1, 5, 7, "th", None), "chlast_9x70x3": (3, 9, 70, "tf", np.float32), "rows_130x67": (1, 130, 67, "th", np.uint8),
          "line_1x33": (2, 1, 33, "th", np.int64), "col_33x1": (1, 33, 1, "th", np.uint8)}


@pytest.mark.parametrize("name", list(SHAPES))
def test_every_branch_on_every_shape(dev, name):
    c, h, w, layout, ldt = SHAPES[name]
    rng = np.random.default_rng(len(name) * 7 + h)
    params = suite(h, w)
    n = len(params)
    x = (rng.standard_normal((n, c, h, w)) * 2).astype(np.float32)
    label = None if ldt is None else rng.integers(0, 5, size=(n, h, w)).astype(ldt)
    xin = np.ascontiguousarray(x.transpose(0, 2, 3, 1)) if layout == "tf" else x
    out, lab = launch(dev, xin, params, label, layout)
    assert out.shape == xin.shape and out.dtype == np.float32
    check(name, x, params, out.transpose(0, 3, 1, 2) if layout == "tf" else out, label, lab)


@pytest.mark.parametrize("border", ["mirror", "nearest", "constant"])
def test_far_outside_folds_over_many_periods(dev, border):
    m = a2()
    h, w = 11, 14
    rng = np.random.default_rng(4)
    params = [m.make_params2d(m.affine_matrix2d(7.0, 0.05, 3.3 * w, -2.6 * h, (h, w))),
              m.make_params2d(m.affine_matrix2d(-11.0, 0.05, -4.2 * w, 5.1 * h, (h, w)), hflip=True, blur=1, kernel=np.full((3, 3), 1 / 9))]
    x = rng.standard_normal((2, 2, h, w)).astype(np.float32)
    for ldt, lcval in ((np.int64, -3), (np.uint8, 0)):
        label = rng.integers(1, 200, size=(2, h, w)).astype(ldt)
        out, lab = launch(dev, x, params, label, "th", border, -0.5, lcval)
        check("far/" + border, x, params, out, label, lab, border, -0.5, lcval)
        if border == "constant":
            assert (lab == lcval).any() and (np.abs(out + 0.5) <= TOL).any()
    # the coordinates really leave the image by many periods
    sy = 10 * params[0][0] + 13 * params[0][1] + params[0][2]
    assert abs(sy) > 20 * h


def test_ties_follow_floor_of_c_plus_half(dev):
    m = a2()
    h, w = 8, 12
    mat = m.affine_matrix2d(0.0, 0.5, 0.0, 0.0, (h, w))
    assert np.array_equal(mat, [[2.0, 0.0, -3.5], [0.0, 2.0, -5.5]])                 # every coordinate is x.5, exactly
    rng = np.random.default_rng(8)
    x = rng.standard_normal((1, 1, h, w)).astype(np.float32)
    label = rng.integers(0, 250, size=(1, h, w)).astype(np.uint8)
    for border in ("mirror", "nearest", "constant"):
        out, lab = launch(dev, x, [m.make_params2d(mat)], label, "th", border, 0.25, 9)
        check("ties/" + border, x, [m.make_params2d(mat)], out, label, lab, border, 0.25, 9)
    # written out for one pixel: output (4, 6) reads coordinate (4.5, 6.5) -> label pixel (5, 7) (round-half-even would take (4, 6))
    out, lab = launch(dev, x, [m.make_params2d(mat)], label, "th", "nearest")
    assert lab[0, 4, 6] == label[0, 5, 7]
    assert abs(out[0, 0, 4, 6] - x[0, 0, 4:6, 6:8].astype(np.float64).mean()) <= TOL * np.abs(x).max()


def mixed_params(h, w):
    m = a2()
    blurs = [dict(), dict(blur=1, kernel=np.full((3, 3), 1 / 9)), dict(blur=2), dict(blur=1, kernel=m.motion_kernel(7, (1, 0), (6, 6)))]          # (its last weight is the one that lives in slot 15)
    params = []
    for i, b in enumerate(blurs):
        for warp in (False, True):
            mat = m.affine_matrix2d(9.0 + 13 * i, 0.9 + 0.07 * i, 0.5 + i, -1.25 * i, (h, w)) if warp else None
            params.append(m.make_params2d(mat, hflip=bool(i & 1), vflip=bool((i >> 1) ^ warp), **b))
    return params


def test_mixed_batch_equals_the_single_launches(dev):
    h, w = 19, 37
    params = mixed_params(h, w)
    assert len(params) == 8 and len({(p[6], p[7], p[8], p[9]) for p in params}) == 8
    rng = np.random.default_rng(12)
    x = rng.standard_normal((8, 2, h, w)).astype(np.float32)
    label = rng.integers(0, 255, size=(8, h, w)).astype(np.uint8)
    out, lab = launch(dev, x, params, label)
    for s in range(8):
        o1, l1 = launch(dev, x[s:s + 1], params[s:s + 1], label[s:s + 1])
        assert np.array_equal(o1[0], out[s]) and np.array_equal(l1[0], lab[s])
    check("mixed_batch", x, params, out, label, lab)


def test_one_source_for_all_samples(dev):
    h, w = 10, 13
    params = mixed_params(h, w)[2:6]
    rng = np.random.default_rng(13)
    x = rng.standard_normal((1, 3, h, w)).astype(np.float32)
    label = rng.integers(0, 9, size=(1, h, w)).astype(np.int64)
    out, lab = launch(dev, x, params, label)                                          # xs_n == 0
    assert out.shape == (4, 3, h, w) and lab.shape == (4, h, w)
    out4, lab4 = launch(dev, np.repeat(x, 4, axis=0), params, np.repeat(label, 4, axis=0))
    assert np.array_equal(out, out4) and np.array_equal(lab, lab4)
    check("xs_n=0", x, params, out, label, lab)
    xl = np.ascontiguousarray(x.transpose(0, 2, 3, 1))
    outl, labl = launch(dev, xl, params, label, "tf")
    assert np.array_equal(outl.transpose(0, 3, 1, 2), out) and np.array_equal(labl, lab)


def test_clip_with_both_bounds_active(dev):
    m = a2()
    h, w = 6, 21
    rng = np.random.default_rng(14)
    x = rng.standard_normal((2, 1, h, w)).astype(np.float32)
    params = [m.make_params2d(alpha=1.3, beta=0.05, clip=(-0.4, 0.6)),
              m.make_params2d(m.affine_matrix2d(21.0, 1.15, 1.3, -0.45, (h, w)), blur=1, kernel=np.full((3, 3), 1 / 9), clip=(-0.1, 0.2))]
    out, _ = launch(dev, x, params)
    check("clip", x, params, out)
    for s, (lo, hi) in enumerate(((-0.4, 0.6), (-0.1, 0.2))):
        assert out[s].min() == np.float32(lo) and out[s].max() == np.float32(hi) and ((out[s] > lo) & (out[s] < hi)).any()


# ---- the draw ---------------------------------------------------------------------------------------------------------------------------------------
def test_a_draw_consumes_sixteen_values():
    m = a2()
    for seed, kw in ((1, {}), (2, dict(blur_p=1.0, affine_p=1.0, brightness_contrast_p=1.0)), (3, dict(hflip_p=0, vflip_p=0, blur_p=0, affine_p=0))):
        np.random.seed(seed)
        stream = [np.random.random() for _ in range(17)]
        np.random.seed(seed)
        p = m.draw_transform2d(m.Segmenation_Aug(**kw), (24, 40))
        assert np.random.random() == stream[16]
        assert p.shape == (m.PARAM_DOUBLES,) and p.dtype == np.float64 and m.Segmenation_Aug.PARAM_DOUBLES == 64 == m.DRAWS_PER_SAMPLE * 4
        np.random.seed(seed)
        assert np.array_equal(p, m.draw_transform2d(m.Segmenation_Aug(**kw), (24, 40)))          # a seeded run is reproducible


def connected(ker):
    pts = [tuple(v) for v in np.argwhere(ker > 0)]
    seen, todo = {pts[0]}, [pts[0]]
    while todo:
        y, x = todo.pop()
        for q in pts:
            if q not in seen and abs(q[0] - y) <= 1 and abs(q[1] - x) <= 1:
                seen.add(q)
                todo.append(q)
    return len(seen) == len(pts)


def test_motion_kernels_are_connected_lines():
    m = a2()
    for k in (3, 5, 7):
        for x0 in range(k):
            for y0 in range(k):
                for x1 in range(k):
                    for y1 in range(k):
                        ker = m.motion_kernel(k, (x0, y0), (x1, y1))
                        assert ker.shape == (k, k) and ker.min() >= 0 and abs(ker.sum() - 1) <= 1e-12 and connected(ker)
                        assert (ker > 0).sum() >= 2
                        if (x0, y0) != (x1, y1):
                            assert ker[y0, x0] > 0 and ker[y1, x1] > 0 and (ker > 0).sum() == max(abs(x1 - x0), abs(y1 - y0)) + 1
                        else:
                            assert ker[y0, x0] > 0 or (x0, y0) == (k // 2, k // 2)
    # the kernels a generator draws
    np.random.seed(5)
    gen = m.Segmenation_Aug(blur_p=1.0, motion_weight=1.0, median_weight=0.0, box_weight=0.0)
    ks = set()
    for _ in range(200):
        p = m.draw_transform2d(gen, (16, 16))
        k = int(p[9])
        slots = np.append(p[16:64], p[15])                 # (weight 48 of a 7 x 7 kernel lives in slot 15)
        ker = slots[:k * k].reshape(k, k)
        ks.add(k)
        assert p[8] == 1 and ker.min() >= 0 and abs(ker.sum() - 1) <= 1e-12 and connected(ker) and not slots[k * k:].any()
    assert ks == {3, 5, 7}


def test_step_frequencies_over_4000_draws():
    m = a2()
    gen = m.Segmenation_Aug()
    np.random.seed(11)
    n = 4000
    blocks = np.stack([m.draw_transform2d(gen, (32, 48)) for _ in range(n)])
    motion = (blocks[:, 8] == 1) & ((blocks[:, 16:25] != 1 / 9).any(axis=1) | (blocks[:, 9] != 3))
    box = (blocks[:, 8] == 1) & ~motion
    seen = {"hflip": ((blocks[:, 6].astype(int) & 1) != 0, 0.5), "vflip": ((blocks[:, 6].astype(int) & 2) != 0, 0.5),
            "blur": (blocks[:, 8] != 0, 0.2), "motion": (motion, 0.1), "median": (blocks[:, 8] == 2, 0.05), "box": (box, 0.05),
            "affine": (blocks[:, 7] != 0, 0.2), "tone": ((blocks[:, 10] != 1) | (blocks[:, 11] != 0), 0.2)}
    for name, (hit, prob) in seen.items():
        sd = np.sqrt(prob * (1 - prob) / n)
        print(name, hit.mean(), "expected", prob, "+-", 4 * sd)
        assert abs(hit.mean() - prob) <= 4 * sd
    warped = blocks[blocks[:, 7] != 0]
    scale = 1 / np.hypot(warped[:, 0], warped[:, 1])
    assert scale.min() >= 0.8 - 1e-12 and scale.max() <= 1.2 + 1e-12
    assert np.abs(np.degrees(np.arctan2(warped[:, 3], warped[:, 0]))).max() <= 45 + 1e-9
    toned = blocks[blocks[:, 10] != 1]
    assert np.abs(toned[:, 10] - 1).max() <= 0.3 and np.abs(toned[:, 11]).max() <= 0.3 and not blocks[:, 12].any()
    assert m.draw_transform2d(m.Segmenation_Aug(brightness_contrast_p=1.0, brightness_scale=255, clip=(0, 255)), (8, 8))[12:15].tolist() == [1, 0, 255]


def test_the_matrix_inverts_shift_rotate_scale_about_the_centre():
    m = a2()
    h, w = 24, 40
    mat = m.affine_matrix2d(30.0, 1.25, 3.0, -2.0, (h, w))
    cx, cy = (w - 1) / 2, (h - 1) / 2
    a = np.radians(30.0)
    for x, y in ((0.0, 0.0), (7.0, 19.0), (cx, cy)):
        fx = 1.25 * (np.cos(a) * (x - cx) - np.sin(a) * (y - cy)) + cx + 3.0            # forward: where source (x, y) lands
        fy = 1.25 * (np.sin(a) * (x - cx) + np.cos(a) * (y - cy)) + cy - 2.0
        sy, sx = mat @ np.array([fy, fx, 1.0])
        assert abs(sy - y) <= 1e-9 and abs(sx - x) <= 1e-9


# ---- refusals -----------------------------------------------------------------------------------------------------------------------------------------
def test_every_refusal_launches_nothing(dev):
    from pytorchdeeplearing_amd import _capi
    m = a2()
    lib = _capi.lib_for(dev)
    h, w = 5, 7
    x = torch.from_numpy(np.random.default_rng(0).standard_normal((1, 1, h, w)).astype(np.float32)).to(dev)
    out = torch.full_like(x, -7.0)
    lab = torch.ones((1, h, w), dtype=torch.uint8, device=dev)
    lab_out = torch.full_like(lab, 7)
    lab64, lab64_out = lab.to(torch.int64), torch.full((1, h, w), 7, dtype=torch.int64, device=dev)
    good = m.pack_params2d([m.make_params2d(m.affine_matrix2d(10.0, 1.0, 0.0, 0.0, (h, w)), blur=1, kernel=np.full((3, 3), 1 / 9))])
    pd = torch.from_numpy(good).to(dev)
    st = _capi.stream_for(dev)
    assert lib.seg_augment2d_ws_bytes(1) >= 0 and lib.seg_augment2d_ws_bytes(0) < 0 and lib.seg_augment2d_ws_bytes(65536) < 0

    def call(params=good, n=1, c=1, ext=(h, w), mode=4, cval=0.0, lcval=0.0, xp=x.data_ptr(), op=out.data_ptr(), pdp=pd.data_ptr(), label=(None, None, 0),
             host=True, strides=None):
        xs_n, xs_c, xs_v = strides if strides else (c * ext[0] * ext[1], ext[0] * ext[1], 1)
        return lib.seg_augment2d(xp, op, n, c, ext[0], ext[1], xs_n, xs_c, xs_v, label[0], label[1], label[2], params.ctypes.data if host else None,
                                 pdp, mode, cval, lcval, None, st)

    def bad(slot, value):
        p = good.copy()
        p[0, slot] = value
        return p
    refused = [call(xp=None), call(op=None), call(pdp=None), call(host=False), call(op=x.data_ptr()),                     # null pointers, out == x
               call(label=(lab.data_ptr(), None, 0)), call(label=(lab.data_ptr(), lab.data_ptr(), 0)),
               call(n=0), call(n=65536), call(c=0), call(ext=(0, w)), call(ext=(h, 0)), call(ext=(65536, 32769)),            # n, extents, h*w > 2^31
               call(bad(0, np.nan)), call(bad(5, np.inf)), call(bad(10, np.nan)), call(bad(11, -np.inf)), call(cval=np.nan),  # non-finite
               call(bad(9, 4.0)), call(bad(9, 9.0)), call(bad(9, 0.0)), call(bad(8, 3.0)),                                   # k, blur
               call(bad(6, 4.0)), call(bad(6, -1.0)), call(bad(6, 1.5)),                                                     # flips
               call(mode=2), call(mode=3), call(mode=5),                                                                     # border modes
               call(mode=1, lcval=-3.0, label=(lab.data_ptr(), lab_out.data_ptr(), 0)),                                      # label_cval a uint8 cannot hold
               call(mode=1, lcval=256.0, label=(lab.data_ptr(), lab_out.data_ptr(), 0)),
               call(mode=1, lcval=0.5, label=(lab64.data_ptr(), lab64_out.data_ptr(), 2)),
               call(label=(lab.data_ptr(), lab_out.data_ptr(), 1)),                                                          # label type
               call(strides=(h * w, h * w, 2)), call(strides=(3, h * w, 1))]
    assert all(rc < 0 for rc in refused), refused
    assert b"seg_augment2d" in lib.seg_last_error()
    assert np.all(out.cpu().numpy() == -7.0) and np.all(lab_out.cpu().numpy() == 7) and np.all(lab64_out.cpu().numpy() == 7)
    # the same call without a defect runs
    assert call(mode=1, lcval=-3.0, label=(lab64.data_ptr(), lab64_out.data_ptr(), 2)) == 0
    want, _, _ = oracle.apply(x.cpu().numpy()[0], good[0], None, oracle.CONSTANT)
    assert np.abs(out.cpu().numpy()[0] - want).max() <= TOL * float(x.abs().max())
    # the python layer
    with pytest.raises(NotImplementedError, match="'mirror', 'nearest' and 'constant'"):
        m.Segmenation_Aug(border_mode="reflect")
    with pytest.raises(ValueError):
        m.Segmenation_Aug(border_mode="zigzag")
    with pytest.raises(TypeError):
        m.transform_batch2d(x.double(), good)
    with pytest.raises(ValueError):
        m.transform_batch2d(x[0], good)
    with pytest.raises(ValueError):
        m.make_params2d(blur=1, kernel=np.ones((4, 4)))
