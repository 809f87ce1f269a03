"""Sliding-window inference with blended probabilities (pytorchdeeplearing_amd/prepost.py over csrc/sliding.hip): window lists, the gather /
blend / finalize kernels and `sliding_window_predict` against a plain fp64 numpy restatement written here (entry list -> mirrored, padded
windows -> weighted accumulation -> division -> threshold / arg-max).  Every device case runs on the host-side execution-model checker
('emu') and, under -m gpu, on the real library.

Tolerances.  A blended probability is the fp32 quotient of two sums of at most 64 positive terms (8 overlapping windows x 8 mirror
entries): relative error <= about (64 + 2) * 2^-24 = 4e-6 on values in [0, 1], so 1e-5 absolute.  A mask voxel is compared only where the
restatement's decision margin (|p - 0.5| for one class, the gap between the two largest classes otherwise) is at least 2e-5, twice that;
the voxels left out must stay below 0.1 % of the volume (on the restatement alone, uniform random window probabilities put 1-3 of 13 320
voxels inside the margin at the largest shape and none at the two small ones)."""
import functools
import itertools
import zlib

import numpy as np
import pytest
import torch

from pytorchdeeplearing_amd import prepost as pp

PROB_TOL, MARGIN, MAX_LEFT_OUT = 1e-5, 2e-5, 1e-3

# volume, patch: odd W (scalar tail, unaligned rows) / 2-D / volume smaller than the patch on z
SHAPES = [((20, 18, 37), (8, 8, 16)), ((1, 24, 40), (1, 16, 16)), ((5, 18, 16), (8, 8, 16))]
# beyond those three: W % 4 == 0, so rows are walked in 16-byte quads, with window origins that are no multiple of 4 (quads cut by a window
# edge next to quads read with one wide load; pw % 4 == 0 and pw % 4 != 0)
QUAD_SHAPES = [((6, 10, 40), (4, 8, 20)), ((3, 9, 40), (2, 4, 18))]
ORIGIN_SHAPES = [((16, 16, 16), (16, 16, 16)), ((40, 16, 24), (16, 16, 16)), ((8, 20, 16), (16, 16, 16)), ((20, 18, 37), (8, 8, 16))]


def _t(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


# ------------------------------------------------------------------------------------------------ the fp64 restatement
def ref_window(vol, entry, patch, pad_value=0.0):
    """what the network sees for one entry: the crop at the origin, `pad_value` outside the volume, then mirrored"""
    z, y, x, f = entry
    win = np.full(patch, pad_value, vol.dtype)
    n = [max(0, min(p, s - o)) for p, s, o in zip(patch, vol.shape, (z, y, x))]
    win[:n[0], :n[1], :n[2]] = vol[z:z + n[0], y:y + n[1], x:x + n[2]]
    for a in range(3):
        if f >> a & 1:
            win = np.flip(win, a)
    return win


def ref_blend(vol_shape, patch, entries, probs, weights):
    """entries + per-entry probabilities (nb, C, pd, ph, pw) -> (acc, wsum) in fp64"""
    c = probs.shape[1]
    acc, wsum = np.zeros((c,) + tuple(vol_shape)), np.zeros(tuple(vol_shape))
    wz, wy, wx = (np.asarray(w, np.float64) for w in weights)
    w3 = wz[:, None, None] * wy[None, :, None] * wx[None, None, :]
    for (z, y, x, f), p in zip(entries, probs.astype(np.float64)):
        for a in range(3):
            if f >> a & 1:
                p = np.flip(p, 1 + a)              # back into the volume's orientation
        n = [max(0, min(q, s - o)) for q, s, o in zip(patch, vol_shape, (z, y, x))]
        acc[:, z:z + n[0], y:y + n[1], x:x + n[2]] += w3[:n[0], :n[1], :n[2]] * p[:, :n[0], :n[1], :n[2]]
        wsum[z:z + n[0], y:y + n[1], x:x + n[2]] += w3[:n[0], :n[1], :n[2]]
    return acc, wsum


def ref_finalize(acc, wsum, threshold=0.5, scale=1):
    """-> (probabilities, mask, decision margin)"""
    with np.errstate(invalid="ignore", divide="ignore"):
        p = np.where(wsum > 0, acc / wsum, 0.0)
    if acc.shape[0] == 1:
        mask, margin = (p[0] > threshold) * scale, np.abs(p[0] - threshold)
    else:
        top = np.sort(p, 0)
        mask, margin = np.argmax(p, 0), top[-1] - top[-2]
    mask = np.where(wsum > 0, mask, 0).astype(np.uint8)
    return p, mask, margin


def check_mask(got, mask, margin):
    keep = margin >= MARGIN
    left_out = 1.0 - keep.mean()
    print("mask: %d of %d voxels inside the %.0e margin" % ((~keep).sum(), keep.size, MARGIN))
    assert left_out <= MAX_LEFT_OUT, left_out
    assert np.array_equal(got[keep], mask[keep])


def batch_box(chunk, patch, vol_shape):
    lo = tuple(min(e[a] for e in chunk) for a in range(3))
    hi = tuple(min(max(e[a] for e in chunk) + patch[a], vol_shape[a]) for a in range(3))
    return lo, hi


def all_entries(vol_shape, patch, overlap, mirror_axes):
    flips = [sum(1 << a for a in s) for r in range(len(mirror_axes) + 1) for s in itertools.combinations(mirror_axes, r)]
    return [o + (f,) for o in pp.window_origins(vol_shape, patch, overlap) for f in flips]


# ------------------------------------------------------------------------------------------------ 1. window_origins
@pytest.mark.parametrize("overlap", [0.0, 0.5, 0.75])
@pytest.mark.parametrize("vol,patch", ORIGIN_SHAPES)
def test_window_origins_cover_the_volume(vol, patch, overlap):
    o = pp.window_origins(vol, patch, overlap)
    assert o == sorted(o) and len(set(o)) == len(o)                    # z-major, x fastest, no repeats
    count = np.zeros(vol, int)
    for z, y, x in o:
        assert min(z, y, x) >= 0
        for s, n, p in zip((z, y, x), vol, patch):
            assert s + p <= max(n, p)                                  # inside the volume (or the single overhanging window)
        count[z:z + patch[0], y:y + patch[1], x:x + patch[2]] += 1
    assert count.min() >= 1
    for a in range(3):
        assert max(e[a] for e in o) == max(0, vol[a] - patch[a])       # the last window ends on the far border
    if overlap == 0.0 and all(n % p == 0 or n <= p for n, p in zip(vol, patch)):
        assert count.max() == 1                                        # overlap 0 tiles
    if overlap == 0.0:
        for a in range(3):                                             # steps of a whole patch, except the border window
            starts = sorted(set(e[a] for e in o))
            assert all(b - c == patch[a] for c, b in zip(starts[:-2], starts[1:-1]))


def test_window_origins_overlap_range():
    for bad in (1.0, 1.5, -0.1):
        with pytest.raises(ValueError):
            pp.window_origins((16, 16, 16), (8, 8, 8), bad)
    assert pp.window_origins((16, 16, 16), (8, 8, 8), 0.99)[1] == (0, 0, 1)      # the step never drops below one voxel


def test_importance_vectors():
    assert np.array_equal(pp.importance_1d(7, "constant"), np.ones(7, np.float32))
    for p in (1, 8, 16, 96):
        g = pp.importance_1d(p, "gaussian")
        i = np.arange(p)
        want = np.exp(-(i - (p - 1) / 2.0) ** 2 / (2 * (0.125 * p) ** 2))
        want = np.maximum(want / want.max(), 1e-3)
        assert g.dtype == np.float32 and g.shape == (p,) and np.allclose(g, want, rtol=1e-6, atol=0)
        assert g.max() == 1.0 and g.min() >= np.float32(1e-3) and np.array_equal(g, g[::-1])
    assert pp.importance_1d(96, "gaussian").min() == np.float32(1e-3)            # the floor is reached at the network's patch size
    with pytest.raises(ValueError):
        pp.importance_1d(8, "triangle")


# ------------------------------------------------------------------------------------------------ gather
@pytest.mark.parametrize("vol,patch", SHAPES + [((9, 10, 11), (4, 6, 7))])          # the last one: pw % 4 != 0, the scalar store path
def test_gather_windows_mirrors_and_pads(dev, vol, patch):
    rs = np.random.RandomState(1)
    v = rs.randn(*vol).astype(np.float32)
    entries = [o + (f,) for o, f in zip(pp.window_origins(vol, patch, 0.5), itertools.cycle(range(8)))]
    entries.append((max(0, vol[0] - 2), vol[1] - 3, vol[2] - 1, 5))                       # overhangs every axis
    got = pp.gather_windows(_t(v, dev), torch.tensor(entries, dtype=torch.int32, device=dev), patch, pad_value=-7.0).cpu().numpy()
    assert got.shape == (len(entries), 1) + patch
    for b, e in enumerate(entries):
        assert np.array_equal(got[b, 0], ref_window(v, e, patch, -7.0)), e


# ------------------------------------------------------------------------------------------------ 2. blend parity, 5. determinism
@functools.lru_cache(maxsize=None)
def blend_case(vol, patch, c, blend):
    """entries (every window once plain and once with random flip bits), random window probabilities, the restatement's answer"""
    rs = np.random.RandomState(zlib.crc32(repr((vol, patch, c, blend)).encode()))
    entries = []
    for o in pp.window_origins(vol, patch, 0.5):
        entries += [o + (0,), o + (int(rs.randint(1, 8)),)]
    probs = rs.rand(len(entries), c, *patch)
    if c > 1:
        probs /= probs.sum(1, keepdims=True)
    probs = probs.astype(np.float32)
    weights = [pp.importance_1d(p, blend) for p in patch]
    acc, wsum = ref_blend(vol, patch, entries, probs, weights)
    return entries, probs, weights, ref_finalize(acc, wsum)


def run_blend(dev, vol, patch, c, blend, bs):
    entries, probs, weights, _ = blend_case(vol, patch, c, blend)
    acc = torch.zeros((c,) + vol, dtype=torch.float32, device=dev)
    wsum = torch.zeros(vol, dtype=torch.float32, device=dev)
    w = [_t(x, dev) for x in weights]
    for s in range(0, len(entries), bs):
        chunk = entries[s:s + bs]
        # batches of one window go through the default box (the whole volume), larger ones through the windows' bounding box
        box = batch_box(chunk, patch, vol) if bs > 1 else None
        pp.blend_windows(_t(probs[s:s + bs], dev), torch.tensor(chunk, dtype=torch.int32, device=dev), w, acc, wsum, box)
    mask, p = pp.blend_finalize(acc, wsum, 0.5, 1, return_probs=True)
    return acc, wsum, mask, p


@pytest.mark.parametrize("bs", [1, 5])
@pytest.mark.parametrize("blend", ["constant", "gaussian"])
@pytest.mark.parametrize("c", [1, 3])
@pytest.mark.parametrize("vol,patch", SHAPES + QUAD_SHAPES)
def test_blend_matches_the_fp64_restatement(dev, vol, patch, c, blend, bs):
    _, _, _, (ref_p, ref_mask, margin) = blend_case(vol, patch, c, blend)
    acc, wsum, mask, p = run_blend(dev, vol, patch, c, blend, bs)
    err = np.abs(p.cpu().numpy() - ref_p).max()
    print("blended probabilities: max |d| = %.2e" % err)
    assert err <= PROB_TOL
    assert mask.dtype == torch.uint8 and tuple(mask.shape) == vol
    check_mask(mask.cpu().numpy(), ref_mask, margin)
    assert np.array_equal(pp.blend_finalize(acc, wsum, 0.5, 1).cpu().numpy(), mask.cpu().numpy())      # without probs_out: the same mask
    if c == 1:                                                                                         # the scale is applied to the mask
        assert np.array_equal(pp.blend_finalize(acc, wsum, 0.5, 255).cpu().numpy(), mask.cpu().numpy() * 255)


@pytest.mark.parametrize("c,blend", [(1, "gaussian"), (3, "constant")])
@pytest.mark.parametrize("vol,patch", SHAPES + QUAD_SHAPES)
def test_blend_is_deterministic(dev, vol, patch, c, blend):
    a = run_blend(dev, vol, patch, c, blend, 5)
    b = run_blend(dev, vol, patch, c, blend, 5)
    for x, y in zip(a, b):
        assert torch.equal(x, y)


def test_uncovered_voxels_give_zero(dev):
    vol, patch = (6, 8, 12), (4, 4, 8)
    rs = np.random.RandomState(3)
    for c in (1, 3):
        probs = (0.6 + 0.4 * rs.rand(1, c, *patch)).astype(np.float32)
        acc = torch.zeros((c,) + vol, dtype=torch.float32, device=dev)
        wsum = torch.zeros(vol, dtype=torch.float32, device=dev)
        pp.blend_windows(_t(probs, dev), torch.tensor([(1, 2, 3, 0)], dtype=torch.int32, device=dev), [np.ones(p, np.float32) for p in patch], acc, wsum)
        mask, p = pp.blend_finalize(acc, wsum, 0.5, 1, return_probs=True)
        inside = np.zeros(vol, bool)
        inside[1:5, 2:6, 3:11] = True
        assert np.array_equal(wsum.cpu().numpy() > 0, inside)
        assert (mask.cpu().numpy()[~inside] == 0).all() and (p.cpu().numpy()[:, ~inside] == 0).all()
        assert np.array_equal(p.cpu().numpy()[:, inside].reshape(c, *patch), probs[0])       # one window of weight 1: the probabilities themselves
        if c == 1:
            assert (mask.cpu().numpy()[inside] == 1).all()


@pytest.mark.gpu
def test_blend_offsets_beyond_2_31_elements():
    """sixteen classes of a 576 x 512 x 512 field: acc holds 2.4e9 floats, so a window in the far corner is reached only with 64-bit
    offsets (class 15 starts at element 2.26e9).  The launch covers the window's box alone; one window of weight 1."""
    dev = torch.device("cuda:0")
    vol, patch, c = (576, 512, 512), (4, 8, 16), 16
    origin = tuple(v - p for v, p in zip(vol, patch))
    rs = np.random.RandomState(9)
    probs = rs.rand(1, c, *patch).astype(np.float32)
    acc = torch.zeros((c,) + vol, dtype=torch.float32, device=dev)
    wsum = torch.zeros(vol, dtype=torch.float32, device=dev)
    e = torch.tensor([origin + (4,)], dtype=torch.int32, device=dev)
    pp.blend_windows(_t(probs, dev), e, [np.ones(p, np.float32) for p in patch], acc, wsum, (origin, vol))
    mask = pp.blend_finalize(acc, wsum)
    corner = tuple(slice(o, None) for o in origin)
    want = probs[0, :, :, :, ::-1]
    assert np.array_equal(acc[(slice(None),) + corner].cpu().numpy(), want)
    assert np.array_equal(mask[corner].cpu().numpy(), want.argmax(0).astype(np.uint8))
    assert float(wsum.sum()) == float(np.prod(patch)) and int(mask.count_nonzero()) == int((want.argmax(0) != 0).sum())
    assert float(acc[:15].sum(dtype=torch.float64)) == pytest.approx(float(want[:15].astype(np.float64).sum()), rel=1e-12)


# ------------------------------------------------------------------------------------------------ 3. pointwise invariance
def _pointwise_fn(c):
    if c == 1:
        return lambda x: torch.sigmoid(1.7 * x - 0.3)
    a = torch.tensor([1.3, -0.8, 0.4]).view(1, 3, 1, 1, 1)
    b = torch.tensor([0.1, 0.5, -0.6]).view(1, 3, 1, 1, 1)
    return lambda x: torch.softmax(a.to(x.device) * x + b.to(x.device), 1)


@pytest.mark.parametrize("c", [1, 3])
@pytest.mark.parametrize("vol,patch", SHAPES + QUAD_SHAPES)
def test_pointwise_network_is_reproduced_on_the_whole_volume(dev, vol, patch, c):
    """a network that acts voxel by voxel must come back unchanged: a wrong flip, a wrong un-flip, padding leaking into the volume or a
    mis-indexed weight breaks this"""
    v = np.random.RandomState(5).randn(*vol).astype(np.float32)
    fn, sizes = _pointwise_fn(c), []

    def counted(x):
        sizes.append(x.shape[0])
        return fn(x)
    mask, p = pp.sliding_window_predict(counted, _t(v, dev), patch, c, batch_size=3, overlap=0.5, blend="gaussian", mirror_axes=(0, 1, 2),
                                        return_probs=True)
    want = fn(torch.from_numpy(v)[None, None].double())[0].numpy()
    assert tuple(p.shape) == (c,) + vol
    n = 8 * len(pp.window_origins(vol, patch, 0.5))
    assert sizes == [3] * ((n + 2) // 3)               # the network sees one batch size; the fill of the last batch is not blended
    err = np.abs(p.cpu().numpy() - want).max()
    print("pointwise: max |d| = %.2e" % err)
    assert err <= PROB_TOL
    _, ref_mask, margin = ref_finalize(want, np.ones(vol))
    check_mask(mask.cpu().numpy(), ref_mask, margin)


# ------------------------------------------------------------------------------------------------ 4. position dependence
def _ramp_fn(c, patch):
    n = patch[0] * patch[1] * patch[2]
    ramp = (torch.arange(n, dtype=torch.float32).view(1, 1, *patch) + 0.5) / n           # the position inside the window the network sees

    def fn(x):
        r = ramp.to(x.device).expand(x.shape[0], 1, *patch)
        return r if c == 1 else torch.cat([r * 0.5, 0.3 + 0 * r, 0.7 - r * 0.5], 1)
    return fn


@pytest.mark.parametrize("c", [1, 3])
@pytest.mark.parametrize("vol,patch", SHAPES)
def test_position_dependent_network_and_importance_map(dev, vol, patch, c):
    v = np.zeros(vol, np.float32)
    fn = _ramp_fn(c, patch)
    entries = all_entries(vol, patch, 0.5, (2,))
    assert len(entries) % 3
    per_window = fn(torch.zeros((len(entries), 1) + patch)).numpy()
    got = {}
    for blend in ("constant", "gaussian"):
        # batches of 3 leave a short last batch at every shape: its fill (a repeat of the last window) must not be blended
        mask, p = pp.sliding_window_predict(fn, _t(v, dev), patch, c, batch_size=3, overlap=0.5, blend=blend, mirror_axes=(2,), return_probs=True)
        ref_p, ref_mask, margin = ref_finalize(*ref_blend(vol, patch, entries, per_window, [pp.importance_1d(q, blend) for q in patch]))
        err = np.abs(p.cpu().numpy() - ref_p).max()
        print("%s blend: max |d| = %.2e" % (blend, err))
        assert err <= PROB_TOL
        check_mask(mask.cpu().numpy(), ref_mask, margin)
        got[blend] = p.cpu().numpy()
    assert len(pp.window_origins(vol, patch, 0.5)) > 1
    assert np.abs(got["gaussian"] - got["constant"]).max() > 1e-3          # an importance map that is silently ignored fails here


# ------------------------------------------------------------------------------------------------ 6. errors
def test_bad_arguments_raise_with_the_library_message(dev):
    patch, vol = (4, 4, 8), (6, 8, 12)
    e = torch.tensor([(0, 0, 0, 0)], dtype=torch.int32, device=dev)
    w = [np.ones(p, np.float32) for p in patch]
    acc = torch.zeros((1,) + vol, dtype=torch.float32, device=dev)
    wsum = torch.zeros(vol, dtype=torch.float32, device=dev)
    probs = torch.zeros((1, 1) + patch, dtype=torch.float32, device=dev)
    with pytest.raises(RuntimeError):                                           # acc / wsum of different volumes
        pp.blend_windows(probs, e, w, acc, torch.zeros((6, 8, 13), dtype=torch.float32, device=dev))
    with pytest.raises(RuntimeError):                                           # class counts differ
        pp.blend_windows(torch.zeros((1, 2) + patch, dtype=torch.float32, device=dev), e, w, acc, wsum)
    with pytest.raises(RuntimeError):                                           # importance vector of the wrong length
        pp.blend_windows(probs, e, [w[0], w[1], np.ones(7, np.float32)], acc, wsum)
    with pytest.raises(RuntimeError):                                           # two entries for one window of probabilities
        pp.blend_windows(probs, torch.zeros((2, 4), dtype=torch.int32, device=dev), w, acc, wsum)
    with pytest.raises(RuntimeError, match="classes must be 1..16"):
        pp.blend_windows(torch.zeros((1, 17) + patch, dtype=torch.float32, device=dev), e, w, torch.zeros((17,) + vol, dtype=torch.float32, device=dev), wsum)
    with pytest.raises(RuntimeError, match="classes must be 1..16"):
        pp.blend_finalize(torch.zeros((17,) + vol, dtype=torch.float32, device=dev), wsum)
    for box in (((0, 0, 0), (6, 8, 13)), ((-1, 0, 0), (6, 8, 12)), ((0, 9, 0), (6, 8, 12)), ((3, 0, 0), (3, 8, 12))):
        with pytest.raises(RuntimeError, match="inside the volume"):
            pp.blend_windows(probs, e, w, acc, wsum, box)
    assert float(acc.abs().max()) == 0.0 and float(wsum.abs().max()) == 0.0     # a refused call launches nothing
    with pytest.raises(RuntimeError):
        pp.blend_finalize(acc, torch.zeros((6, 8, 13), dtype=torch.float32, device=dev))
    with pytest.raises(RuntimeError):                                           # entries must be {z, y, x, flipbits}
        pp.gather_windows(torch.zeros(vol, device=dev), torch.zeros((1, 3), dtype=torch.int32, device=dev), patch)
    with pytest.raises(ValueError):
        pp.sliding_window_predict(lambda x: x, torch.zeros(vol, device=dev), patch, 1, overlap=1.0)
    with pytest.raises(RuntimeError):                                           # fn answers with the wrong class count
        pp.sliding_window_predict(lambda x: x, torch.zeros(vol, device=dev), patch, 2)
