"""Operator-level parity of the Grad-CAM kernels (csrc/gradcam.hip) through seg_op_gradcam, without the planner, on shapes the planner never produces:
all three run dtypes against the float64 evaluation of tests/gradcam_oracle.py ON THE SAME ROUNDED INPUTS (the run dtype's own values), so what is
compared is the kernels' arithmetic alone.

Bound: 1e-5 absolute on maps with values in [0, 1].  The kernels round the channel weights once to fp32 (6e-8 relative, from an fp64 sum), add C products
per voxel in fp32 (C 6e-8 sum|w a|: with Gaussian data about 4e-7 of the map's range at C = 256), then divide, interpolate and scale in fp32 (a few 6e-8
each) - the largest difference seen, on the checker and on MI355X, is 2.3e-7 (printed by every check, pytest -s)."""
import pytest
import torch

import gradcam_oracle as gco
from pytorchdeeplearing_amd import ops

DT = ["f32", "f16", "bf16"]
BOUND = 1e-5


def inputs(n, c, isz, dtype, seed, negative_sample=None):
    """act and grad, channels-last, as the run dtype's own values in float32 (signed activations: the raw map then changes sign from voxel to voxel, so
    the ReLU and both ends of the scaling are exercised); negative_sample: that sample's activation is >= 0 and its gradient negative everywhere, so its
    raw map is negative everywhere"""
    g = torch.Generator().manual_seed(seed)
    act = torch.randn((n,) + tuple(isz) + (c,), generator=g)
    grad = torch.randn((n,) + tuple(isz) + (c,), generator=g)
    if negative_sample is not None:
        act[negative_sample] = act[negative_sample].abs()
        grad[negative_sample] = -grad[negative_sample].abs() - 0.1
    return act.to(ops.TORCH_DTYPE[dtype]).float(), grad.to(ops.TORCH_DTYPE[dtype]).float()


def planar64(t):
    return t.double().movedim(-1, 1)


def run(dev, dtype, layers, osz, inv_scale=1.0):
    """the map of `layers` = [(act, grad), ...] through one seg_op_gradcam call per layer"""
    out = None
    for i, (a, g) in enumerate(layers):
        ad, gd = (ops.aligned_like(t.to(ops.TORCH_DTYPE[dtype]).to(dev)) for t in (a, g))
        out = ops.gradcam_layer(ad, gd, dtype, osz, out=out, inv_loss_scale=inv_scale, weight=1.0 / len(layers), accumulate=i > 0, finalize=i == len(layers) - 1)
    return out.cpu()


def reference(layers, osz):
    feats = {i: (planar64(a), planar64(g)) for i, (a, g) in enumerate(layers)}
    return gco.cam_map(feats, list(feats), osz)


def check(name, got, ref):
    err = float((got.double() - ref).abs().max())
    print("max |d| %-28s %.3g" % (name, err))
    assert torch.isfinite(got).all() and err <= BOUND, (name, err)
    assert float(got.min()) >= 0.0 and float(got.max()) <= 1.0


SHAPES = [                              # n, c, input extents, output extents
    (1, 16, (2, 3), (32, 48)),          # clamped edges on every side, another ratio per axis
    (2, 16, (3, 5), (7, 11)),           # ratios that are no integers, sizes that are no multiple of a wave
    (2, 256, (3, 5), (7, 11)),
    (1, 256, (2, 3, 5), (5, 7, 11)),    # trilinear
    (2, 16, (2, 3, 5), (5, 7, 11)),
    (2, 16, (48, 48), (48, 48)),        # 2304 voxels: five slabs per sample, the last ragged - the folds across workgroups; ratio 1
]


@pytest.mark.parametrize("dtype", DT)
@pytest.mark.parametrize("n,c,isz,osz", SHAPES)
def test_one_layer_vs_float64(dev, dtype, n, c, isz, osz):
    a, g = inputs(n, c, isz, dtype, 3 + c + len(isz))
    ref = reference([(a, g)], osz)
    assert float(ref.reshape(n, -1).max(1).values.min()) > 0.99 and float(ref.reshape(n, -1).min(1).values.max()) == 0.0        # no sample's map is trivial
    check("%s %s->%s C%d" % (dtype, isz, osz, c), run(dev, dtype, [(a, g)], osz), ref)


@pytest.mark.parametrize("dtype", DT)
@pytest.mark.parametrize("c", [16, 256])
def test_one_voxel_gives_a_zero_map(dev, dtype, c):
    """min = max: the scaled layer map is exactly 0, and so is the aggregate"""
    for isz, osz in (((1, 1), (16, 16)), ((1, 1, 1), (4, 6, 8))):
        a, g = inputs(2, c, isz, dtype, 5)
        assert float(gco.raw_map(planar64(a), planar64(g)).abs().min()) > 0
        got = run(dev, dtype, [(a, g)], osz)
        assert tuple(got.shape) == (2,) + osz and torch.count_nonzero(got) == 0


@pytest.mark.parametrize("dtype", DT)
def test_scaling_is_per_sample_and_an_all_negative_sample_is_zero(dev, dtype):
    a, g = inputs(2, 16, (3, 5), dtype, 8, negative_sample=0)
    assert float(gco.raw_map(planar64(a), planar64(g))[0].max()) < 0
    got = run(dev, dtype, [(a, g)], (7, 11))
    check(dtype, got, reference([(a, g)], (7, 11)))
    assert torch.count_nonzero(got[0]) == 0 and not torch.isnan(got).any()
    assert float(got[1].max()) > 0.99 and float(got[1].min()) == 0.0
    # ... and the other sample's map does not depend on its neighbour
    alone = run(dev, dtype, [(a[1:], g[1:])], (7, 11))
    assert torch.equal(alone[0], got[1])


LAYER_STACKS = [
    ((12, 20), [(16, (3, 5)), (32, (6, 10))]),
    ((16, 32), [(16, (16, 32)), (32, (8, 16)), (64, (4, 8)), (128, (2, 4)), (256, (1, 2))]),        # the five taps of a 16 x 32 input
    ((4, 6, 10), [(16, (2, 3, 5)), (64, (1, 2, 3))]),
]


@pytest.mark.parametrize("dtype", DT)
@pytest.mark.parametrize("osz,stack", LAYER_STACKS)
def test_layers_of_different_extents_accumulate(dev, dtype, osz, stack):
    layers = [inputs(2, c, isz, dtype, 20 + i) for i, (c, isz) in enumerate(stack)]
    check("%s %d layers" % (dtype, len(layers)), run(dev, dtype, layers, osz), reference(layers, osz))


@pytest.mark.parametrize("dtype", DT)
def test_two_runs_agree_bit_for_bit(dev, dtype):
    layers = [inputs(2, 16, (48, 48), dtype, 30), inputs(2, 256, (3, 5), dtype, 31)]
    assert torch.equal(run(dev, dtype, layers, (48, 48)), run(dev, dtype, layers, (48, 48)))


@pytest.mark.parametrize("dtype", DT)
def test_the_loss_scale_is_divided_out(dev, dtype):
    """gradients times 1024 with inv_loss_scale = 1 / 1024 give the map of the unscaled gradients bit for bit: a power of two scales every fp64 sum, the
    division by V and the rounding to fp32 exactly.  (The 1e-7 of the scaling is not scale-invariant: the weights, not the map, carry the factor.)"""
    a, g = inputs(2, 16, (48, 48), dtype, 40)
    g1024 = (g * 1024).to(ops.TORCH_DTYPE[dtype]).float()
    assert torch.equal(g1024, g * 1024)
    plain = run(dev, dtype, [(a, g)], (48, 48))
    assert torch.equal(run(dev, dtype, [(a, g1024)], (48, 48), inv_scale=1.0 / 1024), plain)
    assert not torch.equal(run(dev, dtype, [(a, g1024)], (48, 48)), plain)


def test_bad_arguments_are_refused(dev):
    from pytorchdeeplearing_amd import _capi
    lib = _capi.lib_for(dev)
    assert lib.seg_op_gradcam_ws_bytes(0, 16, 1, 4, 4, 1, 8, 8) < 0 and lib.seg_op_gradcam_ws_bytes(1, 24, 1, 4, 4, 1, 8, 8) < 0
    assert lib.seg_op_gradcam_ws_bytes(1, 16, 1, 0, 4, 1, 8, 8) < 0 and lib.seg_op_gradcam_ws_bytes(1, 16, 1, 4, 4, 1, 8, 8) > 0
    a, g = inputs(1, 16, (3, 5), "f32", 1)
    a24 = torch.zeros((1, 3, 5, 24))
    with pytest.raises(RuntimeError, match="c must be 16"):
        ops.gradcam_layer(ops.aligned_like(a24.to(dev)), ops.aligned_like(a24.to(dev)), "f32", (7, 11))
    with pytest.raises(RuntimeError, match="positive and finite"):
        ops.gradcam_layer(ops.aligned_like(a.to(dev)), ops.aligned_like(g.to(dev)), "f32", (7, 11), inv_loss_scale=0.0)
