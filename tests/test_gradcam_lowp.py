"""Grad-CAM in the 16-bit run dtypes (GPU): what 16-bit storage of the activations and their gradients costs the maps, against the float64 oracle, and
next to stock PyTorch under torch.autocast on the same device and inputs.  No point-wise bound is fixed in advance for the shallow layers: there the
channel weights and the weighted sum are cancelling sums (the raw map of in_tr spans +-2e-3), and single pixels move by tenths in autocast as well."""
import pytest
import torch

import cls_oracle
import gradcam_oracle as gco
from pytorchdeeplearing_amd import _capi
from pytorchdeeplearing_amd.engine import SegEngine

CASE = {c[0]: c for c in cls_oracle.CASES}
TAGS = ["resnet2d_bin_v6", "resnet2d_mc3_32", "resnet3d_mc2_v6"]           # (resnet3d_bin_16: level 4 is one voxel, its map is 0 in every format)
TORCH = {"f16": torch.float16, "bf16": torch.bfloat16}
# down_tr256: the smaller of (a) twice the worst |map - float64 map| measured on MI355X over TAGS and every class (f16 2.62e-3, bf16 6.41e-2), rounded up to
# one digit (0.006, 0.2), and (b) the cap above which the error is a defect to find, not a bound to widen: four times / twice what torch.autocast shows on
# the CPU (0.01, 0.1).  For bf16 the cap is the one that binds.
DEEP_BOUND = {"f16": 0.006, "bf16": 0.1}
_runs = {}


def runs(dtype):
    """{(tag, cls): (engine maps per layer, autocast maps per layer, float64 maps per layer)} - computed once per dtype, shared, never modified"""
    if dtype not in _runs:
        dev = torch.device("cuda:0")
        _capi.product_library()
        out = {}
        for tag in TAGS:
            _, ndim, shape, numclass, _, _ = CASE[tag]
            params, x = gco.case_inputs(tag)
            e = SegEngine("resnet", ndim, shape[1], numclass, dtype=dtype, device=dev)
            e.load_state_dict(params)
            e.forward(x.to(dev), _capi.MASKS_EVAL)
            for cls in range(numclass):
                dl = torch.zeros((shape[0], numclass))
                dl[:, cls] = e.loss_scale
                e.backward(dl.to(dev), zero_grads=True)
                eng = {n: e.last_pass_cam((n,)).double().cpu() for n in gco.NAMES}
                f64 = gco.features(params, x, cls, dtype=torch.float64)[1]
                ac = gco.features(params, x.to(dev), cls, autocast=TORCH[dtype], scale=e.loss_scale)[1]
                out[(tag, cls)] = (eng, {n: gco.cam_map(ac, (n,), shape[2:]) for n in gco.NAMES}, {n: gco.cam_map(f64, (n,), shape[2:]) for n in gco.NAMES})
        _runs[dtype] = out
    return _runs[dtype]


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", ["f16", "bf16"])
def test_deepest_layer_vs_float64(dtype):
    """down_tr256 against the float64 oracle, point-wise.  Measured worst |d| on MI355X:
        f16   resnet2d_bin_v6 1.71e-3   resnet2d_mc3_32 c0 2.62e-3   resnet3d_mc2_v6 c1 2.16e-3
        bf16  resnet2d_bin_v6 2.79e-2   resnet2d_mc3_32 c0 6.41e-2   resnet3d_mc2_v6 c1 1.61e-2
    and exactly 0 on the three maps whose raw map is negative everywhere (resnet2d_mc3_32 c1 / c2, resnet3d_mc2_v6 c0)."""
    worst = 0.0
    for (tag, cls), (eng, _, f64) in runs(dtype).items():
        err = float((eng["down_tr256"] - f64["down_tr256"]).abs().max())
        print("%s %-16s c%d down_tr256 max |d| %.3g" % (dtype, tag, cls, err))
        worst = max(worst, err)
    print("%s down_tr256 worst %.3g (bound %.3g)" % (dtype, worst, DEEP_BOUND[dtype]))
    assert worst <= DEEP_BOUND[dtype]


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", ["f16", "bf16"])
def test_shallow_layers_vs_autocast(dtype):
    """in_tr .. down_tr128: the engine's mean absolute map error against float64 is at most 1.5 x that of the restatement under torch.autocast (same device,
    inputs and loss scale), per layer, pooled over TAGS and every class - the calibration used for the 16-bit parameter gradients.  Pooled, because a
    single map's error is dominated by the few pixels that set its minimum and maximum and scatters by a factor either way from map to map.
    Measured on MI355X, mean |d| engine : autocast (ratio), in_tr / down_tr32 / down_tr64 / down_tr128:
        f16   0.0105 : 0.0116 (0.90)   0.0137 : 0.0142 (0.96)   0.0089 : 0.0093 (0.95)   0.0048 : 0.0051 (0.94)
        bf16  0.0230 : 0.0274 (0.84)   0.0324 : 0.0348 (0.93)   0.0274 : 0.0274 (1.00)   0.0171 : 0.0178 (0.96)
    (worst single pixel, engine / autocast: f16 0.36 / 0.31 at in_tr, bf16 0.50 / 0.93 at in_tr.)
    What the pooling averages over, the ratio of every single map (6 maps x 4 layers x 2 dtypes, printed): 0.50 .. 1.69, 27 of the 48 below 1, 2 at 1.00,
    19 above; above 1.5: 1.54, 1.62, 1.64, 1.69 (four different case / class / layer / dtype combinations) against 0.50, 0.51, 0.54, 0.55, 0.55 at the
    other end - two independent 16-bit evaluations scattering around each other, no case or class in which the engine is systematically behind.  Each
    single map is held to 4 x autocast (twice the worst measured ratio, rounded up to one digit) so that an outlier cannot hide in a mean."""
    res = runs(dtype)
    mae, single = {}, {}
    for n in gco.NAMES[:-1]:
        e_mae = sum(float((eng[n] - f64[n]).abs().mean()) for eng, _, f64 in res.values()) / len(res)
        a_mae = sum(float((ac[n] - f64[n]).abs().mean()) for _, ac, f64 in res.values()) / len(res)
        e_max = max(float((eng[n] - f64[n]).abs().max()) for eng, _, f64 in res.values())
        a_max = max(float((ac[n] - f64[n]).abs().max()) for _, ac, f64 in res.values())
        print("%s %-10s mean |d| engine %.3g autocast %.3g ratio %.2f; worst |d| engine %.3g autocast %.3g" % (dtype, n, e_mae, a_mae, e_mae / a_mae, e_max, a_max))
        mae[n] = (e_mae, a_mae)
        for (tag, cls), (eng, ac, f64) in res.items():          # what the pooling averages over
            e1, a1 = float((eng[n] - f64[n]).abs().mean()), float((ac[n] - f64[n]).abs().mean())
            print("    %s %-10s %-16s c%d mean |d| engine %.3g autocast %.3g ratio %.2f" % (dtype, n, tag, cls, e1, a1, e1 / a1))
            single[(n, tag, cls)] = (e1, a1)
    for n, (e_mae, a_mae) in mae.items():            # (after every figure is printed)
        assert e_mae <= 1.5 * a_mae, (n, e_mae, a_mae)
    for k, (e1, a1) in single.items():
        assert e1 <= 4 * a1, (k, e1, a1)
