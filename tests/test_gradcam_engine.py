"""Feature taps and Grad-CAM at engine level (seg_feature_find / seg_feature_read / seg_gradcam through SegEngine.feature, .grad_cam, .last_pass_cam)
against tests/gradcam_oracle.py evaluated in float64, and against the maps recorded from the reference's class (tests/golden/gradcam_2d.npz)."""
import functools
import os

import numpy as np
import pytest
import torch

import cls_oracle
import conftest
import gradcam_oracle as gco
from oracle import seg_oracle as seg
from pytorchdeeplearing_amd import _capi
from pytorchdeeplearing_amd.engine import SegEngine

CASE = {c[0]: c for c in cls_oracle.CASES}
TAGS = [c[0] for c in cls_oracle.CASES]
SLOW_ON_CHECKER = ("resnet3d_bin_16", "resnet3d_mc2_v6")          # minutes there (tests/test_resnet.py)


@functools.lru_cache(maxsize=None)
def golden():
    return dict(np.load(os.path.join(conftest.GOLDEN, "gradcam_2d.npz")))


@functools.lru_cache(maxsize=None)
def oracle64(tag, cls):
    """(logits, {name: (activation, gradient)}) in float64 for the class score `cls` of every sample: computed once, shared, never modified"""
    params, x = gco.case_inputs(tag)
    return gco.features(params, x, cls, dtype=torch.float64)


def one_hot(e, n, cls):
    dl = torch.zeros((n, e.numclass), dtype=torch.float32)
    dl[:, cls] = e.loss_scale
    return dl.to(e.device)


def rel(got, ref):
    return float((got.double().cpu() - ref).norm()), float(ref.norm())


@pytest.mark.parametrize("tag", TAGS)
def test_taps_and_maps_vs_oracle_and_golden(dev, tag):
    """f32 run dtype.  Every tap and its gradient: ||d|| <= 5e-3 ||ref|| + 1e-9 (the bound of test_resnet.py::check_grads; the ratios are printed); the
    activation is bit-identical before and after the backward pass; every map within 1e-4 of the float64 oracle and of the golden (the project's f32
    bound for logits: the maps are O(1) and were measured well conditioned in f32, 2.7e-6)."""
    if tag in SLOW_ON_CHECKER:
        conftest.checker_slow(dev)
    _, ndim, shape, numclass, _, _ = CASE[tag]
    params, x = gco.case_inputs(tag)
    e = SegEngine("resnet", ndim, shape[1], numclass, dtype="f32", device=dev)
    e.load_state_dict(params)
    xd = x.to(dev)
    worst = 0.0
    for cls in gco.golden_classes(numclass):
        logits64, feats = oracle64(tag, cls)
        logits, _ = e.forward(xd, _capi.MASKS_EVAL)
        assert float((logits.cpu().double() - logits64).abs().max()) < 1e-4
        before = {n: e.feature(n) for n in gco.NAMES}
        with pytest.raises(RuntimeError, match="holds no gradient"):
            e.feature("down_tr64", grad=True)
        e.backward(one_hot(e, shape[0], cls), zero_grads=True)
        for n in gco.NAMES:
            a, g = feats[n]
            assert tuple(before[n].shape) == tuple(a.shape) and before[n].dtype == torch.float32
            assert torch.equal(e.feature(n), before[n]), n
            for what, got, ref in (("act", before[n], a), ("grad", e.feature(n, grad=True), g)):
                d, r = rel(got, ref)
                print("%s c%d %-10s %-4s ||d|| / ||ref|| = %.2e" % (tag, cls, n, what, d / r))
                assert d <= 5e-3 * r + 1e-9, (n, what, d, r)
        for ls, names in gco.LAYER_SETS.items():
            got = e.last_pass_cam(names).cpu()
            ref = gco.cam_map(feats, names, shape[2:])
            assert tuple(got.shape) == (shape[0],) + tuple(shape[2:]) and got.dtype == torch.float32
            err = float((got.double() - ref).abs().max())
            worst = max(worst, err)
            assert err < 1e-4 and float(got.min()) >= 0.0 and float(got.max()) <= 1.0, (ls, cls, err)
            if ndim == 2:
                assert float((got - torch.from_numpy(golden()[gco.golden_key(tag, ls, cls)])).abs().max()) < 1e-4, (ls, cls)
    print(tag, "worst map error", worst)
    # the one-call form: forward, one-hot backward (one class per sample) and the map
    cls = gco.golden_classes(numclass)[-1]
    got = e.grad_cam(xd, [cls] * shape[0], ("down_tr256", "in_tr")).cpu()
    assert float((got.double() - gco.cam_map(oracle64(tag, cls)[1], ("down_tr256", "in_tr"), shape[2:])).abs().max()) < 1e-4


@pytest.mark.parametrize("dtype", ["f32", "f16", "bf16"])
def test_all_negative_maps_are_exactly_zero(dev, dtype):
    """resnet2d_mc3_32, down_tr256, classes 1 and 2 (raw map below -0.05 everywhere): zeros, not NaN, in every run dtype - the margin is 50 x a 16-bit rounding"""
    if dtype == "f16":
        conftest.checker_slow(dev, "a third engine on the host checker; bf16, the coarser format, runs there")
    tag = "resnet2d_mc3_32"
    _, ndim, shape, numclass, _, _ = CASE[tag]
    params, x = gco.case_inputs(tag)
    e = SegEngine("resnet", ndim, shape[1], numclass, dtype=dtype, device=dev)
    e.load_state_dict(params)
    e.forward(x.to(dev), _capi.MASKS_EVAL)
    for cls in (1, 2):
        e.backward(one_hot(e, shape[0], cls), zero_grads=True)
        m = e.last_pass_cam(("down_tr256",)).cpu()
        assert torch.count_nonzero(m) == 0 and not torch.isnan(m).any(), (dtype, cls)
        assert float(e.last_pass_cam(("down_tr128",)).max()) > 0.99              # (the pass did leave gradients)


def test_vnet_tap_gradient_sums_both_contributions(dev, monkeypatch):
    """a VNet skip level collects two gradient tensors (the decoder's concat conv and the next DownTransition): feature(grad=True) is their sum.  The oracle's
    tensor is caught where seg_oracle.vnet_forward hands it to down_tr128.down_conv."""
    kind, shape, ncls = "vnet", (2, 1, 32, 32), 2
    params = seg.perturb_params(seg.init_params(kind, 2, 1, ncls, seed=0), seed=7)
    x, _ = seg.synthetic_batch(shape[0], shape[2:], 1, ncls, seed=1)
    dl = torch.randn((shape[0], ncls) + shape[2:], generator=torch.Generator().manual_seed(2))
    P = {k: v.double() for k, v in params.items()}
    caught = {}
    conv2d = seg._conv(2)

    def conv(inp, w, *a, **kw):
        if w is P["down_tr128.down_conv.weight"]:
            inp.retain_grad()
            caught["down_tr64"] = inp
        return conv2d(inp, w, *a, **kw)

    monkeypatch.setattr(seg, "_conv", lambda ndim: conv)
    logits64, _ = seg.vnet_forward(P, x.double().requires_grad_(True))
    logits64.backward(dl.double())
    ref_a, ref_g = caught["down_tr64"].detach(), caught["down_tr64"].grad
    e = SegEngine(kind, 2, 1, ncls, dtype="f32", device=dev)
    e.load_state_dict(params)
    logits, _ = e.forward(x.to(dev), _capi.MASKS_EVAL)
    assert float((logits.cpu().double() - logits64.detach()).abs().max()) < 1e-3
    e.backward((dl * e.loss_scale).to(dev).contiguous(), zero_grads=True)
    for what, got, ref in (("act", e.feature("down_tr64"), ref_a), ("grad", e.feature("down_tr64", grad=True), ref_g)):
        d, r = rel(got, ref)
        print("vnet down_tr64 %-4s ||d|| / ||ref|| = %.2e" % (what, d / r))
        assert tuple(got.shape) == (2, 64, 8, 8) and d <= 5e-3 * r + 1e-9, (what, d, r)
    # the unscaled sum: a loss scale other than 1 is divided out
    e.loss_scale = 256.0
    e.forward(x.to(dev), _capi.MASKS_EVAL)
    e.backward((dl * 256.0).to(dev).contiguous(), zero_grads=True)
    d, r = rel(e.feature("down_tr64", grad=True), ref_g)
    assert d <= 5e-3 * r + 1e-9


def test_reads_without_the_pass_they_need_are_refused(dev):
    """the library's messages: unknown names, no forward pass, no (complete) backward pass, after a train step, after a re-plan; a UNet has no taps"""
    e = SegEngine("resnet", 2, 1, 2, dtype="f32", device=dev)
    torch.manual_seed(0)
    e.params.normal_(0, 0.05)
    x, y = cls_oracle.batch((2, 1, 16, 16), 2, seed=4)
    x, y = x.to(dev), y.to(dev)
    with pytest.raises(RuntimeError, match="no feature tap 'fc_layers'.*in_tr, down_tr32, down_tr64, down_tr128, down_tr256"):
        e.feature("fc_layers")
    with pytest.raises(RuntimeError, match="no forward pass"):
        e.feature("in_tr")
    e.forward(x)
    assert tuple(e.feature("down_tr256").shape) == (2, 256, 1, 1) and tuple(e.feature("in_tr").shape) == (2, 16, 16, 16)
    with pytest.raises(RuntimeError, match="holds no gradient: it needs a complete backward pass"):
        e.feature("in_tr", grad=True)
    with pytest.raises(RuntimeError, match="holds no gradient"):
        e.last_pass_cam(("in_tr",))
    dl = one_hot(e, 2, 1)
    nops = e.lib.seg_backward_ops(e.h)
    e.backward(dl, op_range=(0, nops // 2))
    with pytest.raises(RuntimeError, match="holds no gradient"):          # half a pass
        e.feature("in_tr", grad=True)
    e.backward(dl, zero_grads=False, op_range=(nops // 2, nops))
    assert tuple(e.feature("in_tr", grad=True).shape) == (2, 16, 16, 16)
    full = e.last_pass_cam(("in_tr", "down_tr32"))
    e.forward(x)
    e.backward(dl)
    assert float((e.last_pass_cam(("in_tr", "down_tr32")) - full).abs().max()) < 1e-5      # slices in order are a complete pass
    e.train_step(x, y, "MutilCrossEntropyLoss", mask_mode=_capi.MASKS_EVAL)
    for grad in (False, True):
        with pytest.raises(RuntimeError, match="holds no activation: no seg_forward at the current plan"):
            e.feature("in_tr", grad=grad)
    e.forward(x)
    e.backward(dl)
    e.feature("in_tr", grad=True)
    e.loss_scale = 1.0                                                     # the scale the pass ran with: nothing changes
    e.feature("in_tr", grad=True)
    e.loss_scale = 4.0                                                     # another one: the tensors carry the old scale, the activation is untouched
    with pytest.raises(RuntimeError, match="holds no gradient"):
        e.feature("in_tr", grad=True)
    with pytest.raises(RuntimeError, match="holds no gradient"):
        e.last_pass_cam(("in_tr",))
    e.feature("in_tr")
    e.loss_scale = 1.0
    e.forward(x)
    e.backward(dl)
    e.feature("in_tr", grad=True)
    e.forward(x[:1].contiguous())                                       # a re-plan; its forward is readable, the old gradient is gone
    assert tuple(e.feature("in_tr").shape) == (1, 16, 16, 16)
    with pytest.raises(RuntimeError, match="holds no gradient"):
        e.feature("in_tr", grad=True)
    with pytest.raises(ValueError):
        e.grad_cam(x, 2, ("in_tr",))                                       # class out of range
    with pytest.raises(ValueError):
        e.grad_cam(x, [0], ("in_tr",))                                     # one class for two samples
    u = SegEngine("unet", 2, 1, 1, dtype="f32", device=dev)
    with pytest.raises(RuntimeError, match="taps: none"):
        u.feature("in_tr")
