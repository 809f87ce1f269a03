"""The script-facing Grad-CAM surface: `Grad_CAM_Visual` on the four ResNet wrappers (model/modelResNet.py:419-426 has it on MutilResNet2dModel),
`model.visualization.GradCAM` with the reference's constructor and call, and that a call leaves no state behind in the engine."""
import numpy as np
import pytest
import torch

import cls_oracle
import conftest
from pytorchdeeplearing_amd import _capi, networks
from pytorchdeeplearing_amd.engine import SegEngine

WRAPPERS = [("BinaryResNet2dModel", 2, 1), ("MutilResNet2dModel", 2, 3), ("BinaryResNet3dModel", 3, 1), ("MutilResNet3dModel", 3, 2)]


def make(dev, monkeypatch, cls, ndim, numclass, seed=5):
    import model
    monkeypatch.setenv("SEGENGINE_DTYPE", "f32")
    dims = (16, 16, 16) if ndim == 3 else (32, 48)
    m = getattr(model, cls)(*dims, 1, numclass, 2, use_cuda=dev.type == "cuda")
    torch.manual_seed(seed)
    m.model.apply(networks.initialize_weights)
    return m, dims


@pytest.mark.parametrize("cls,ndim,numclass", WRAPPERS)
def test_grad_cam_visual_on_the_four_wrappers(dev, monkeypatch, cls, ndim, numclass):
    """float32 of the input's spatial shape, values in [0, 1], and the map SegEngine.grad_cam gives for the same input (two runs of the same passes: equal on
    the checker, within 1e-5 on the device, where the GroupNorm statistics are summed with atomics)"""
    if ndim == 3:
        conftest.checker_slow(dev)
    m, dims = make(dev, monkeypatch, cls, ndim, numclass)
    img = np.random.RandomState(3).randn(1, *dims).astype(np.float32)
    net = m.model
    layers = [net.down_tr128, net.in_tr]
    cam = m.Grad_CAM_Visual(img, numclass - 1, layers)
    assert isinstance(cam, np.ndarray) and cam.dtype == np.float32 and cam.shape == dims
    assert float(cam.min()) >= 0.0 and float(cam.max()) <= 1.0 and float(cam.max()) > 0.99
    x = torch.from_numpy(img)[None].to(m.device)
    ref = net.engine.grad_cam(x, numclass - 1, ("down_tr128", "in_tr")).cpu().numpy()[0]
    if dev.type == "cpu":
        assert np.array_equal(cam, ref)
    assert float(np.abs(cam - ref).max()) <= 1e-5
    # target_category = None: the arg-max class of the sample, printed as the reference prints it
    with torch.no_grad():
        top = int(torch.argmax(net(x)[0]))
    auto = m.Grad_CAM_Visual(img, None, layers)
    assert net.engine.last_cam_categories == [top]
    assert float(np.abs(auto - net.engine.grad_cam(x, top, ("down_tr128", "in_tr")).cpu().numpy()[0]).max()) <= 1e-5
    # a class index is a class index, whatever holds it: a numpy scalar, a 0-d tensor
    for cat in (np.int64(top), torch.tensor(top), np.array(top)):
        assert float(np.abs(m.Grad_CAM_Visual(img, cat, layers) - auto).max()) <= 1e-5


def test_target_layers_are_resolved_by_identity(dev, monkeypatch, capsys):
    from model.visualization import GradCAM                     # the top-level package the reference scripts import
    from pytorchdeeplearing_amd.model import visualization
    assert GradCAM is visualization.GradCAM
    m, dims = make(dev, monkeypatch, "MutilResNet2dModel", 2, 3)
    net = m.model
    for bad in (net.fc_layers, net.down_tr32.ops, net.down_tr64.down_conv, torch.nn.ReLU()):
        with pytest.raises(ValueError, match="model.in_tr, model.down_tr32, model.down_tr64, model.down_tr128, model.down_tr256"):
            GradCAM(net, [net.down_tr256, bad])
    with pytest.raises(NotImplementedError, match="reshape_transform"):
        GradCAM(net, [net.down_tr256], reshape_transform=lambda t: t)
    with pytest.raises(NotImplementedError, match="activation of a target layer and its gradient"):
        m.Grad_CAM_Visual(np.zeros((1,) + dims), 0, [])
    cam = GradCAM(model=net, target_layers=[net.down_tr32, net.down_tr256], use_cuda=dev.type == "cuda")
    assert cam.names == ["down_tr32", "down_tr256"] and not net.training
    x = torch.from_numpy(np.random.RandomState(4).randn(2, 1, *dims).astype(np.float32))
    out = cam(input_tensor=x, target_category=None)
    assert out.dtype == np.float32 and out.shape == (2,) + dims
    with torch.no_grad():
        top = [int(c) for c in torch.argmax(net(x.to(m.device)), 1)]
    assert "category id: %s" % top in capsys.readouterr().out
    per_sample = cam(x, top)
    assert float(np.abs(out - per_sample).max()) <= 1e-5
    with cam as c:
        assert c is cam


def test_a_grad_cam_call_leaves_no_state_behind(dev):
    """f32, SEG_MASKS_GIVEN: two train steps after a Grad-CAM call give the losses and the parameters of the same steps without it - bit for bit on the
    host checker.  On the device the steps WITHOUT the call are not bit-reproducible among themselves (fp32 / fp64 atomics in the weight-gradient and
    GroupNorm sums, tests/test_engine.py says the same).  Measured on MI355X on this very case, 20 runs without and 20 with the call against one run
    without: losses equal in every run, parameters at most 2.33e-10 apart in BOTH groups (18 distinct parameter sets among the 40).  So there the test
    asserts that run-to-run spread with a small factor: parameters within 1e-8 (43 x the measured spread; a leftover of the call that moved a gradient by
    a percent would show at 1e-5 after two Adam steps), losses within 1e-6 relative (measured spread 0; the room is for an f32 rounding of the second
    step's loss going the other way on parameters 1e-10 apart).  What a step reads is also checked directly: parameters, loss scale and draw counter
    are untouched by the call."""
    shape, numclass = (2, 1, 16, 16), 3
    x, y = cls_oracle.batch(shape, numclass, seed=4)
    x, y = x.to(dev), y.to(dev)
    torch.manual_seed(3)
    net = networks.ResNet2d(1, numclass, dtype="f32")
    net.apply(networks.initialize_weights)
    sd = {k: v.detach().clone() for k, v in net.state_dict().items()}
    g = torch.Generator().manual_seed(9)
    masks = [(torch.rand((shape[0], c), generator=g) > 0.2).float() / 0.8 for c in cls_oracle.dropout_channels()]
    alpha = torch.ones(numclass, device=dev)
    runs = []
    for with_cam in (False, True):
        e = SegEngine("resnet", 2, 1, numclass, dtype="f32", device=dev)
        e.load_state_dict(sd)
        if with_cam:
            m = e.grad_cam(x, [0, 2], ("in_tr", "down_tr64", "down_tr256"))
            assert float(m.max()) > 0.99
            e.feature("down_tr32", grad=True)
            assert all(torch.equal(e.param_view(k).cpu(), v) for k, v in sd.items()) and e.loss_scale == 1.0 and e.lib.seg_dropout_draws(e.h) == 0
        losses = [float(e.train_step(x, y, "MutilFocalLoss", lr=1e-3, weight_decay=0.0, decoupled=False, class_alpha=alpha, mask_mode=_capi.MASKS_GIVEN,
                                     masks=masks)[0]) for _ in range(2)]
        runs.append((losses, e.params.detach().cpu().clone()))
    (l0, p0), (l1, p1) = runs
    d = (p0 - p1).abs()
    print("losses", l0, l1, "parameters max |d|", float(d.max()))
    if dev.type == "cpu":
        assert l0 == l1 and torch.equal(p0, p1), (l0, l1, float(d.max()))
    else:
        assert all(abs(a - b) <= 1e-6 * abs(a) for a, b in zip(l0, l1)) and float(d.max()) <= 1e-8, (l0, l1, float(d.max()))
