"""TEST INFRASTRUCTURE ONLY: plain-torch restatement of the reference's Grad-CAM (model/visualization.py:112-238) for the classifiers.  The forward pass is
cls_oracle.resnet_forward (eval mode) with the five block outputs kept (`retain_grad`), the map is the reference's arithmetic with cv2.resize replaced by
F.interpolate(mode = "bilinear" / "trilinear", align_corners = False) - the same taps and weights when enlarging.  Works in 2-D and 3-D, in the dtype of the
parameters it is handed.  Pinned against maps recorded from the reference's own class (tools/make_golden_gradcam.py, tests/golden/gradcam_2d.npz)."""
import os
import sys
import types
from collections import OrderedDict

import numpy as np
import torch
import torch.nn.functional as F

import cls_oracle
from oracle import seg_oracle as seg

NAMES = ("in_tr", "down_tr32", "down_tr64", "down_tr128", "down_tr256")
LAYER_SETS = OrderedDict((("down_tr256", ("down_tr256",)), ("down_tr64", ("down_tr64",)), ("in_tr", ("in_tr",)), ("all", NAMES)))
CASES_2D = [c for c in cls_oracle.CASES if c[1] == 2]


def golden_classes(numclass):
    """the first and the last class"""
    return sorted({0, numclass - 1})


def golden_key(tag, layer_set, cls):
    return "%s__%s__c%d" % (tag, layer_set, cls)


_inputs = {}


def case_inputs(tag):
    """(params, x) of a case of cls_oracle.CASES, as every side derives them from the seed; computed once, shared, never modified"""
    if tag not in _inputs:
        import conftest
        from pytorchdeeplearing_amd import networks
        _, ndim, shape, numclass, _, seed = {c[0]: c for c in cls_oracle.CASES}[tag]
        if not torch.cuda.is_available():
            conftest.emu_library()           # (the module reads its parameter table from whichever library serves the host)
        m = getattr(networks, "ResNet%dd" % ndim)(shape[1], numclass, dtype="f32")
        _inputs[tag] = (cls_oracle.seeded_params(m, networks.initialize_weights, seed), cls_oracle.batch(shape, numclass)[0])
    return _inputs[tag]


def forward_taps(P, x):
    """cls_oracle.resnet_forward in eval mode; returns (logits, {name: block output})"""
    ndim = x.dim() - 2
    conv = seg._conv(ndim)
    none = seg._Masks(None)
    taps = OrderedDict()
    gw, gb = P["in_tr.bn1.weight"], P["in_tr.bn1.bias"]
    out = (seg._gn_drop_relu(conv(x, P["in_tr.conv1.weight"], P["in_tr.conv1.bias"], padding=1), gw, gb, none) +
           seg._gn_drop_relu(conv(x, P["in_tr.conv2.weight"], P["in_tr.conv2.bias"]), gw, gb, none))
    taps["in_tr"] = out
    for pre in NAMES[1:]:
        down = seg._gn_drop_relu(conv(out, P[pre + ".down_conv.weight"], P[pre + ".down_conv.bias"], stride=2), P[pre + ".bn1.weight"], P[pre + ".bn1.bias"], none)
        t, i = down, 0
        while "%s.ops.%d.conv1.weight" % (pre, i) in P:
            op = "%s.ops.%d" % (pre, i)
            t = seg._gn_drop_relu(conv(t, P[op + ".conv1.weight"], P[op + ".conv1.bias"], padding=1), P[op + ".bn1.weight"], P[op + ".bn1.bias"], none)
            i += 1
        out = t + down
        taps[pre] = out
    pooled = out.reshape(out.shape[0], out.shape[1], -1).mean(2)
    h = F.relu(F.linear(pooled, P["fc_layers.0.weight"], P["fc_layers.0.bias"]))
    return F.linear(h, P["fc_layers.2.weight"], P["fc_layers.2.bias"]), taps


def features(params, x, target, dtype=torch.float64, autocast=None, scale=1.0):
    """(logits, {name: (activation, gradient of sum_n logits[n, target[n]] wrt it)}) as float64 tensors on the CPU.  autocast: a torch dtype - the passes run
    under torch.autocast on x's device with float32 parameters and `scale` times the score is differentiated (the engine's loss scale), so the taps and their
    gradients are stored in that dtype; the scale is divided out in float64."""
    cats = [int(target)] * x.shape[0] if not hasattr(target, "__len__") else [int(c) for c in target]
    P = OrderedDict((k, v.detach().to(device=x.device, dtype=torch.float32 if autocast else dtype)) for k, v in params.items())
    x = x.to(torch.float32 if autocast else dtype)
    if autocast:
        with torch.autocast(device_type=x.device.type, dtype=autocast):
            x = x.clone().requires_grad_(True)           # (the taps need a graph even though no parameter asks for a gradient)
            logits, taps = forward_taps(P, x)
    else:
        x = x.clone().requires_grad_(True)
        logits, taps = forward_taps(P, x)
    for t in taps.values():
        t.retain_grad()
    score = sum(logits[i, c] for i, c in enumerate(cats))
    (score.float() * scale if autocast else score).backward()
    return logits.detach().double().cpu(), OrderedDict((k, (t.detach().double().cpu(), t.grad.double().cpu() / scale)) for k, t in taps.items())


def scale_cam(m):
    """scale_cam_image (visualization.py:183-187) per sample, without the resize"""
    flat = m.reshape(m.shape[0], -1)
    shape = (m.shape[0],) + (1,) * (m.dim() - 1)
    mn = flat.min(1).values.reshape(shape)
    return (m - mn) / (1e-7 + (flat.max(1).values.reshape(shape) - mn))


def raw_map(a, g):
    """get_cam_image (visualization.py:146-151): (N, [D,] H, W), before the ReLU"""
    w = g.mean(tuple(range(2, g.dim())), keepdim=True)
    return (w * a).sum(1)


def layer_map(a, g, out_size):
    """compute_cam_per_layer (visualization.py:158-174) for one layer"""
    s = scale_cam(raw_map(a, g).clamp(min=0))
    return F.interpolate(s[:, None], size=tuple(out_size), mode="bilinear" if len(out_size) == 2 else "trilinear", align_corners=False)[:, 0]


def cam_map(feats, names, out_size):
    """the map of GradCAM.__call__ for the layers `names`; feats: {name: (activation, gradient)}"""
    layers = torch.stack([layer_map(*feats[n], out_size) for n in names], 1)
    return scale_cam(layers.clamp(min=0).mean(1))           # aggregate_multi_layers (visualization.py:176-180)


# ------------------------------------------------------------------------------------------------------------------------------------------
# the live reference's class (where the reference tree is present): three shims, no reference file is edited
# ------------------------------------------------------------------------------------------------------------------------------------------
def inter_linear_resize(img, dsize, interpolation=None):
    """cv2.resize(img, (width, height)) with INTER_LINEAR restated from its published definition for one float32 plane: source coordinate
    (o + 0.5) * in / out - 0.5 rounded to float32, taps floor / floor + 1 clamped to the axis (weight 0 on the clamped side), rows first, then columns."""
    img = np.asarray(img, dtype=np.float32)

    def axis(o_n, i_n):
        f = ((np.arange(o_n, dtype=np.float64) + 0.5) * (i_n / o_n) - 0.5).astype(np.float32)
        i0 = np.floor(f).astype(np.int64)
        w1 = (f - i0.astype(np.float32)).astype(np.float32)
        w1[(i0 < 0) | (i0 >= i_n - 1)] = 0
        i0 = np.clip(i0, 0, i_n - 1)
        return i0, np.minimum(i0 + 1, i_n - 1), w1

    x0, x1, wx = axis(int(dsize[0]), img.shape[1])
    y0, y1, wy = axis(int(dsize[1]), img.shape[0])
    rows = img[:, x0] * (np.float32(1) - wx) + img[:, x1] * wx
    return (rows[y0] * (np.float32(1) - wy)[:, None] + rows[y1] * wy[:, None]).astype(np.float32)


class ScoreTriple(torch.nn.Module):
    """what the reference's GradCAM unpacks from `model(x)`: (logits, softmax, argmax) - its own ResNet2d.forward returns the logits alone"""

    def __init__(self, net):
        super().__init__()
        self.net = net

    def forward(self, x):
        z = self.net(x)
        return z, torch.softmax(z, 1), torch.argmax(z, 1)


def load_reference_gradcam():
    """(reference networks package with prob = 0.2 set, the reference's GradCAM class)"""
    import importlib.util
    from oracle import ref_loader
    nets, _, _ = ref_loader.load()
    for name in ("ResNet3d", "ResNet2d"):
        sys.modules["ref_networks." + name].prob = 0.2              # tools/make_golden_cls.py: the module global the reference never defines
    if "ref_model.visualization" not in sys.modules:
        stubs = {"cv2": types.ModuleType("cv2"), "SimpleITK": types.ModuleType("SimpleITK")}
        stubs["cv2"].resize = inter_linear_resize
        saved = {k: sys.modules.get(k) for k in stubs}
        sys.modules.update(stubs)
        try:
            spec = importlib.util.spec_from_file_location("ref_model.visualization", os.path.join(ref_loader.REF, "model", "visualization.py"))
            mod = importlib.util.module_from_spec(spec)
            spec.loader.exec_module(mod)
            sys.modules["ref_model.visualization"] = mod
        finally:
            for k, v in saved.items():
                if v is None:
                    sys.modules.pop(k, None)
                else:
                    sys.modules[k] = v
    return nets, sys.modules["ref_model.visualization"].GradCAM


def reference_maps(nets, GradCAM, case, layer_names, cls):
    """the reference's map (N, H, W) float32 for one case, and the raw map's (min, max) per layer and sample: (L, N, 2)"""
    tag, ndim, shape, numclass, _, seed = case
    m = getattr(nets, "ResNet%dd" % ndim)(shape[1], numclass)
    m.load_state_dict(cls_oracle.seeded_params(m, nets.initialize_weights, seed), strict=True)
    x, _ = cls_oracle.batch(shape, numclass)
    cam = GradCAM(model=ScoreTriple(m), target_layers=[getattr(m, n) for n in layer_names], use_cuda=False)
    out = cam(input_tensor=x, target_category=cls)
    ag = cam.activations_and_grads
    raw = [cam.get_cam_image(a.numpy(), g.numpy()) for a, g in zip(ag.activations, ag.gradients)]
    mm = np.array([[[r[i].min(), r[i].max()] for i in range(r.shape[0])] for r in raw], dtype=np.float32)
    ag.release()
    return np.asarray(out, dtype=np.float32), mm
