"""TEST INFRASTRUCTURE ONLY: plain-torch restatement of the reference's classifiers (networks/ResNet3d.py:24-118, ResNet2d.py) on a parameter dict, built from
the blocks of oracle/seg_oracle.py.  Pinned against golden vectors recorded from the reference itself (tools/make_golden_cls.py, tests/test_resnet.py).

The reference's DownTransition reads an undefined module global `prob`; the goldens were recorded with prob = 0.2 (the VNet value) set on the reference
modules.  Channel dropout sits only behind each down_conv: `do1` is in place, so `down` itself is the dropped tensor and the residual adds it."""
from collections import OrderedDict

import torch
import torch.nn.functional as F

from oracle import seg_oracle as seg

CASES = [        # tag, ndim, input shape, numclass, loss, seed of `manual_seed(seed); apply(initialize_weights)`
    ("resnet3d_bin_16", 3, (2, 1, 16, 16, 16), 1, "BinaryCrossEntropyLoss", 200),
    ("resnet3d_mc2_v6", 3, (2, 1, 16, 32, 48), 2, "MutilCrossEntropyLoss", 201),
    ("resnet2d_bin_v6", 2, (2, 1, 32, 48), 1, "BinaryFocalLoss", 202),
    ("resnet2d_mc3_32", 2, (2, 3, 32, 32), 3, "MutilFocalLoss", 203),
]
PERTURB_SEED = 7
DATA_SEED = 1


def resnet_param_shapes(ndim, image_channel, numclass, feat=16):
    """state_dict layout of networks/ResNet3d.py:79-96: the VNet encoder's entries, then the two Linear layers"""
    P = OrderedDict((k, v) for k, v in seg.vnet_param_shapes(ndim, image_channel, 1, feat).items() if k.startswith(("in_tr.", "down_tr")))
    P["fc_layers.0.weight"], P["fc_layers.0.bias"] = (128, 16 * feat), (128,)
    P["fc_layers.2.weight"], P["fc_layers.2.bias"] = (numclass, 128), (numclass,)
    return P


def dropout_channels(feat=16):
    return [2 * feat, 4 * feat, 8 * feat, 16 * feat]


def resnet_forward(P, x, masks=None):
    """logits (N, numclass).  masks: None (eval) or the four (N, C) multipliers in call order"""
    ndim = x.dim() - 2
    conv = seg._conv(ndim)
    drop, none = seg._Masks(masks), seg._Masks(None)
    gw, gb = P["in_tr.bn1.weight"], P["in_tr.bn1.bias"]
    out = (seg._gn_drop_relu(conv(x, P["in_tr.conv1.weight"], P["in_tr.conv1.bias"], padding=1), gw, gb, none) +
           seg._gn_drop_relu(conv(x, P["in_tr.conv2.weight"], P["in_tr.conv2.bias"]), gw, gb, none))
    for pre in ("down_tr32", "down_tr64", "down_tr128", "down_tr256"):
        down = drop(seg._gn_drop_relu(conv(out, P[pre + ".down_conv.weight"], P[pre + ".down_conv.bias"], stride=2),
                                      P[pre + ".bn1.weight"], P[pre + ".bn1.bias"], none))            # relu, then the in-place dropout
        t, i = down, 0
        while "%s.ops.%d.conv1.weight" % (pre, i) in P:
            op = "%s.ops.%d" % (pre, i)
            t = seg._gn_drop_relu(conv(t, P[op + ".conv1.weight"], P[op + ".conv1.bias"], padding=1), P[op + ".bn1.weight"], P[op + ".bn1.bias"], none)
            i += 1
        out = t + down
    pooled = out.reshape(out.shape[0], out.shape[1], -1).mean(2)
    h = F.relu(F.linear(pooled, P["fc_layers.0.weight"], P["fc_layers.0.bias"]))
    return F.linear(h, P["fc_layers.2.weight"], P["fc_layers.2.bias"])


def labels(n, numclass, seed=DATA_SEED):
    """(N,) int64 class labels, as the reference's classification datasets deliver them"""
    g = torch.Generator().manual_seed(seed + 1000)
    return torch.randint(0, max(numclass, 2), (n,), generator=g)


def batch(shape, numclass, seed=DATA_SEED):
    x, _ = seg.synthetic_batch(shape[0], shape[2:], shape[1], 1, seed=seed)
    return x, labels(shape[0], numclass, seed)


def forward_backward(params, x, y, loss_name, masks=None):
    P = OrderedDict((k, v.detach().clone().requires_grad_(True)) for k, v in params.items())
    logits = resnet_forward(P, x, masks)
    loss = seg.loss_fn(loss_name, torch.ones(logits.shape[1]))(logits, y)
    loss.backward()
    return dict(loss=loss.detach(), logits=logits.detach(), grads=OrderedDict((k, v.grad) for k, v in P.items()))


def seeded_params(module, init_fn, seed):
    """the parameters every side starts from: `manual_seed(seed); module.apply(initialize_weights)` (value-identical between the reference's modules and
    this package's - tests/test_resnet.py checks the SHA-256 of every tensor), then the perturbation that makes biases and GroupNorm affines non-trivial"""
    torch.manual_seed(seed)
    module.apply(init_fn)
    return seg.perturb_params(OrderedDict((k, v.detach().clone()) for k, v in module.state_dict().items()), seed=PERTURB_SEED)
