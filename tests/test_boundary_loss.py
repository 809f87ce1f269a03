"""seg_boundary_loss and the BinaryBoundaryLoss / MutilBoundaryLoss modules against float64 torch: softmax / sigmoid, the maps of the brute-force oracle
(tests/edt_oracle.py), .mean() over the selected planes, autograd for the gradient.

Bounds.  The loss is a signed sum that may cancel, so it is held to 1e-5 of the mean ABSOLUTE product: each f32 product carries about 4 * 2^-24 from expf and
the division plus the map's error, the accumulation is in double - 1e-5 leaves about a factor of ten.  The gradient's bracket phi_j - sum p_k phi_k cancels
too, so its error scales with max |phi| / M, not with the entry."""
import numpy as np
import pytest
import torch

import edt_oracle as oracle
from edt_oracle import CASES, UNIT


def binary_case(shape, seed):
    """logits 3 * randn of `shape` (N, 1, *spatial) and a 0 / 1 target with both kinds of voxel in every sample"""
    g = torch.Generator().manual_seed(seed)
    logits = 3.0 * torch.randn(shape, generator=g)
    if len(shape) == 5:
        target = CASES["labels"] != 0                              # (2, 6, 11, 70)
    else:
        target = np.random.default_rng(seed).random((shape[0],) + tuple(shape[2:])) < 0.3
    assert tuple(target.shape) == (shape[0],) + tuple(shape[2:])
    for s in target:
        assert s.any() and not s.all()
    return logits, torch.from_numpy(target.astype(np.uint8))


def multi_case(seed=21):
    g = torch.Generator().manual_seed(seed)
    return 3.0 * torch.randn((2, 4, 6, 11, 70), generator=g), torch.from_numpy(CASES["labels"].astype(np.int64))


def reference(logits, maps, first_class):
    """float64: (loss, gradient, mean |p * phi| over the selected planes, max |phi|, M)"""
    z = logits.double().clone().requires_grad_(True)
    phi = torch.from_numpy(maps)
    p = torch.sigmoid(z) if z.shape[1] == 1 else torch.softmax(z, dim=1)
    prod = (p * phi)[:, first_class:]
    loss = prod.mean()
    loss.backward()
    return float(loss.detach()), z.grad.numpy(), float(prod.detach().abs().mean()), float(phi.abs().max()), prod.numel()


def check(dev, module, logits, target, maps, first_class):
    want, wgrad, mean_abs, max_phi, m = reference(logits, maps, first_class)
    assert mean_abs > 0 and max_phi > 1
    x = logits.to(dev).clone().requires_grad_(True)             # (a copy: on the checker .to() hands back `logits` itself)
    got = module(x, target.to(dev))
    assert got.dtype == torch.float32 and got.dim() == 0
    got.backward()
    value = float(got.detach())
    print("boundary loss: got %.9g want %.9g, |diff| / mean|p phi| = %.3g" % (value, want, abs(value - want) / mean_abs))
    assert abs(value - want) <= 1e-5 * mean_abs
    gerr = np.abs(x.grad.cpu().numpy() - wgrad).max()
    print("boundary loss gradient: max error %.3g of the allowed %.3g" % (gerr, 1e-5 * max_phi / m))
    np.testing.assert_allclose(x.grad.cpu().numpy(), wgrad, rtol=0, atol=1e-5 * max_phi / m)
    return got, x.grad


@pytest.mark.parametrize("shape", [(2, 1, 6, 11, 70), (3, 1, 40, 70)], ids=["3d", "2d"])
def test_binary_boundary_loss(dev, shape):
    from pytorchdeeplearing_amd import losses, prepost
    from model import losses as shim
    assert shim.BinaryBoundaryLoss is losses.BinaryBoundaryLoss and shim.MutilBoundaryLoss is losses.MutilBoundaryLoss
    logits, target = binary_case(shape, seed=17)
    maps = oracle.boundary_maps(target.numpy(), 1)
    got, grad = check(dev, losses.BinaryBoundaryLoss(), logits, target, maps, 0)
    # maps handed in by the caller: the same loss, bit for bit, and a float target of the logits' shape is read as target != 0
    dm = prepost.boundary_distance_maps(target.to(dev), 1)
    np.testing.assert_allclose(dm.cpu().numpy(), maps, rtol=0, atol=2.0 ** -23 * np.abs(maps).max())      # (one f32 rounding of the root, one of the result)
    assert float(losses.BinaryBoundaryLoss()(logits.to(dev), target.to(dev), dist_maps=dm)) == float(got.detach())
    assert float(losses.BinaryBoundaryLoss()(logits.to(dev), (2.0 * target.to(dev).float()).unsqueeze(1))) == float(got.detach())


def test_binary_boundary_loss_with_spacing(dev):
    from pytorchdeeplearing_amd import losses
    logits, target = binary_case((2, 1, 6, 11, 70), seed=18)
    sampling = (2.5, 0.78, 0.78)
    check(dev, losses.BinaryBoundaryLoss(sampling=sampling), logits, target, oracle.boundary_maps(target.numpy(), 1, sampling), 0)


@pytest.mark.parametrize("include_background", [False, True], ids=["fg", "all"])
def test_multiclass_boundary_loss(dev, include_background):
    from pytorchdeeplearing_amd import losses
    logits, target = multi_case()
    maps = oracle.boundary_maps(target.numpy(), 4)
    assert not maps[1, 3].any() and maps[0, 3].any()              # class 3 is absent from sample 1: a zero plane there
    check(dev, losses.MutilBoundaryLoss(include_background=include_background), logits, target, maps, 0 if include_background else 1)


def op(dev, logits, maps, first_class, grad_scale=1.0, want_grad=True):
    """seg_boundary_loss through the C-ABI -> (loss, dlogits or None)"""
    from pytorchdeeplearing_amd import _capi
    from pytorchdeeplearing_amd.engine import aligned_empty
    lib = _capi.lib_for(dev)
    n, c = logits.shape[0], logits.shape[1]
    v = logits.numel() // (n * c)
    nbytes = lib.seg_boundary_loss_ws_bytes(n, c, v)
    lib.check(nbytes, "seg_boundary_loss_ws_bytes")
    ws = aligned_empty(nbytes, dev)
    out1 = torch.zeros(4, dtype=torch.float32, device=dev)
    dl = torch.full(logits.shape, float("nan"), dtype=torch.float32, device=dev) if want_grad else None
    lib.check(lib.seg_boundary_loss(logits.data_ptr(), maps.data_ptr(), n, c, v, first_class, grad_scale, ws.data_ptr(), out1.data_ptr(),
                                    dl.data_ptr() if want_grad else None, _capi.stream_for(dev)), "seg_boundary_loss")
    return float(out1[0]), dl


def test_op_grad_scale_null_gradient_and_errors(dev):
    from pytorchdeeplearing_amd import _capi
    logits, target = multi_case()
    maps64 = oracle.boundary_maps(target.numpy(), 4)
    _, wgrad, _, max_phi, m = reference(logits, maps64, 1)
    x, phi = logits.to(dev).contiguous(), torch.from_numpy(maps64.astype(np.float32)).to(dev)
    keep = x.clone()
    l1, g1 = op(dev, x, phi, 1, 1.0)
    l3, g3 = op(dev, x, phi, 1, 3.0)
    assert l1 == l3 and torch.equal(g3, 3.0 * g1)                  # the scale is the last factor: exact
    np.testing.assert_allclose(g3.cpu().numpy(), 3.0 * wgrad, rtol=0, atol=3e-5 * max_phi / m)
    assert float(g1[:, 0].abs().max()) > 0                         # the background logits get a gradient through the softmax
    l0, none = op(dev, x, phi, 1, 1.0, want_grad=False)
    assert none is None and l0 == l1 and torch.equal(x, keep)      # dlogits = NULL: the same loss, the logits untouched
    l1b, g1b = op(dev, x, phi, 1, 1.0)
    assert l1b == l1 and torch.equal(g1b, g1)                      # two calls agree bit for bit
    lib = _capi.lib_for(dev)
    n, c, v = 2, 4, x.numel() // 8
    out1 = torch.zeros(4, dtype=torch.float32, device=dev)
    ws = torch.zeros(16384, dtype=torch.uint8, device=dev)
    st = _capi.stream_for(dev)
    bad = [(None, phi.data_ptr(), n, c, v, 1, ws.data_ptr(), out1.data_ptr()), (x.data_ptr(), None, n, c, v, 1, ws.data_ptr(), out1.data_ptr()),
           (x.data_ptr(), phi.data_ptr(), n, c, v, 1, None, out1.data_ptr()), (x.data_ptr(), phi.data_ptr(), n, c, v, 1, ws.data_ptr(), None),
           (x.data_ptr(), phi.data_ptr(), 0, c, v, 1, ws.data_ptr(), out1.data_ptr()), (x.data_ptr(), phi.data_ptr(), n, 0, v, 1, ws.data_ptr(), out1.data_ptr()),
           (x.data_ptr(), phi.data_ptr(), n, 17, v, 1, ws.data_ptr(), out1.data_ptr()), (x.data_ptr(), phi.data_ptr(), n, c, 0, 1, ws.data_ptr(), out1.data_ptr()),
           (x.data_ptr(), phi.data_ptr(), n, c, v, 4, ws.data_ptr(), out1.data_ptr()), (x.data_ptr(), phi.data_ptr(), n, c, v, -1, ws.data_ptr(), out1.data_ptr())]
    for lg, ph, n_, c_, v_, fc, w_, o_ in bad:
        rc = lib.seg_boundary_loss(lg, ph, n_, c_, v_, fc, 1.0, w_, o_, None, st)
        assert rc < 0
        with pytest.raises(RuntimeError, match="seg_boundary_loss"):
            lib.check(rc, "seg_boundary_loss")
    assert float(out1.abs().max()) == 0


def test_low_precision_logits(dev):
    from pytorchdeeplearing_amd import losses
    logits, target = multi_case()
    x = logits.to(dev).half().requires_grad_(True)
    v = losses.MutilBoundaryLoss()(x, target.to(dev))
    v.backward()
    assert v.dtype == torch.float32 and x.grad.dtype == torch.float16 and x.grad.shape == x.shape
    ref = logits.half().float().to(dev).requires_grad_(True)      # the same values in f32: the same loss, the gradient rounded to f16
    w = losses.MutilBoundaryLoss()(ref, target.to(dev))
    w.backward()
    assert float(v.detach()) == float(w.detach()) and torch.equal(x.grad, ref.grad.half())


def test_no_foreground_gives_zero(dev):
    from pytorchdeeplearing_amd import losses
    g = torch.Generator().manual_seed(3)
    z = (3.0 * torch.randn((2, 1, 4, 9, 70), generator=g)).to(dev).requires_grad_(True)
    v = losses.BinaryBoundaryLoss()(z, torch.zeros((2, 4, 9, 70), dtype=torch.uint8, device=dev))
    v.backward()
    assert float(v.detach()) == 0.0 and not torch.isnan(z.grad).any() and float(z.grad.abs().max()) == 0.0
    z4 = (3.0 * torch.randn((2, 3, 4, 9, 70), generator=g)).to(dev).requires_grad_(True)
    v = losses.MutilBoundaryLoss(include_background=True)(z4, torch.zeros((2, 4, 9, 70), dtype=torch.int64, device=dev))
    v.backward()
    assert float(v.detach()) == 0.0 and not torch.isnan(z4.grad).any() and float(z4.grad.abs().max()) == 0.0
