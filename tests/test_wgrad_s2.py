"""Weight gradients of the 2^d stride-2 windows through the multi-step streaming kernel (csrc/wgrad.hip wgrad_s2_kernel, switch SEG_WG_S2): the
down-convolutions (conv k2 s2, dW[co][ci][tap] = sum_m dY[m][co] X[2m + tap][ci]) and, with the roles of the tensors swapped, the ConvTranspose
up-convolutions (dW[ci][co][tap] = sum_m X[m][ci] dY[2m + tap][co]) of networks/VNet3d.py / Unet3d.py on 16-bit tensors.

Bounds.  1: integer data in [-2, 2], every product and sum exact in fp32 (|dW| < 2^24 asserted) -> equality with torch autograd.  2: the same voxel slices
as wgrad_kernel (SEG_WG_S2=2) and the same 32-row MFMA steps in ascending row order -> bit-identical on real-valued data.  3: the default slicing (fewer,
longer fp32 chains) moves the last bits; both paths are measured against the float64 gradient of the same rounded inputs, see MARGIN.  4: everything the
eligibility test turns away keeps wgrad_kernel and stays exact.  Every case asserts which kernel ran (ops.last_wgrad_kernel)."""
import pytest
import torch
import torch.nn.functional as F

import conftest
from pytorchdeeplearing_amd import ops
from test_ops import cl, ints, to_dev

DT16 = ["f16", "bf16"]
S2, GENERIC = 2, 0          # seg_op_wgrad_kernel ids

# role, ndim, N, coarse extents, cin, cout
A3 = ("conv", 3, 3, (3, 5, 7), 16, 32)      # OW odd and shorter than a step; steps straddle w-rows, planes and samples; M = 315: no multiple of 32 or 128
B3 = ("convT", 3, 2, (2, 3, 5), 32, 16)
C3 = ("conv", 3, 1, (1, 1, 1), 16, 32)      # M = 1: less than one MFMA step
D2 = ("conv", 2, 2, (5, 9), 16, 32)         # four taps
D2T = ("convT", 2, 2, (5, 9), 32, 16)
E3 = ("conv", 3, 1, (2, 3, 4), 16, 64)      # two p-tiles (grid.x = 2)
E3T = ("convT", 3, 1, (2, 3, 4), 64, 16)    # the shape class of VNet's up-convolutions (P = 2 x 16)
# GPU only.  M = 110592 rows; default slicing: 124 slices of 892 rows = 6 full 128-row steps + one of 124 rows - 7 steps per slice: the two-set
# register ring goes round 3 1/2 times and every slice ends on a ragged step
BIG = ("conv", 3, 1, (48, 48, 48), 16, 32)


def problem(case, seed, integer):
    """tensors of one layer with torch's weight gradient: returns (dr, x0) channels-last fp32 as ops.wgrad takes them, and w.grad (float64 for real data)"""
    role, ndim, N, sp, cin, cout = case
    g = torch.Generator().manual_seed(seed)
    draw = (lambda s: ints(s, -2, 2, g)) if integer else (lambda s: torch.randn(s, generator=g))
    fine = tuple(2 * s for s in sp)
    if role == "conv":
        x = draw((N, cin) + fine)
        w = torch.zeros((cout, cin) + (2,) * ndim, requires_grad=True)
        dy = draw((N, cout) + sp)
    else:
        x = draw((N, cin) + sp)
        w = torch.zeros((cin, cout) + (2,) * ndim, requires_grad=True)
        dy = draw((N, cout) + fine)
    return role, ndim, x, w, dy


def torch_grad(role, ndim, x, w, dy, dtype=None):
    """autograd of the reference's call; dtype: the 16-bit run dtype whose rounding the inputs get first, gradient in float64"""
    if dtype is not None:
        x, dy = x.to(ops.TORCH_DTYPE[dtype]).double(), dy.to(ops.TORCH_DTYPE[dtype]).double()
        w = w.detach().double().requires_grad_(True)
    f = {("conv", 3): F.conv3d, ("conv", 2): F.conv2d, ("convT", 3): F.conv_transpose3d, ("convT", 2): F.conv_transpose2d}[(role, ndim)]
    f(x, w, stride=2).backward(dy)
    return w.grad


def engine_grad(role, ndim, x, dy, dtype, dev, with_partial=False):
    dr, x0 = (dy, x) if role == "conv" else (x, dy)
    got = ops.wgrad(to_dev(cl(dr), dtype, dev), to_dev(cl(x0), dtype, dev), dtype, ndim, 2, 2, 0, with_partial=with_partial)
    return (got[0].cpu(), got[1].cpu()) if with_partial else got.cpu()


def slow(dev, case):
    if case is BIG:
        conftest.checker_slow(dev, "110 k voxel rows x 8 taps on the host checker")


# ------------------------------------------------------------------------------------------------------------------------------------------
# 1. exact on integer data
# ------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DT16)
@pytest.mark.parametrize("case", [A3, B3, C3, D2, D2T, E3, E3T, BIG], ids=["A3", "B3", "C3", "D2", "D2T", "E3", "E3T", "BIG"])
def test_wgrad_s2_exact(dev, dtype, case, monkeypatch):
    slow(dev, case)
    monkeypatch.delenv("SEG_WG_S2", raising=False)
    role, ndim, x, w, dy = problem(case, 11 + sum(case[3]), True)
    want = torch_grad(role, ndim, x, w, dy)
    assert 0 < float(want.abs().max()) < 2 ** 24
    got = engine_grad(role, ndim, x, dy, dtype, dev)
    assert ops.last_wgrad_kernel == S2
    assert torch.equal(got, want), float((got - want).abs().max())


# ------------------------------------------------------------------------------------------------------------------------------------------
# 2. the same slices as wgrad_kernel: bit-identical on real-valued data
# ------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DT16)
@pytest.mark.parametrize("case", [A3, B3, D2, BIG], ids=["A3", "B3", "D2", "BIG"])
def test_wgrad_s2_same_slices_bit_identical(dev, dtype, case, monkeypatch):
    slow(dev, case)
    """The partial tiles of every slice are equal, and so is dW wherever wgrad_reduce_kernel adds them in a fixed order: up to 32 slices.  Beyond that
    (BIG: 864 slices) its groups of 32 slices meet in dW through one float atomic each, in an order that differs between two launches of wgrad_kernel
    itself (measured on the device: 8 ulp) - there the sum of the equal partial tiles is compared within that freedom."""
    slow(dev, case)
    role, ndim, x, w, dy = problem(case, 5, False)
    res = {}
    for sw, kern in (("2", S2), ("0", GENERIC)):
        monkeypatch.setenv("SEG_WG_S2", sw)
        res[sw] = engine_grad(role, ndim, x, dy, dtype, dev, with_partial=True)
        assert ops.last_wgrad_kernel == kern
    (dw2, part2), (dw0, part0) = res["2"], res["0"]
    assert float(dw0.abs().max()) > 0 and not torch.isnan(part0).any()
    assert torch.equal(part2, part0), float((part2 - part0).abs().max())
    slices = part0.numel() // dw0.numel()
    if slices <= 32 or dev.type == "cpu":              # (the host checker runs the workgroups of a launch one after another)
        assert torch.equal(dw2, dw0), float((dw2 - dw0).abs().max())
    else:
        ulp = torch.finfo(torch.float32).eps * dw0.abs().max()
        assert float((dw2 - dw0).abs().max()) <= (slices + 31) // 32 * float(ulp)


# ------------------------------------------------------------------------------------------------------------------------------------------
# 3. default slicing on real-valued data
# ------------------------------------------------------------------------------------------------------------------------------------------
# relative L2 error of dW against the float64 gradient of the same rounded inputs (f16, conv 16 -> 32), data seeds 1, 2, 3
# (profiles/r09_wgrad_s2_oracle_error.txt).  MARGIN = the largest seed-to-seed ratio of wgrad_kernel's OWN error over those seeds, plus 25 %:
#   device, N = 2, coarse 24^3:  wgrad_kernel 1.338e-07, 1.322e-07, 1.320e-07 -> largest ratio 1.014   (default slices: 1.098e-07, 1.107e-07, 1.086e-07)
#   checker, N = 1, coarse 12^3: wgrad_kernel 1.176e-07, 1.154e-07, 1.145e-07 -> largest ratio 1.027   (default slices: 1.186e-07, 1.163e-07, 1.154e-07)
MARGIN = {"cuda": 1.014 * 1.25, "cpu": 1.027 * 1.25}


def test_wgrad_s2_default_slices_error_vs_float64(dev, monkeypatch):
    case = ("conv", 3, 2, (24, 24, 24), 16, 32) if dev.type == "cuda" else ("conv", 3, 1, (12, 12, 12), 16, 32)
    err = {"1": [], "0": []}
    for seed in (1, 2, 3):
        role, ndim, x, w, dy = problem(case, seed, False)
        want = torch_grad(role, ndim, x, w, dy, "f16")
        for sw, kern in (("1", S2), ("0", GENERIC)):
            monkeypatch.setenv("SEG_WG_S2", sw)
            got = engine_grad(role, ndim, x, dy, "f16", dev).double()
            assert ops.last_wgrad_kernel == kern
            err[sw].append(float((got - want).norm() / want.norm()))
    print("wgrad_s2 oracle error %s %s: default %s wgrad_kernel %s, wgrad_kernel seed-to-seed ratio %.3f" % (
        dev.type, case[3], ["%.3e" % e for e in err["1"]], ["%.3e" % e for e in err["0"]], max(err["0"]) / min(err["0"])))
    for e1, e0 in zip(err["1"], err["0"]):
        assert e1 <= e0 * MARGIN[dev.type], (err, MARGIN[dev.type])


# ------------------------------------------------------------------------------------------------------------------------------------------
# 4. what is not eligible keeps wgrad_kernel
# ------------------------------------------------------------------------------------------------------------------------------------------
def generic_case(dev, dtype, ndim, N, sp, cins, cout, k, stride, pad, seed):
    g = torch.Generator().manual_seed(seed)
    conv = F.conv3d if ndim == 3 else F.conv2d
    x = ints((N, sum(cins)) + sp, -2, 2, g)
    w = torch.zeros((cout, sum(cins)) + (k,) * ndim, requires_grad=True)
    y = conv(x, w, stride=stride, padding=pad)
    dy = ints(tuple(y.shape), -2, 2, g)
    y.backward(dy)
    xs = torch.split(x, cins, dim=1)
    x1 = to_dev(cl(xs[1]), dtype, dev) if len(xs) > 1 else None
    got = ops.wgrad(to_dev(cl(dy), dtype, dev), to_dev(cl(xs[0]), dtype, dev), dtype, ndim, k, stride, pad, x1=x1)
    assert ops.last_wgrad_kernel == GENERIC
    assert torch.equal(got.cpu(), w.grad), float((got.cpu() - w.grad).abs().max())


@pytest.mark.parametrize("why,args", [
    ("f32", ("f32", 3, 2, (4, 6, 4), [16], 32, 2, 2, 0)),
    ("concat source", ("f16", 3, 1, (4, 4, 6), [16, 16], 32, 2, 2, 0)),
    ("stride 1", ("f16", 3, 1, (3, 4, 5), [16], 32, 2, 1, 0)),
    ("k = 3", ("bf16", 2, 2, (7, 9), [16], 32, 3, 1, 1)),
    ("odd fine extent IW = 2 OW + 1", ("f16", 3, 1, (4, 6, 7), [16], 32, 2, 2, 0)),
    ("32-channel q-tile", ("f16", 3, 1, (4, 4, 4), [32], 64, 2, 2, 0)),
])
def test_wgrad_s2_ineligible_keeps_wgrad_kernel(dev, why, args, monkeypatch):
    monkeypatch.delenv("SEG_WG_S2", raising=False)
    generic_case(dev, *args, seed=17)


# ------------------------------------------------------------------------------------------------------------------------------------------
# engine level
# ------------------------------------------------------------------------------------------------------------------------------------------
def test_engine_down_and_up_conv_gradients_equal_under_same_slices(dev, monkeypatch):
    """VNet3d 2 x 1 x 16^3 f16, two steps (forward, loss, backward) on the same handle: the weight gradients of the down- and up-convolutions read from the
    engine's gradient buffer are equal with SEG_WG_S2=2 and =0 (down_tr32 and up_tr32 run wgrad_s2_kernel; the deeper ones have 32 or more input
    channels and keep wgrad_kernel either way).  Other tensors pass through float atomics: not compared."""
    conftest.checker_slow(dev, "four forward + backward passes of a 16-bit VNet3d on the host checker")
    from test_engine import build, run_engine
    res = {}
    for sw in ("2", "0"):
        monkeypatch.setenv("SEG_WG_S2", sw)
        e, params, x, y, masks, alpha, loss = build("vnet3d", "f16", dev, True)
        res[sw] = [run_engine(e, x, y, masks, alpha, loss, dev)[3] for _ in range(2)]
        del e
    keys = [k for k in res["0"][0] if k.endswith("down_conv.weight") or k.endswith("up_conv.weight")]
    assert len(keys) == 8
    for step in range(2):
        for k in keys:
            a, b = res["2"][step][k], res["0"][step][k]
            assert float(b.abs().max()) > 0, k
            assert torch.equal(a, b), (step, k, float((a - b).abs().max()))
