"""The weight / bias gradient of a one-class 1^d head collected by the GroupNorm-backward reduce passes under the head (SEG_HEAD_WFUSE; csrc/norm.hip
gn_bwd_reduce_kernel NDY 6 / 7, gn_head_w_fold; Planner::mark_head_wfuse) instead of head_bwd_kernel's pass over the head's input, and the train step that
then no longer writes that input.

    head input = relu(GN(L)) + xcat,  xcat = relu(GN(C)) stored in the run dtype T
    dW[c] = sum dl * relu(GN(L))[c]  (pass of unit L, fp32)  +  sum dl * round_T(relu(GN(C)))[c]  (pass of unit C),   db = sum dl

Bounds.  Operator level: integer data, every product and sum exact in fp32 -> equality.  Engine level: the switch changes nothing in the forward pass and
nothing in any backward launch but the two reduce / apply pairs, whose Q sums and d(raw) are computed by the same instructions - so everything except the
head's own gradient is compared like test_engine.test_step_riders_equal_separate_bookkeeping_launches compares its two runs (equal on the host checker,
whose launches run serially; |a - b| <= 2e-3 max(1, |b|) on the device, where the order of the fp64 atomics is free).  The head's gradient differs by
design - a_L + xcat_T in place of round_T(a_L + xcat_T), and another summation order - so both paths are measured against the fp64 oracle and the fused one
may be at most 1.25 x as far from it as head_bwd_kernel (the margin is for the summation order; the missing rounding can only help)."""
import pytest

import conftest
import torch

from oracle import seg_oracle as seg
from pytorchdeeplearing_amd import _capi, ops
from test_engine import CASES, build, run_engine
from test_norm import channel_sums, dev_f, dev_t, exact_inputs, scatter

DT = ["f32", "f16", "bf16"]
HEAD_KEYS = {"vnet": ("out_tr.conv.weight", "out_tr.conv.bias"), "unet": ("conv.weight", "conv.bias")}


# ------------------------------------------------------------------------------------------------------------------------------------------
# 1. operator level, exact
# ------------------------------------------------------------------------------------------------------------------------------------------
def run_head_exact(d, dev, dtype, path, rep, head):
    N, V, C = d["r"].shape
    g = torch.Generator().manual_seed(9)
    ident = {"mean": dev_f(torch.zeros(N, 8), dev), "rstd": dev_f(torch.ones(N, 8), dev)}
    stats = dev_f(scatter(channel_sums(d["r"].double()), rep, g, integer=True), dev, torch.float64)
    fwd = dict(ident, scale=dev_f(d["scale"], dev), shift=dev_f(d["shift"], dev))
    return ops.gn_backward([dev_t(x, dtype, dev) for x in d["dys"]], dev_t(d["r"], dtype, dev), fwd, stats, dev_f(torch.ones(C), dev), dtype, path, rep, rep,
                           vdl=dev_f(d["vdl"], dev), vw=dev_f(d["vw"], dev), head=head)


# V = 12^3: 1728 rows = full slabs of rows and a partial one; V = 24 * 40: 960 rows, fewer than 1024.  N = 2: two workgroups fold into the same gradient.
@pytest.mark.parametrize("dtype", DT)
@pytest.mark.parametrize("path,rep", [("fold", 4), ("separate", 32)])
@pytest.mark.parametrize("nstored", [0, 1])
@pytest.mark.parametrize("V", [12 * 12 * 12, 24 * 40])
def test_head_sums_on_the_reduce_pass_exact(dev, dtype, path, rep, nstored, V):
    """integer raw tensor, scale / shift and dl in {-2 .. 2}: the folded dW / db equal sum dl * act computed in fp64 bit for bit (act = relu(scale r + shift),
    half-integers at most: exact in all three run dtypes, so the rounding of the one-stored-source variant is the identity); Q, d(raw) and the other
    gradients equal those of the launch pair without the head sums"""
    C, N = 16, 2
    d = exact_inputs(C, N, V, nstored, 1, False, 700 + nstored + V)
    o = run_head_exact(d, dev, dtype, path, rep, True)
    p = run_head_exact(d, dev, dtype, path, rep, False)
    act = torch.relu(d["scale"][:, None, :].double() * d["r"].double() + d["shift"][:, None, :].double())
    dl = d["vdl"][:, 0, :].double()
    dw = torch.einsum("nv,nvc->c", dl, act)
    assert float(dw.abs().max()) < 2 ** 24 and dw.abs().max() > 0
    assert torch.equal(o["head_dw"].cpu().double(), dw), (o["head_dw"].cpu(), dw)
    assert torch.equal(o["head_db"].cpu().double(), dl.sum().reshape(1) if nstored == 0 else torch.zeros(1, dtype=torch.float64))
    hs = o["head_sums"].cpu()
    assert not hs[rep:].any(), "replicas beyond rep_q written"
    for k in ("Q", "dr", "dgamma", "dbeta", "dbias"):
        assert torch.equal(o[k].cpu(), p[k].cpu()), k
    assert torch.equal(o["Q"].cpu().sum(0), d["Q"])


def test_head_sums_refusals(dev):
    """two classes, a second stored source or the one-launch paths: refused, nothing launched"""
    d = exact_inputs(16, 1, 40, 1, 1, False, 3)
    with pytest.raises(RuntimeError, match="seg_op_gn_backward_head"):
        run_head_exact(d, dev, "f32", "coop", 4, True)
    d2 = exact_inputs(16, 1, 40, 0, 2, False, 4)
    with pytest.raises(RuntimeError, match="seg_op_gn_backward_head"):
        run_head_exact(d2, dev, "f32", "fold", 4, True)
    d3 = exact_inputs(16, 1, 40, 2, 1, False, 5)
    with pytest.raises(RuntimeError, match="seg_op_gn_backward_head"):
        run_head_exact(d3, dev, "f32", "fold", 4, True)


# ------------------------------------------------------------------------------------------------------------------------------------------
# 2. engine level
# ------------------------------------------------------------------------------------------------------------------------------------------
def close_as_riders(a, b, dev):
    """the comparison of two runs of test_step_riders_equal_separate_bookkeeping_launches"""
    if dev.type == "cpu":
        return torch.equal(a, b)
    return bool(((a - b).abs() <= 2e-3 * b.abs().clamp_min(1.0)).all())


_oracle64 = {}


def oracle64(tag, params, x, y, masks, alpha, loss):
    if tag not in _oracle64:
        p64 = {k: v.double() for k, v in params.items()}
        m64 = None if masks is None else [m.double() for m in masks]
        _oracle64[tag] = seg.forward_backward(CASES[tag][0], p64, x.double(), y, loss, masks=m64, alpha=alpha.double())["grads"]
    return _oracle64[tag]


@pytest.mark.parametrize("tag,dtype", [("vnet3d", "f32"), ("vnet2d_s", "f16"), ("vnet2d_s", "f32")])
def test_head_gradient_from_the_reduce_passes_equals_head_bwd(dev, tag, dtype, monkeypatch):
    if (tag, dtype) != ("vnet2d_s", "f32"):
        conftest.checker_slow(dev, "VNet3d 2 x 16^3 / a 16-bit VNet forward + backward twice on the host checker (the f32 VNet2d runs there)")
    res = {}
    for sw in ("2", "0"):
        monkeypatch.setenv("SEG_HEAD_WFUSE", sw)
        e, params, x, y, masks, alpha, loss = build(tag, dtype, dev, True)
        res[sw] = run_engine(e, x, y, masks, alpha, loss, dev)
        assert e.lib.seg_plan_count(e.h, 3) == (1 if sw == "2" else 0)
        del e
    (lg1, pr1, o1, g1), (lg0, pr0, o0, g0) = res["2"], res["0"]
    assert torch.equal(lg1, lg0) and torch.equal(pr1, pr0) and torch.equal(o1, o0)
    hw, hb = HEAD_KEYS[CASES[tag][0]]
    for k in g1:
        if k not in (hw, hb):
            assert close_as_riders(g1[k], g0[k], dev), (k, float((g1[k] - g0[k]).abs().max()))
    r64 = oracle64(tag, params, x, y, masks, alpha, loss)
    for k in (hw, hb):
        nrm = float(r64[k].norm()) + 1e-30
        err1 = float((g1[k].double() - r64[k]).norm()) / nrm
        err0 = float((g0[k].double() - r64[k]).norm()) / nrm
        print("%s %s %s: relative L2 error vs the fp64 oracle: fused %.3e, head_bwd_kernel %.3e" % (tag, dtype, k, err1, err0))
        assert err1 <= 1.25 * err0, (k, err1, err0)


def test_multi_class_head_keeps_head_bwd(dev, monkeypatch):
    """"unet3d" (4 classes): the planner falls back - the head launch stays in the profile, the gradients are those of SEG_HEAD_WFUSE=0"""
    res = {}
    for sw in ("2", "0"):
        monkeypatch.setenv("SEG_HEAD_WFUSE", sw)
        e, params, x, y, masks, alpha, loss = build("unet3d", "f32", dev, True)
        e.plan(x.shape[0], x.shape[2:])
        assert e.lib.seg_plan_count(e.h, 3) == 0
        if sw == "2":
            conftest.checker_slow(dev, "the two UNet3d passes behind the plan check")
        e.profile_enable(_capi.KERNEL_CLASSES)
        res[sw] = run_engine(e, x, y, masks, alpha, loss, dev)
        prof = e.profile_read()
        assert e.lib.seg_plan_count(e.h, 3) == 0
        assert prof["head"]["calls"] == 1, prof["head"]          # bwd_head (the forward head is inside the activation pass)
        del e
    for k in res["2"][3]:
        assert close_as_riders(res["2"][3][k], res["0"][3][k], dev), k


def test_one_class_unet_head_has_one_term(dev, monkeypatch):
    """UNet shape (no residual under the head: one reduce pass collects everything) - "unet2d", one class"""
    res = {}
    for sw in ("2", "0"):
        monkeypatch.setenv("SEG_HEAD_WFUSE", sw)
        e, params, x, y, masks, alpha, loss = build("unet2d", "f32", dev, True)
        res[sw] = run_engine(e, x, y, masks, alpha, loss, dev)
        assert e.lib.seg_plan_count(e.h, 3) == (1 if sw == "2" else 0)
        del e
    r64 = oracle64("unet2d", params, x, y, masks, alpha, loss)
    for k in res["2"][3]:
        if k in HEAD_KEYS["unet"]:
            nrm = float(r64[k].norm()) + 1e-30
            err1, err0 = (float((res[s][3][k].double() - r64[k]).norm()) / nrm for s in ("2", "0"))
            print("unet2d f32 %s: fused %.3e, head_bwd_kernel %.3e" % (k, err1, err0))
            assert err1 <= 1.25 * err0, (k, err1, err0)
        else:
            assert close_as_riders(res["2"][3][k], res["0"][3][k], dev), k


# ------------------------------------------------------------------------------------------------------------------------------------------
# 3. train steps: the head's input is not written there - and written again by the next plain forward
# ------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", ["f32", "f16"])
def test_train_steps_without_the_head_input_store(dev, dtype, monkeypatch):
    if dtype == "f16":
        conftest.checker_slow(dev, "16-bit VNet train steps on the host checker (the f32 case runs there)")
    tag, nsteps, lr = "vnet2d_s", 3 if dev.type != "cpu" else 1, 1e-3          # (the host checker takes half a minute per step: one there, like the riders test)
    res = []
    for sw in ("2", "0"):
        monkeypatch.setenv("SEG_HEAD_WFUSE", sw)
        e, params, x, y, _, alpha, loss = build(tag, dtype, dev, False)
        xd, yd = x.to(dev), y.to(dev)
        losses = [float(e.train_step(xd, yd, loss, lr=lr)[0]) for _ in range(nsteps)]
        p = e.params.clone().cpu()
        st = [int(v) for v in e.opt_state[:3].cpu()]
        with pytest.raises(RuntimeError, match="up_tr32"):
            e.feature("up_tr32")                   # a train step leaves nothing to read
        # the workspace slot of the head's input is stale now (SEG_HEAD_WFUSE=2 never wrote it): a plain forward of the first parameters must rewrite it
        e.load_state_dict(params)
        lg, _ = e.forward(xd)
        res.append((losses, p, st, e.feature("up_tr32").cpu(), lg.cpu()))
        del e
    (l1, p1, s1, f1, lg1), (l0, p0, s0, f0, lg0) = res
    assert s1 == s0 == [nsteps, 0, 0]
    for a, b in zip(l1, l0):
        assert abs(a - b) <= 2e-3 * max(1.0, abs(b)), (l1, l0)
    assert l1[0] == l0[0]                           # the first forward pass is the same pass
    # Adam moves a parameter by at most lr per step whatever the gradient: the riders test's bound for two runs whose gradients differ in rounding
    assert float((p1 - p0).abs().max()) <= nsteps * 2 * lr
    assert close_as_riders(lg1, lg0, dev)
    assert close_as_riders(f1, f0, dev) and float(f0.abs().max()) > 0
