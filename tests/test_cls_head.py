"""Operator-level parity of the classification head (csrc/cls_head.hip) through seg_op_cls_head_forward / seg_op_cls_head_backward, without the planner,
against plain torch in float64.

EXACT layer: small integers in the activation, signed powers of two (sparse) in the weights, V a power of two - every product, every sum and the division
by V is exact in fp32 and in the run dtype, so pooled, h, logits, every parameter gradient and d(activation) equal float64 torch bit for bit.

REAL layer: Gaussian data.  Every stage is compared with the float64 evaluation of that stage ON THE KERNEL'S OWN INPUTS of the stage (the run dtype's values
of the activation, the stored fp32 pooled / h / dh), so each bound covers one stage and follows from the number formats alone:
    u32 = 2^-24, uT = 2^-11 (f16) / 2^-8 (bf16) / 2^-24 (f32): one rounding, relative
  * pooled: an fp64 sum and quotient (no bound of their own) rounded once to fp32: u32 |ref|;
  * every fp32 sum (h, logits, dh, dW1, db1, dW2, db2): (n - 1) u32 sum|addends|, n counting the value the chain starts from (the bias, the value the gradient
    buffer holds, or 0) next to the products / terms - the kernels' fmaf chains and the wave butterfly round at most once per product or term, and the bound
    holds for any order; ReLU is 1-Lipschitz and the gate [h > 0] is taken from the stored h;
  * d(activation) = T(fl32(dpooled / V)): one run-dtype rounding uT |ref| (the fp32 rounding of the quotient in front of a 16-bit rounding vanishes in the
    gap between uT / (1 + uT) and uT: u32 (1 + 2 uT) <= uT^2), plus the f16 subnormal step, plus the bound of the 128-term fp32 sum dpooled carried through
    the division and the rounding: (1 + uT) 128 u32 sum|W1 dh| / V;
  * probs: sigmoid / soft-max of the kernel's own logits; expf is within 1 ulp = 2 u32, its argument z - max carries one rounding that the exponential turns
    into |z - max| u32, the sum of C positive terms (C - 1) u32, the quotient u32 - numerator and denominator together: (2 dmax + C + 5) u32 p.
No bound was taken from a run; every check prints its largest error / bound ratio (pytest -s), DESIGN.md section 2 quotes them."""
import math

import pytest
import torch

from pytorchdeeplearing_amd import ops

DT = ["f32", "f16", "bf16"]
U32 = 2.0 ** -24
UT = {"f32": 2.0 ** -24, "f16": 2.0 ** -11, "bf16": 2.0 ** -8}
SUBNORMAL_STEP = {"f32": 0.0, "f16": 2.0 ** -24, "bf16": 0.0}
K, H = 256, 128
GRADS = ("dw1", "db1", "dw2", "db2")
RATIOS = {}


def dev_f(x, dev):
    return ops.aligned_like(x.to(torch.float32).to(dev))


def dev_t(x, dtype, dev):
    return ops.aligned_like(x.to(ops.TORCH_DTYPE[dtype]).to(dev))


def check(name, got, ref, bound):
    """|got - ref| <= bound elementwise (bound 0: equal); prints the largest error / bound ratio"""
    err = (got.double().cpu() - ref.double()).abs()
    assert torch.isfinite(err).all(), name
    bound = bound.double().expand_as(err)
    ratio = float(torch.where(bound > 0, err / bound.clamp_min(1e-300), torch.where(err > 0, torch.full_like(err, math.inf), torch.zeros_like(err))).max())
    RATIOS[name] = max(RATIOS.get(name, 0.0), ratio)
    print("ratio %-8s %.4f" % (name, ratio))
    assert ratio <= 1.0, (name, ratio, float(err.max()))


def run(dev, dtype, act, w1, b1, w2, b2, dl, grads=None, zero_grads=True):
    """the two operator calls; returns everything on the host, fp64"""
    d = dict(w1=dev_f(w1, dev), b1=dev_f(b1, dev), w2=dev_f(w2, dev), b2=dev_f(b2, dev))
    fwd = ops.cls_head_forward(dev_t(act, dtype, dev), d["w1"], d["b1"], d["w2"], d["b2"], dtype)
    g = None if grads is None else {k: dev_f(v, dev) for k, v in grads.items()}
    bwd = ops.cls_head_backward(fwd, dev_f(dl, dev), d["w1"], d["w2"], dtype, grads=g, zero_grads=zero_grads)
    out = {k: fwd[k].cpu().clone() for k in ("logits", "probs", "pooled", "h")}
    out.update({k: bwd[k].cpu().clone() for k in GRADS + ("dact",)})
    return out


def reference(act, w1, b1, w2, b2, dl):
    """the whole head in float64 with autograd (act: the run dtype's values as fp64)"""
    a = act.double().requires_grad_(True)
    p = {k: v.double().requires_grad_(True) for k, v in dict(w1=w1, b1=b1, w2=w2, b2=b2).items()}
    pooled = a.mean(1)
    h = torch.relu(pooled @ p["w1"].t() + p["b1"])
    logits = h @ p["w2"].t() + p["b2"]
    logits.backward(dl.double())
    return dict(pooled=pooled.detach(), h=h.detach(), logits=logits.detach(), dw1=p["w1"].grad, db1=p["b1"].grad, dw2=p["w2"].grad, db2=p["b2"].grad,
                dact=a.grad)


# ------------------------------------------------------------------------------------------------------------------------------------------
# EXACT layer
# ------------------------------------------------------------------------------------------------------------------------------------------
def pow2(shape, density, g):
    """signed powers of two {0.5, 1, 2} at the given density, zero elsewhere"""
    mag = torch.tensor([0.5, 1.0, 2.0])[torch.randint(0, 3, shape, generator=g)]
    sign = torch.randint(0, 2, shape, generator=g).float() * 2 - 1
    return mag * sign * (torch.rand(shape, generator=g) < density).float()


@pytest.mark.parametrize("dtype", DT)
@pytest.mark.parametrize("N,V,C", [(1, 1, 1), (3, 8, 2), (3, 256, 5), (1, 1024, 2)])
def test_integer_layer_is_bit_exact(dev, dtype, N, V, C):
    g = torch.Generator().manual_seed(7 + N + V + C)
    act = torch.randint(-3, 4, (N, V, K), generator=g).float()
    w1, b1 = pow2((H, K), 1 / 32, g), torch.randint(-1, 3, (H,), generator=g).float()
    w2, b2 = pow2((C, H), 0.5, g).sign(), torch.randint(-2, 3, (C,), generator=g).float()
    dl = torch.randint(-1, 2, (N, C), generator=g).float()
    ref = reference(act, w1, b1, w2, b2, dl)
    # the layer is built so that the run dtype holds d(activation) exactly (bf16: 8 significant bits) and some units are on either side of the ReLU
    assert torch.equal(ref["dact"].to(ops.TORCH_DTYPE[dtype]).double(), ref["dact"])
    assert (ref["h"] > 0).any() and (ref["h"] == 0).any() and ref["dw1"].abs().sum() > 0
    got = run(dev, dtype, act, w1, b1, w2, b2, dl)
    for k in ("pooled", "h", "logits") + GRADS + ("dact",):
        assert torch.equal(got[k].double(), ref[k]), k
    p = torch.sigmoid(ref["logits"]) if C == 1 else torch.softmax(ref["logits"], 1)
    assert torch.allclose(got["probs"].double(), p, rtol=1e-5, atol=1e-7)


# ------------------------------------------------------------------------------------------------------------------------------------------
# REAL layer
# ------------------------------------------------------------------------------------------------------------------------------------------
def real_inputs(N, V, C, dtype, seed):
    g = torch.Generator().manual_seed(seed)
    act = (torch.randn((N, V, K), generator=g) + 0.25).to(ops.TORCH_DTYPE[dtype]).float()       # the run dtype's own values
    w1, b1 = torch.randn((H, K), generator=g) / 16, torch.randn((H,), generator=g) / 4
    w2, b2 = torch.randn((C, H), generator=g) / 8, torch.randn((C,), generator=g) / 4
    dl = torch.randn((N, C), generator=g)
    return act, w1, b1, w2, b2, dl


def check_real(got, act, w1, b1, w2, b2, dl, dtype, base=None):
    """stage by stage, each stage from the kernel's own stored inputs; base: what the gradient buffers held (zero_grads = 0)"""
    N, V, _ = act.shape
    C = w2.shape[0]
    a, W1, B1, W2, B2, DL = (t.double() for t in (act, w1, b1, w2, b2, dl))
    pooled, h = got["pooled"].double(), got["h"].double()
    ref = a.sum(1) / V
    check("pooled", got["pooled"], ref, U32 * ref.abs())
    prod = pooled[:, None, :] * W1[None]                                   # [N][H][K]
    check("h", got["h"], torch.relu(prod.sum(2) + B1), K * U32 * (prod.abs().sum(2) + B1.abs()))
    prod = h[:, None, :] * W2[None]                                        # [N][C][H]
    check("logits", got["logits"], prod.sum(2) + B2, H * U32 * (prod.abs().sum(2) + B2.abs()))
    z = got["logits"].double()
    if C == 1:
        p, dmax = torch.sigmoid(z), torch.zeros_like(z)
    else:
        p, dmax = torch.softmax(z, 1), (z.max(1, keepdim=True).values - z.min(1, keepdim=True).values).expand_as(z)
    check("probs", got["probs"], p, (2 * dmax + C + 5) * U32 * p)
    # backward: dh is not an output of the operator; its float64 value from the stored h carries the bound of its C-term chain into what reads it
    gate = (h > 0).double()
    prod = DL[:, :, None] * W2[None] * gate[:, None, :]                    # [N][C][H]
    dh, dh_err = prod.sum(1), C * U32 * prod.abs().sum(1)
    z0 = {k: torch.zeros(s, dtype=torch.float64) for k, s in dict(dw1=(H, K), db1=(H,), dw2=(C, H), db2=(C,)).items()}
    b = {k: (base[k].double() if base is not None else z0[k]) for k in z0}
    prod = DL[:, :, None] * h[:, None, :]                                  # [N][C][H]
    check("dw2", got["dw2"], b["dw2"] + prod.sum(0), N * U32 * (prod.abs().sum(0) + b["dw2"].abs()))
    check("db2", got["db2"], b["db2"] + DL.sum(0), N * U32 * (DL.abs().sum(0) + b["db2"].abs()))
    prod = dh[:, :, None] * pooled[:, None, :]                             # [N][H][K]
    slack = (dh_err[:, :, None] * pooled.abs()[:, None, :]).sum(0) * (1 + N * U32)
    check("dw1", got["dw1"], b["dw1"] + prod.sum(0), N * U32 * (prod.abs().sum(0) + b["dw1"].abs()) + slack)
    check("db1", got["db1"], b["db1"] + dh.sum(0), N * U32 * (dh.abs().sum(0) + b["db1"].abs()) + dh_err.sum(0) * (1 + N * U32))
    prod = dh[:, :, None] * W1[None]                                       # [N][H][K]
    dp, dp_err = prod.sum(1), H * U32 * prod.abs().sum(1) + (dh_err[:, :, None] * W1.abs()[None]).sum(1) * (1 + H * U32)
    ut = UT[dtype]
    refd = (dp / V)[:, None, :].expand(N, V, K)
    check("dact", got["dact"], refd, (ut * refd.abs() + SUBNORMAL_STEP[dtype] + (1 + ut) * (dp_err / V)[:, None, :]).expand(N, V, K))


@pytest.mark.parametrize("dtype", DT)
@pytest.mark.parametrize("C", [1, 2, 5])
@pytest.mark.parametrize("V", [1, 6, 216, 1027])
@pytest.mark.parametrize("N", [1, 3])
def test_real_layer_within_format_bounds(dev, dtype, N, V, C):
    inp = real_inputs(N, V, C, dtype, 100 * N + V + C)
    got = run(dev, dtype, *inp)
    check_real(got, *inp, dtype)
    # ... and the stages together against the head evaluated end to end in float64: the logits within the sum of the stage bounds carried forward
    ref = reference(*inp)
    w1, w2 = inp[1].double(), inp[3].double()
    e_p = U32 * ref["pooled"].abs()
    e_h = e_p @ w1.abs().t() * (1 + K * U32) + K * U32 * ((ref["pooled"].abs() + e_p) @ w1.abs().t() + inp[2].double().abs())
    e_z = e_h @ w2.abs().t() * (1 + H * U32) + H * U32 * ((ref["h"] + e_h) @ w2.abs().t() + inp[4].double().abs())
    check("logits_e2e", got["logits"], ref["logits"], e_z)


@pytest.mark.parametrize("dtype", ["f32", "f16"])
def test_zero_grads_overwrites_and_accumulate_adds(dev, dtype):
    N, V, C = 3, 70, 5                                                     # two slabs, the second ragged
    inp = real_inputs(N, V, C, dtype, 5)
    g = torch.Generator().manual_seed(6)
    base = dict(dw1=torch.randn((H, K), generator=g), db1=torch.randn((H,), generator=g), dw2=torch.randn((C, H), generator=g),
                db2=torch.randn((C,), generator=g))
    fresh = run(dev, dtype, *inp)
    over = run(dev, dtype, *inp, grads=base, zero_grads=True)
    for k in GRADS + ("dact",):
        assert torch.equal(over[k], fresh[k]), k                           # zero_grads = 1: what the buffers held is gone
    acc = run(dev, dtype, *inp, grads=base, zero_grads=False)
    check_real(acc, *inp, dtype, base=base)
    for k in GRADS:
        assert not torch.equal(acc[k], fresh[k]), k
    assert torch.equal(acc["dact"], fresh["dact"])


@pytest.mark.parametrize("dtype", DT)
def test_two_calls_agree_bit_for_bit(dev, dtype):
    inp = real_inputs(3, 1027, 5, dtype, 11)
    a, b = run(dev, dtype, *inp), run(dev, dtype, *inp)
    for k in a:
        assert torch.equal(a[k], b[k]), k


def test_bad_arguments_are_refused(dev):
    from pytorchdeeplearing_amd import _capi
    lib = _capi.lib_for(dev)
    assert lib.seg_op_cls_head_ws_bytes(0, 8) < 0 and lib.seg_op_cls_head_ws_bytes(1, 0) < 0 and lib.seg_op_cls_head_ws_bytes(1, 1 << 23) < 0
    act, w1, b1, w2, b2, dl = real_inputs(1, 2, 2, "f32", 1)
    w2big = torch.zeros((17, H))
    with pytest.raises(RuntimeError, match="c 1..16"):
        ops.cls_head_forward(dev_t(act, "f32", dev), dev_f(w1, dev), dev_f(b1, dev), dev_f(w2big, dev), dev_f(torch.zeros(17), dev), "f32")
