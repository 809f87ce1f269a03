"""Operator-level parity of the GroupNorm family (csrc/norm.hip: gn_finalize, gn_act, gn_bwd_reduce, gn_bwd_finalize, gn_bwd_apply, gn_fwd_group,
gn_bwd_group, gn_bwd_coop) and of the max-pool kernels (csrc/misc.hip) through seg_op_gn_forward / seg_op_gn_backward / seg_op_maxpool, one path at a
time, against plain torch in float64.

Two layers.  EXACT: integer data, power-of-two scales - every gate and every sum of the reduce kernels is exact in fp32, the comparison is bit for bit in
all three run dtypes.  REAL: Gaussian data (one group with mean = 30 x its standard deviation), random gamma / beta / dropout multipliers; the reference is
F.group_norm + autograd in float64 on the run dtype's own values, and every bound follows from the number formats:
    u32 = 2^-24 (half an fp32 ulp, relative), uT = 2^-11 (f16) / 2^-8 (bf16) / 2^-24 (f32): one rounding to the run dtype
  * mean, rstd, scale, shift, coef are one fp64 expression rounded once to fp32: two roundings of (nearly) the same fp64 value differ by at most one
    ulp = 2 u32, relative to the largest term of the expression;
  * out, dr: one rounding to the run dtype (uT |ref|, plus the f16 subnormal step) behind an fp32 fma chain on fp32 coefficients: 4 u32 x the sum of the
    magnitudes of the terms: |scale r| + |shift| (+ the second branch's, + |res|) for out, |A d| + |B r| + |Cc| for dr;
  * per-channel sums (Q, dgamma, dbeta, dbias): (n - 1) u32 x the sum of the magnitudes of the n addends - true for ANY summation order.
No bound was taken from a run; each check prints its largest error / bound ratio (pytest -s)."""
import functools
import math

import pytest

import conftest
import torch
import torch.nn.functional as F

from pytorchdeeplearing_amd import _capi, ops
from test_ops import cl, ints, to_dev

DT = ["f32", "f16", "bf16"]
U32 = 2.0 ** -24
UT = {"f32": 2.0 ** -24, "f16": 2.0 ** -11, "bf16": 2.0 ** -8}
SUBNORMAL_STEP = {"f32": 0.0, "f16": 2.0 ** -24, "bf16": 0.0}
MANT = {"f32": 23, "f16": 10, "bf16": 7}
EMIN = {"f32": -126, "f16": -14, "bf16": -126}
EPS = 1e-5
MARGIN = 1e-3
PAD = 16                  # mask_ld = C + PAD: a mask row is not a channel row


def rt(x, dtype):
    """round to the run dtype; returned as float64 (the run dtype's own values)"""
    return x.to(ops.TORCH_DTYPE[dtype]).double()


def dev_t(x64, dtype, dev):
    return to_dev(x64, dtype, dev)


def dev_f(x, dev, dt=torch.float32):
    return ops.aligned_like(x.to(dt).to(dev))


def channel_sums(r):
    """[N, V, C] fp64 -> [N, C, 2] = {sum r, sum r^2} (what the conv epilogues deliver)"""
    return torch.stack([r.sum(1), (r * r).sum(1)], dim=2)


def scatter(total, rep, g, integer=False):
    """[N, C, 2] -> [32, N, C, 2]: the totals spread at random over the first `rep` replicas (the others zero) so that the replicas sum to the total: a
    replica that is skipped or folded twice shows"""
    out = torch.zeros((32,) + tuple(total.shape), dtype=torch.float64)
    if rep == 1:
        out[0] = total
        return out
    shp = (rep - 1,) + tuple(total.shape)
    if integer:
        parts = torch.randint(-40, 41, shp, generator=g).double()
    else:
        parts = total * (torch.rand(shp, generator=g, dtype=torch.float64) * 1.5 - 0.5)
    last = int(torch.randint(0, rep, (1,), generator=g))
    idx = [k for k in range(rep) if k != last]
    out[idx] = parts
    out[last] = total - parts.sum(0)
    return out


RATIOS = {}


def check(name, got, ref, bound):
    """|got - ref| <= bound elementwise (bound 0: equal); prints the largest error / bound ratio"""
    err = (got.double() - ref.double()).abs()
    assert torch.isfinite(err).all(), name
    bound = bound.double().expand_as(err)
    ratio = float(torch.where(bound > 0, err / bound.clamp_min(1e-300), torch.where(err > 0, torch.full_like(err, math.inf), torch.zeros_like(err))).max())
    RATIOS[name] = max(RATIOS.get(name, 0.0), ratio)
    print("ratio %-8s %.4f" % (name, ratio))
    assert ratio <= 1.0, (name, ratio, float(err.max()))


# ------------------------------------------------------------------------------------------------------------------------------------------
# EXACT layer
# ------------------------------------------------------------------------------------------------------------------------------------------
SCALES = torch.tensor([0.0, 0.5, 1.0, 2.0])


def exact_inputs(C, N, V, nstored, vK, dual, seed):
    g = torch.Generator().manual_seed(seed)
    d = {"r": ints((N, V, C), -4, 4, g), "dys": [ints((N, V, C), -2, 2, g) for _ in range(nstored)]}
    d["scale"] = SCALES[torch.randint(0, 4, (N, C), generator=g)]
    d["shift"] = ints((N, C), -2, 2, g)
    if dual:
        d["r2"] = ints((N, V, C), -4, 4, g)
        d["scale2"] = SCALES[torch.randint(0, 4, (N, C), generator=g)]
        d["shift2"] = ints((N, C), -2, 2, g)
    dz = sum(d["dys"]) if nstored else torch.zeros((N, V, C))
    if vK:
        d["vdl"] = ints((N, vK, V), -2, 2, g)
        d["vw"] = ints((vK, C), -2, 2, g)
        dz = dz + torch.einsum("nkv,kc->nvc", d["vdl"], d["vw"])
    d["dz"] = dz.double()

    def sums(r, sc, sh):
        gate = (sc[:, None, :] * r + sh[:, None, :] > 0).double()
        return torch.stack([(d["dz"] * gate).sum(1), (d["dz"] * gate * r.double()).sum(1)], dim=2)

    d["Q"] = sums(d["r"], d["scale"], d["shift"])
    assert float(d["Q"].abs().max()) * N < 2 ** 24
    if dual:
        d["Q2"] = sums(d["r2"], d["scale2"], d["shift2"])
    d["g"] = g
    return d


def run_exact(d, dev, dtype, path, rep):
    """the backward entry on the exact inputs with identity statistics (mean 0, rstd 1, gamma 1, no mask): dbeta = sum_n Q[.., 0], dgamma = sum_n Q[.., 1]"""
    N, V, C = d["r"].shape
    ident = {"mean": dev_f(torch.zeros(N, 8), dev), "rstd": dev_f(torch.ones(N, 8), dev)}
    stats = dev_f(scatter(channel_sums(d["r"].double()), rep, d["g"], integer=True), dev, torch.float64)
    ones = dev_f(torch.ones(C), dev)
    second = None
    if "r2" in d:
        second = dict(ident, r=dev_t(d["r2"], dtype, dev), scale=dev_f(d["scale2"], dev), shift=dev_f(d["shift2"], dev),
                      stats=dev_f(scatter(channel_sums(d["r2"].double()), rep, d["g"], integer=True), dev, torch.float64), gamma=ones)
    fwd = dict(ident, scale=dev_f(d["scale"], dev), shift=dev_f(d["shift"], dev))
    return ops.gn_backward([dev_t(x, dtype, dev) for x in d["dys"]], dev_t(d["r"], dtype, dev), fwd, stats, ones, dtype, path, rep, rep,
                           vdl=dev_f(d["vdl"], dev) if "vdl" in d else None, vw=dev_f(d["vw"], dev) if "vw" in d else None, second=second)


# (stored sources, vK, second branch, C, N, V): every source variant (NDY 1 2 3; 4 5 = one-class virtual head + 0 / 1 stored; 0 = generic), DUAL on and
# off, every channel count, N = 1 and 3, and V = 37 / 300 / 2100: below one slab of rows, and never a multiple of the slab (256 / 128 / 64 / 32 / 16 rows)
EXACT_REDUCE = [
    (1, 0, False, 16, 1, 37), (2, 0, True, 16, 3, 300), (3, 0, False, 16, 1, 2100), (0, 1, True, 16, 3, 37), (1, 1, False, 16, 1, 300),
    (1, 2, True, 16, 1, 2100), (0, 4, False, 32, 3, 37), (1, 0, True, 32, 1, 300), (2, 0, False, 32, 3, 2100), (3, 0, True, 64, 1, 37),
    (1, 1, True, 64, 3, 300), (1, 0, False, 64, 1, 2100), (2, 0, False, 128, 3, 37), (0, 1, False, 128, 1, 300), (3, 0, True, 128, 1, 2100),
    (1, 0, True, 256, 3, 37), (0, 4, True, 256, 1, 300), (2, 0, False, 256, 1, 2100), (1, 2, False, 256, 3, 300),
]


@pytest.mark.parametrize("dtype", DT)
@pytest.mark.parametrize("case", EXACT_REDUCE, ids=lambda c: "s%dv%d%s-C%d-N%d-V%d" % (c[0], c[1], "dual" if c[2] else "", c[3], c[4], c[5]))
def test_reduce_exact(dev, dtype, case):
    """gn_bwd_reduce_kernel (all NDY / DUAL instantiations): Q summed over its replicas equals the fp64 sums bit for bit; so do the gamma / beta gradients
    that gn_bwd_finalize_kernel (three launches) or gn_bwd_fold_block (two launches) derive from them under identity statistics"""
    nstored, vK, dual, C, N, V = case
    i = EXACT_REDUCE.index(case)
    rep = (1, 4, 32)[i % 3]
    d = exact_inputs(C, N, V, nstored, vK, dual, 100 + i)
    o = run_exact(d, dev, dtype, ("separate", "fold")[(i // 3) % 2], rep)
    for b in ("", "2") if dual else ("",):
        q = o["Q" + b].cpu()
        assert not q[rep:].any(), "replicas beyond rep_q written"
        if V > 2 * 256 and rep > 1:
            assert q[1].any(), "one replica took everything"
        assert torch.equal(q.sum(0), d["Q" + b]), float((q.sum(0) - d["Q" + b]).abs().max())
        assert torch.equal(o["dbeta" + b].cpu().double(), d["Q" + b][..., 0].sum(0))
        assert torch.equal(o["dgamma" + b].cpu().double(), d["Q" + b][..., 1].sum(0))


# co-operative kernel (ndy, C, N, V): S = 1 / ragged S > 1 / S = 32, all three K instantiations
EXACT_COOP = [(1, 64, 1, 300), (2, 128, 3, 700), (3, 256, 1, 2100), (1, 64, 1, 7937), (2, 64, 3, 37), (3, 256, 1, 1500), (1, 128, 3, 216)]


@pytest.mark.parametrize("dtype", DT)
@pytest.mark.parametrize("case", EXACT_COOP, ids=lambda c: "s%d-C%d-N%d-V%d" % c)
def test_coop_phase1_exact(dev, dtype, case):
    """first half of gn_bwd_coop_kernel (slice loads, gate, DPP row sums, LDS, slot words): the partial sums of the S workgroups of a (sample, group)
    add up to the fp64 sums exactly - read from the slot words on the host checker, and from the published gamma / beta gradients everywhere"""
    ndy, C, N, V = case
    plan = ops.gn_coop_plan(C, V, N, dtype)
    d = exact_inputs(C, N, V, ndy, 0, False, 200 + EXACT_COOP.index(case))
    if plan is None:
        assert dtype == "f32" and (C, V) == (256, 2100)           # five chunks per thread: more than the f32 instantiations hold
        with pytest.raises(RuntimeError, match="co-operative"):
            run_exact(d, dev, dtype, "coop", 4)
        return
    S, ku = plan
    o = run_exact(d, dev, dtype, "coop", 4)
    assert torch.equal(o["dbeta"].cpu().double(), d["Q"][..., 0].sum(0))
    assert torch.equal(o["dgamma"].cpu().double(), d["Q"][..., 1].sum(0))
    if dev.type == "cpu":
        cpg = C // 8
        w = o["Q"].cpu().view(torch.float32).flatten()[:N * 8 * S * cpg * 2].view(N, 8, S, cpg, 2).double()
        assert torch.equal(w.sum(2).reshape(N, C, 2) + 0.0, d["Q"])


def exact_params(g, C, N):
    """gamma / beta multiples of 1/4, dropout multipliers 0 / 1 / 2 in a padded mask, per-group integer mean and power-of-two rstd"""
    gamma, beta = ints((C,), -4, 4, g) / 4, ints((C,), -8, 8, g) / 4
    mask = torch.full((N, C + PAD), 7.0)
    mask[:, :C] = ints((N, C), 0, 2, g)
    mean = ints((N, 8), -3, 3, g)
    rstd = torch.tensor([0.25, 0.5, 1.0, 2.0])[torch.randint(0, 4, (N, 8), generator=g)]
    return gamma, beta, mask, mean, rstd


@pytest.mark.parametrize("dtype", DT)
def test_paths_agree_exactly(dev, dtype):
    """Every path computes the same coefficients from the same sums.  Inputs on which every fp64 intermediate of the coefficient formulas is exact (small
    integers, multiples of 1/4, powers of two; Mg = 2048; N = 1: one addend per parameter gradient): mean / rstd / scale / shift and coef / dgamma / dbeta /
    dbias equal the formulas evaluated in float64 and rounded to fp32, with tolerance 0, on every path; out and dr are bit-identical across the paths and
    within the format bounds of the module docstring of the float64 reference."""
    C, N, V, rep = 64, 1, 256, 4
    cpg, Mg = C // 8, float(C // 8 * V)
    assert ops.gn_group_eligible(C, V, dtype) and ops.gn_coop_plan(C, V, N, dtype) is not None
    g = torch.Generator().manual_seed(77)
    rep8 = lambda t: t.double().repeat_interleave(cpg, dim=1)
    grp = lambda t: rep8(t.reshape(N, 8, cpg).sum(2))
    f32 = lambda t: t.float().double()
    bits = lambda t: t.cpu().contiguous().view(torch.uint8)
    r = ints((N, V, C), -4, 4, g).double()
    rd = dev_t(r, dtype, dev)

    # ---- backward: statistics as given (not those of r), Q computed by the entry from integer data
    gamma, beta, mask, mean, rstd = exact_params(g, C, N)
    mk, ga, mu, rs = mask[:, :C].double(), gamma.double()[None, :], rep8(mean), rep8(rstd)
    scale, shift = mk * ga * rs, mk * (beta.double()[None, :] - ga * mu * rs)
    dys = [ints((N, V, C), -2, 2, g).double() for _ in range(2)]
    dz = (dys[0] + dys[1]) * (scale[:, None, :] * r + shift[:, None, :] > 0)
    Q1, Q2, R1 = dz.sum(1), (dz * r).sum(1), r.sum(1)
    q1 = mk * Q1
    qx = (mk * Q2 - mu * q1) * rs
    S1, S2 = grp(ga * q1), grp(ga * qx)
    A, B, Cc = rs * ga * mk, -rs * rs * S2 / Mg, -rs * S1 / Mg + rs * rs * S2 * mu / Mg
    want = {"dbeta": q1.sum(0), "dgamma": qx.sum(0), "dbias": (A * Q1 + B * R1 + Cc * float(V)).sum(0), "coef": torch.stack([A, B, Cc], dim=2)}
    dr = A[:, None, :] * dz + B[:, None, :] * r + Cc[:, None, :]
    dr_terms = (A[:, None, :] * dz).abs() + (B[:, None, :] * r).abs() + Cc.abs()[:, None, :]
    fwd = dict(scale=dev_f(scale, dev), shift=dev_f(shift, dev), mean=dev_f(mean, dev), rstd=dev_f(rstd, dev))
    stats = dev_f(scatter(channel_sums(r), rep, g, integer=True), dev, torch.float64)
    first = None
    for path in ("separate", "fold", "group", "coop"):
        o = ops.gn_backward([dev_t(x, dtype, dev) for x in dys], rd, fwd, stats, dev_f(gamma, dev), dtype, path, rep, rep, mask=dev_f(mask, dev))
        for k in ("dbeta", "dgamma", "dbias") + (("coef",) if path in ("separate", "fold") else ()):
            print("%s %s largest difference %g" % (path, k, float((o[k].cpu().double() - f32(want[k])).abs().max())))
            assert torch.equal(o[k].cpu().double(), f32(want[k])), (path, k)
        if path in ("separate", "fold"):
            assert torch.equal(o["Q"].cpu().sum(0), torch.stack([Q1, Q2], dim=2)), path
        check("dr", o["dr"].cpu(), dr, UT[dtype] * dr.abs() + 4 * U32 * dr_terms + SUBNORMAL_STEP[dtype])
        first = first if first is not None else bits(o["dr"])
        assert torch.equal(bits(o["dr"]), first), path

    # ---- forward: eps = 0 and synthetic channel sums whose group moments are an integer mean and a variance in {1/4, 1, 4, 16}
    gamma, beta, mask, mean, rstd = exact_params(g, C, N)
    mk, ga = mask[:, :C].double(), gamma.double()[None, :]
    var = 1.0 / (rstd.double() * rstd.double())
    tot = torch.stack([mean.double() * Mg, (var + mean.double() ** 2) * Mg], dim=2)             # [N, 8, 2]: group sums, integers
    st = ints((N, 8, cpg, 2), -1000, 1000, g).double()
    st[:, :, cpg - 1] = tot - st[:, :, :cpg - 1].sum(2)
    stats = dev_f(scatter(st.reshape(N, C, 2), rep, g, integer=True), dev, torch.float64)
    scale, shift = mk * ga * rep8(rstd), mk * (beta.double()[None, :] - ga * rep8(mean) * rep8(rstd))
    want = {"mean1": mean, "rstd1": rstd, "scale1": scale, "shift1": shift}
    out = torch.relu(scale[:, None, :] * r + shift[:, None, :])
    terms = (scale[:, None, :] * r).abs() + shift.abs()[:, None, :]
    first = None
    for path in ("finalize", "fold", "group"):
        o = ops.gn_forward(rd, stats, dev_f(gamma, dev), dev_f(beta, dev), dtype, path, rep, mask1=dev_f(mask, dev), eps=0.0)
        for k in want:
            print("%s %s largest difference %g" % (path, k, float((o[k].cpu().double() - f32(want[k])).abs().max())))
            assert torch.equal(o[k].cpu().double(), f32(want[k])), (path, k)
        check("out", o["out"].cpu(), out, UT[dtype] * out.abs() + 4 * U32 * terms + SUBNORMAL_STEP[dtype])
        first = first if first is not None else bits(o["out"])
        assert torch.equal(bits(o["out"]), first), path


POOL_WINDOWS = [(2, 2, 2), (1, 2, 2), (1, 1, 1)]


@pytest.mark.parametrize("dtype", DT)
@pytest.mark.parametrize("C", [16, 64])
@pytest.mark.parametrize("window", POOL_WINDOWS, ids=lambda w: "%dx%dx%d" % w)
def test_maxpool_exact(dev, dtype, C, window):
    """maxpool_fwd_kernel / maxpool_bwd_kernel against F.max_pool3d / F.max_pool2d and their autograd on data full of ties: post-ReLU zeros, whole windows
    equal, negative-only windows - the gradient lands on the FIRST maximum in (d, h, w) scan order"""
    g = torch.Generator().manual_seed(C + sum(window))
    N, D, H, W = 2, 4, 6, 8
    x = torch.relu(ints((N, C, D, H, W), -3, 2, g))             # two thirds zeros
    x[:, :, :2, :2, :] = 2.0                                     # whole windows equal
    x[:, :, 2:, 4:, :4] = ints((N, C, 2, 2, 4), -3, -1, g)       # negative-only windows (with ties)
    x = x.requires_grad_(True)
    if window[0] == 1:
        ref = F.max_pool2d(x.transpose(1, 2).reshape(N * D, C, H, W), window[1:]).reshape(N, D, C, H // window[1], W // window[2]).transpose(1, 2)
    else:
        ref = F.max_pool3d(x, window)
    dy = ints(tuple(ref.shape), -3, 3, g)
    dy[dy == 0] = 1.0                                            # a gradient on a wrong element must show
    ref.backward(dy)
    xd = to_dev(cl(x.detach()), dtype, dev)
    out = ops.maxpool(xd, window, dtype)
    assert torch.equal(out.float().cpu(), cl(ref.detach()))
    din = ops.maxpool(xd, window, dtype, dout=to_dev(cl(dy), dtype, dev))
    assert torch.equal(din.float().cpu(), cl(x.grad))


# ------------------------------------------------------------------------------------------------------------------------------------------
# REAL-valued layer
# ------------------------------------------------------------------------------------------------------------------------------------------
def spacing(x, dtype):
    e = torch.floor(torch.log2(x.abs().clamp_min(2.0 ** EMIN[dtype]))).clamp_min(EMIN[dtype])
    return torch.pow(torch.tensor(2.0, dtype=torch.float64), e - MANT[dtype])


def group_moments(r):
    """[N, V, C] fp64 -> mean, var [N, 8] (two-pass, biased variance)"""
    N, V, C = r.shape
    x = r.reshape(N, V, 8, C // 8)
    mean = x.mean(dim=(1, 3))
    var = ((x - mean[:, None, :, None]) ** 2).mean(dim=(1, 3))
    return mean, var


def pre_activation(r, gamma, beta, mk):
    """fp64 scale, shift [N, C] and scale * r + shift"""
    C = r.shape[2]
    mean, var = group_moments(r)
    rstd = 1.0 / torch.sqrt(var + EPS)
    scale = mk * gamma[None, :] * rstd.repeat_interleave(C // 8, dim=1)
    shift = mk * (beta[None, :] - gamma[None, :] * (mean * rstd).repeat_interleave(C // 8, dim=1))
    return scale, shift, scale[:, None, :] * r + shift[:, None, :]


def clear_margin(r, gamma, beta, mk, dtype):
    """move the elements of r whose pre-activation lies within the margin of zero to the nearest run-dtype value that clears it (the statistics move with
    them: iterate).  Channels with multiplier 0 have scale = shift = 0: their pre-activation is exactly 0 on both sides and their gate is shut on both."""
    live = (mk != 0)[:, None, :]
    for _ in range(40):
        scale, shift, pre = pre_activation(r, gamma, beta, mk)
        bad = live & (pre.abs() < 2 * MARGIN)
        if not bad.any():
            break
        sgn = torch.where(pre >= 0, 1.0, -1.0).double()
        step = (sgn * 3 * MARGIN - pre) / torch.where(scale == 0, torch.ones_like(scale), scale)[:, None, :]
        cand = rt(r + step, dtype)
        stuck = cand == r
        cand = torch.where(stuck, rt(r + torch.sign(step) * spacing(r, dtype), dtype), cand)
        r = torch.where(bad, cand, r)
    return r


def margin_violations(r, gamma, beta, mk):
    _, _, pre = pre_activation(r, gamma, beta, mk)
    return int((((mk != 0)[:, None, :]) & (pre.abs() < MARGIN)).sum())


class Branch:
    pass


def make_branch(g, dtype, C, N, V, drop):
    b = Branch()
    cpg = C // 8
    # Conditioning of the inputs, decided from the bound and not from a run.  The dr bound asks for B and Cc to a few u32 of THEMSELVES; B and Cc are fp64
    # expressions of the group sums S1 = sum gamma dz and S2 = sum gamma dz xhat, which the kernels accumulate in fp32 inside a thread: good to a few u32 of
    # the sum of the MAGNITUDES of their addends.  On sums that cancel the check would measure the inputs.  So: gradients with a non-zero mean (real_case),
    # one sign of gamma per group (groups 2 and 5 negative: S1 has that sign, S2 is positive), and a group mean of the opposite sign (per-group offset, small
    # per-channel spread), so that the two terms of Cc = -rs S1 / Mg + rs^2 S2 mu / Mg have one sign - except group 1, whose second term is 24 x the first
    sign = torch.ones(8)
    sign[2] = sign[5] = -1.0
    goff = -sign.double() * (0.5 + 2.5 * torch.rand(8, generator=g, dtype=torch.float64))
    off = goff.repeat_interleave(cpg) + 0.3 * torch.randn(C, generator=g, dtype=torch.float64)
    sd = torch.rand(C, generator=g, dtype=torch.float64) * 1.5 + 0.5
    off[cpg:2 * cpg] = 30.0                       # group 1: mean = 30 x standard deviation (E[x^2] - mean^2 loses 3 digits)
    sd[cpg:2 * cpg] = 1.0
    b.gamma = (torch.rand(C, generator=g) + 0.5) * sign.repeat_interleave(cpg)
    b.beta = torch.randn(C, generator=g) * 0.5
    b.mask = torch.full((N, C + PAD), 7.0)       # (the padding columns hold something a wrong stride would pick up)
    b.mask[:, :C] = torch.where(torch.rand(N, C, generator=g) < 0.2, 0.0, 1.25) if drop else 1.25
    if drop:
        b.mask[0, 2 * cpg] = 0.0
    b.mk = b.mask[:, :C].double()
    r = rt(off + sd * torch.randn(N, V, C, generator=g, dtype=torch.float64), dtype)
    b.r = clear_margin(r, b.gamma.double(), b.beta.double(), b.mk, dtype)
    b.stats = channel_sums(b.r)
    return b


@functools.lru_cache(maxsize=2)
def real_case(dtype, C, N, V, dual, res, ndy, vK):
    """inputs and the float64 reference (F.group_norm -> multiplier -> relu -> sum of branches + residual; gradients from autograd), computed once per case"""
    g = torch.Generator().manual_seed(C * 7 + N * 3 + V)
    c = Branch()
    c.dtype, c.C, c.N, c.V = dtype, C, N, V
    c.br = [make_branch(g, dtype, C, N, V, True)] + ([make_branch(g, dtype, C, N, V, True)] if dual else [])
    c.res = rt(torch.randn(N, V, C, generator=g, dtype=torch.float64), dtype) if res else None
    c.dys = [rt(0.5 + 0.5 * torch.randn(N, V, C, generator=g, dtype=torch.float64), dtype) for _ in range(ndy)]
    c.vdl = 0.5 + 0.5 * torch.randn(N, vK, V, generator=g) if vK else None
    c.vw = 0.5 + torch.rand(vK, C, generator=g) if vK else None
    src = list(c.dys) + ([c.vdl.double()[:, k, :, None] * c.vw.double()[k][None, None, :] for k in range(vK)] if vK else [])
    c.dsum, c.dabs, c.nsrc = sum(src), sum(s.abs() for s in src), len(src)
    out = 0.0
    for b in c.br:
        b.rg = b.r.clone().requires_grad_(True)
        b.gg, b.bg = b.gamma.double().requires_grad_(True), b.beta.double().requires_grad_(True)
        y = F.group_norm(b.rg.permute(0, 2, 1), 8, b.gg, b.bg, EPS) * b.mk[:, :, None]
        out = out + torch.relu(y)
    if res:
        out = out + c.res.permute(0, 2, 1)
    out.backward(c.dsum.permute(0, 2, 1))
    c.out = out.detach().permute(0, 2, 1)
    Mg = float(C // 8 * V)
    rep8 = lambda t: t.repeat_interleave(C // 8, dim=1)
    grp = lambda t: t.reshape(N, 8, C // 8).sum(2)
    for b in c.br:
        b.dr, b.dgamma, b.dbeta = b.rg.grad, b.gg.grad, b.bg.grad
        b.dbias = b.dr.sum(dim=(0, 1))
        # the same quantities term by term (for the bounds), checked against autograd
        b.mean, var = group_moments(b.r)
        b.rstd = 1.0 / torch.sqrt(var + EPS)
        b.scale, b.shift, pre = pre_activation(b.r, b.gamma.double(), b.beta.double(), b.mk)
        b.gate = (pre > 0).double()
        b.Q = torch.stack([(c.dsum * b.gate).sum(1), (c.dsum * b.gate * b.r).sum(1)], dim=2)
        b.Qabs = torch.stack([(c.dabs * b.gate).sum(1), (c.dabs * b.gate * b.r.abs()).sum(1)], dim=2)
        ga, mu, rs = b.gamma.double()[None, :], rep8(b.mean), rep8(b.rstd)
        q1 = b.mk * b.Q[..., 0]
        qx = (b.mk * b.Q[..., 1] - mu * q1) * rs
        S1, S2 = rep8(grp(ga * q1)), rep8(grp(ga * qx))
        b.A, b.B, b.Cc = rs * ga * b.mk, -rs * rs * S2 / Mg, -rs * S1 / Mg + rs * rs * S2 * mu / Mg
        dr = b.A[:, None, :] * c.dsum * b.gate + b.B[:, None, :] * b.r + b.Cc[:, None, :]
        assert float((dr - b.dr).abs().max()) <= 1e-9 * float(b.dr.abs().max())
        assert float((qx.sum(0) - b.dgamma).abs().max()) <= 1e-9 * float(b.dgamma.abs().max() + 1)
        # sums of term magnitudes
        b.dr_terms = (b.A[:, None, :] * c.dsum * b.gate).abs() + (b.B[:, None, :] * b.r).abs() + b.Cc.abs()[:, None, :]
        b.dbeta_terms = (b.mk * b.Qabs[..., 0]).sum(0)
        b.dgamma_terms = ((b.mk * b.Qabs[..., 1] + mu.abs() * b.mk * b.Qabs[..., 0]) * rs).sum(0)
        b.dbias_terms = b.dr_terms.sum(dim=(0, 1))
    return c


def check_forward(c, o, path, strict=True):
    dtype, C = c.dtype, c.C
    terms = 0.0
    for i, b in enumerate(c.br):
        k = str(i + 1)
        f32 = lambda t: t.float().double()
        check("mean", o["mean" + k].cpu(), f32(b.mean), 2 * U32 * b.mean.abs() + 2.0 ** -45 * b.r.abs().mean())
        check("rstd", o["rstd" + k].cpu(), f32(b.rstd), 2 * U32 * b.rstd)
        check("scale", o["scale" + k].cpu(), f32(b.scale), 2 * U32 * b.scale.abs())
        big = torch.maximum((b.mk * b.beta.double()[None, :]).abs(), (b.scale * b.mean.repeat_interleave(C // 8, dim=1)).abs())
        check("shift", o["shift" + k].cpu(), f32(b.shift), 2 * U32 * big)
        dropped = b.mk == 0
        assert not o["scale" + k].cpu()[dropped].any() and not o["shift" + k].cpu()[dropped].any()       # shut gates: exactly zero
        terms = terms + (b.scale[:, None, :] * b.r).abs() + b.shift.abs()[:, None, :]
    if c.res is not None:
        terms = terms + c.res.abs()
    check("out", o["out"].cpu(), c.out, UT[dtype] * c.out.abs() + 4 * U32 * terms + SUBNORMAL_STEP[dtype])


def sum_bound(n, terms):
    return (n - 1) * U32 * terms


def coef_reference(b, c, Qtot, stats_tot, mean_f, rstd_f):
    """gn_bwd_finalize's expressions in fp64 on the entry's own inputs (fp32 mean / rstd, the Q it was handed): A, B, Cc and the two terms of Cc"""
    C, N, V = c.C, c.N, c.V
    Mg = float(C // 8 * V)
    rep8 = lambda t: t.repeat_interleave(C // 8, dim=1)
    grp = lambda t: t.reshape(N, 8, C // 8).sum(2)
    ga, mu, rs = b.gamma.double()[None, :], rep8(mean_f.double()), rep8(rstd_f.double())
    q1 = b.mk * Qtot[..., 0]
    qx = (b.mk * Qtot[..., 1] - mu * q1) * rs
    S1, S2 = rep8(grp(ga * q1)), rep8(grp(ga * qx))
    t1, t2 = -rs * S1 / Mg, rs * rs * S2 * mu / Mg
    return rs * ga * b.mk, -rs * rs * S2 / Mg, t1 + t2, torch.maximum(t1.abs(), t2.abs())


def check_backward(c, o, path, fwd_host, S=None):
    dtype, C, N, V = c.dtype, c.C, c.N, c.V
    for i, b in enumerate(c.br):
        k = "" if i == 0 else "2"
        check("dr", o["dr" + k].cpu(), b.dr, UT[dtype] * b.dr.abs() + 4 * U32 * b.dr_terms + SUBNORMAL_STEP[dtype])
        check("dbeta", o["dbeta" + k].cpu(), b.dbeta, sum_bound(N * V * c.nsrc, b.dbeta_terms))
        check("dgamma", o["dgamma" + k].cpu(), b.dgamma, sum_bound(2 * N * V * c.nsrc, b.dgamma_terms))
        check("dbias", o["dbias" + k].cpu(), b.dbias, sum_bound(N * V * (c.nsrc + 2), b.dbias_terms))
        if path in ("separate", "fold"):
            Qtot = o["Q" + k].cpu().sum(0)
            check("Q", Qtot, b.Q, sum_bound(V * c.nsrc, b.Qabs))
            A, B, Cc, Cbig = coef_reference(b, c, Qtot, b.stats, fwd_host[i]["mean"], fwd_host[i]["rstd"])
            co = o["coef" + k].cpu()
            f32 = lambda t: t.float().double()
            check("coef", co[..., 0], f32(A), 2 * U32 * A.abs())
            check("coef", co[..., 1], f32(B), 2 * U32 * B.abs())
            check("coef", co[..., 2], f32(Cc), 2 * U32 * Cbig)
        elif path == "coop":
            cpg = C // 8
            w = o["Q"].cpu().view(torch.float32).flatten()[:N * 8 * S * cpg * 2].view(N, 8, S, cpg, 2).double()
            check("Q", w.sum(2).reshape(N, C, 2), b.Q, sum_bound(V * c.nsrc, b.Qabs))


def upload(c, dev, rep, g):
    dtype = c.dtype
    u = Branch()
    u.br = []
    for b in c.br:
        u.br.append(dict(r=dev_t(b.r, dtype, dev), stats=dev_f(scatter(b.stats, rep, g), dev, torch.float64), gamma=dev_f(b.gamma, dev),
                         beta=dev_f(b.beta, dev), mask=dev_f(b.mask, dev)))
    u.res = dev_t(c.res, dtype, dev) if c.res is not None else None
    u.dys = [dev_t(x, dtype, dev) for x in c.dys]
    u.vdl = dev_f(c.vdl, dev) if c.vdl is not None else None
    u.vw = dev_f(c.vw, dev) if c.vw is not None else None
    return u


def forward(c, u, path, rep):
    a, b2 = u.br[0], (u.br[1] if len(u.br) > 1 else None)
    kw = dict(r2=b2["r"], stats2=b2["stats"], gamma2=b2["gamma"], beta2=b2["beta"], mask2=b2["mask"]) if b2 else {}
    return ops.gn_forward(a["r"], a["stats"], a["gamma"], a["beta"], c.dtype, path, rep, mask1=a["mask"], res=u.res, eps=EPS, **kw)


def backward(c, u, fo, path, rep_q, rep_s, bufs=None):
    a = u.br[0]
    fwd = {k: fo[k + "1"] for k in ("scale", "shift", "mean", "rstd")}
    second = None
    if len(u.br) > 1:
        b2 = u.br[1]
        second = dict({k: fo[k + "2"] for k in ("scale", "shift", "mean", "rstd")}, r=b2["r"], stats=b2["stats"], gamma=b2["gamma"], mask=b2["mask"])
    return ops.gn_backward(u.dys, a["r"], fwd, a["stats"], a["gamma"], c.dtype, path, rep_q, rep_s, mask=a["mask"], vdl=u.vdl, vw=u.vw, second=second,
                           bufs=bufs)


# C, N, V, second branch, residual, stored sources, vK of a virtual source
REAL = {
    "coop-S2": (64, 1, 300, False, True, 1, 0),                # co-operative S = 2, ku = 1, ragged last slice
    "coop-N3": (128, 3, 700, False, False, 2, 0),
    "coop-K8": (256, 1, 2100, False, True, 1, 0),              # 16-bit: ku = 5 (K = 8), S = 7, ragged; f32: not eligible
    "coop-K4": (256, 1, 1500, False, False, 3, 0),             # ku = 3 (K = 4)
    "coop-S32": (64, 1, 7937, False, False, 1, 0),             # S at its cap, one item in the last slice
    "coop-bench": (64, 4, 13824, False, True, 2, 0),           # the benchmark's 24^3 level: ku = 7 in 16 bits
    "group-216": (64, 1, 216, False, True, 1, 0),              # one workgroup per group (and co-operative S = 1)
    "group-37": (64, 3, 37, False, False, 2, 0),
    "group-C256": (256, 2, 36, False, True, 3, 0),
    "group-edge": (64, 1, 1024, False, False, 1, 0),           # the largest f16 tensor the group form takes
    "fold-16-dual": (16, 3, 300, True, True, 1, 1),            # fold and separate forms; r2 + res; one-class virtual source + a stored one
    "fold-16-res": (16, 1, 4096, False, True, 0, 2),           # res only; generic virtual source alone
    "fold-32": (32, 3, 300, False, False, 2, 0),               # neither
    "fold-32-dual": (32, 1, 4096, True, True, 1, 0),
}


def real_params():
    out = []
    for name, shp in REAL.items():
        big = shp[0] * shp[1] * shp[2] > 400000
        for dtype in (["f16"] if name == "coop-bench" else DT):
            for rep in ([4] if big else [1, 4, 32]):
                out.append(pytest.param(name, dtype, rep, id="%s-%s-rep%d" % (name, dtype, rep)))
    return out


@pytest.mark.parametrize("name,dtype,rep", real_params())
def test_real_valued(dev, name, dtype, rep):
    """every forward and backward path the shape is eligible for, on the same inputs, against the float64 reference within the format bounds of the module
    docstring; the paths against one another; on the host checker a second call of every backward path bit-identical to the first"""
    C, N, V, dual, res, ndy, vK = REAL[name]
    if C * N * V > 600000:
        conftest.checker_slow(dev, "%d k elements on the host checker" % (C * N * V // 1000))
    c = real_case(dtype, C, N, V, dual, res, ndy, vK)
    for b in c.br:
        assert margin_violations(b.r, b.gamma.double(), b.beta.double(), b.mk) == 0
        assert float(b.mean[:, 1].abs().min() * b.rstd[:, 1].max()) > 20          # the ill-conditioned group is there
    u = upload(c, dev, rep, torch.Generator().manual_seed(rep))
    group_ok = ops.gn_group_eligible(C, V, dtype)
    plan = ops.gn_coop_plan(C, V, N, dtype)
    fpaths = ["finalize", "fold"] + (["group"] if group_ok and not dual else [])
    fo = None
    for p in fpaths:
        o = forward(c, u, p, rep)
        check_forward(c, o, p)
        fo = fo or o
    fwd_host = [{k: fo[k + str(i + 1)].cpu() for k in ("mean", "rstd")} for i in range(len(c.br))]
    bpaths = ["separate", "fold"] + (["group"] if group_ok and not dual and not vK else []) + (["coop"] if plan and not dual and not vK else [])
    got = {}
    for p in bpaths:
        got[p] = backward(c, u, fo, p, rep, rep)
        check_backward(c, got[p], p, fwd_host, S=plan[0] if plan else None)
        if dev.type == "cpu":
            again = backward(c, u, fo, p, rep, rep)
            for k in got[p]:
                assert torch.equal(got[p][k].cpu().view(torch.uint8), again[k].cpu().view(torch.uint8)), (p, k)
    # path against path: each within its bound of the reference, so any two within the sum of their bounds
    for i, b in enumerate(c.br):
        k = "" if i == 0 else "2"
        bd = UT[dtype] * b.dr.abs() + 4 * U32 * b.dr_terms + SUBNORMAL_STEP[dtype]
        for p in bpaths[1:]:
            check("dr-x", got[p]["dr" + k].cpu(), got[bpaths[0]]["dr" + k].cpu(), 2 * bd)
            check("dgam-x", got[p]["dgamma" + k].cpu(), got[bpaths[0]]["dgamma" + k].cpu(), 2 * sum_bound(2 * N * V * c.nsrc, b.dgamma_terms))
            check("dbet-x", got[p]["dbeta" + k].cpu(), got[bpaths[0]]["dbeta" + k].cpu(), 2 * sum_bound(N * V * c.nsrc, b.dbeta_terms))
            check("dbia-x", got[p]["dbias" + k].cpu(), got[bpaths[0]]["dbias" + k].cpu(), 2 * sum_bound(N * V * (c.nsrc + 2), b.dbias_terms))


def test_shapes_reach_every_instantiation(dev):
    """what the cases above rely on, asked from the library's own plan and eligibility functions (not from a hand-computed list)"""
    plan = lambda name, dtype: ops.gn_coop_plan(*[REAL[name][i] for i in (0, 2, 1)], dtype)
    ragged = lambda name, dtype: (REAL[name][2] * (REAL[name][0] // 64)) % (plan(name, dtype)[1] * 256) != 0
    for dtype in DT:
        assert plan("coop-S2", dtype) == (2, 1) and ragged("coop-S2", dtype)
        S, ku = plan("coop-N3", dtype)
        assert S > 1 and ku <= 2 and ragged("coop-N3", dtype)
        S, ku = plan("coop-K4", dtype)
        assert 2 < ku <= 4 and S > 1
        assert plan("coop-S32", dtype)[0] == 32 and ragged("coop-S32", dtype)
        assert plan("group-216", dtype)[0] == 1 and plan("group-37", dtype)[0] == 1
        for name in ("group-216", "group-37", "group-C256"):
            assert ops.gn_group_eligible(REAL[name][0], REAL[name][2], dtype)
        for name in ("fold-16-dual", "fold-16-res", "fold-32", "fold-32-dual"):
            assert plan(name, dtype) is None and not ops.gn_group_eligible(REAL[name][0], REAL[name][2], dtype)
    for dtype in ("f16", "bf16"):
        S, ku = plan("coop-K8", dtype)
        assert ku > 4 and S == 7 and ragged("coop-K8", dtype)
    assert plan("coop-K8", "f32") is None                         # five chunks per thread do not fit the f32 instantiations, and S is at its cap
    S, ku = plan("coop-bench", "f16")
    assert ku == 7 and S == 8
    # the edge of the one-workgroup-per-group form: 128 KB per sample
    assert ops.gn_group_eligible(64, 1024, "f16") and not ops.gn_group_eligible(64, 1025, "f16")
    assert ops.gn_group_eligible(64, 512, "f32") and not ops.gn_group_eligible(64, 513, "f32")
    assert not ops.gn_group_eligible(32, 64, "f16")


# ------------------------------------------------------------------------------------------------------------------------------------------
# refusals
# ------------------------------------------------------------------------------------------------------------------------------------------
def poisoned(dev, dtype, N, V, C, second=False):
    b = {}
    for s in ("", "2") if second else ("",):
        b["Q" + s] = dev_f(torch.full((32, N, C, 2), 7.0), dev, torch.float64)
        b["coef" + s] = dev_f(torch.full((N, C, 3), 7.0), dev)
        b["dr" + s] = to_dev(torch.full((N, V, C), 7.0), dtype, dev)
        for k in ("dgamma", "dbeta", "dbias"):
            b[k + s] = dev_f(torch.full((C,), 7.0), dev)
    return b


def refused_bwd(dev, dtype, match, C, N, V, path, rep_q=4, rep_s=4, dual=False, virt=False, drop=None):
    """the backward entry reports `match` and leaves its output buffers as they were"""
    z = lambda *s: dev_f(torch.zeros(*s), dev)
    r = to_dev(torch.zeros(N, V, C), dtype, dev)
    fwd = dict(scale=z(N, C), shift=z(N, C), mean=z(N, 8), rstd=z(N, 8))
    stats = dev_f(torch.zeros(32, N, C, 2), dev, torch.float64)
    second = dict(fwd, r=r, stats=stats, gamma=z(C)) if dual else None
    bufs = poisoned(dev, dtype, N, V, C, dual)
    if drop:
        bufs[drop] = None
    gamma = None if drop == "gamma" else z(C)
    with pytest.raises(RuntimeError, match=match):
        ops.gn_backward([r], r, fwd, stats, gamma, dtype, path, rep_q, rep_s, vdl=z(N, 1, V) if virt else None, vw=z(1, C) if virt else None,
                        second=second, bufs=bufs)
    for k, t in bufs.items():
        if t is not None:
            assert bool((t.float() == 7.0).all()), k


def test_refusals_backward(dev):
    refused_bwd(dev, "f16", "co-operative", 64, 1, 300, "coop", virt=True)
    refused_bwd(dev, "f16", "co-operative", 64, 1, 300, "coop", dual=True)
    refused_bwd(dev, "f32", "co-operative", 256, 1, 2100, "coop")              # no plan within K = 4
    refused_bwd(dev, "f16", "co-operative", 32, 1, 300, "coop")
    refused_bwd(dev, "f16", "one-workgroup-per-group", 64, 1, 1025, "group")   # above 128 KB
    refused_bwd(dev, "f32", "one-workgroup-per-group", 64, 1, 513, "group")
    refused_bwd(dev, "f16", "one-workgroup-per-group", 32, 1, 64, "group")
    refused_bwd(dev, "f16", "one-workgroup-per-group", 64, 1, 64, "group", dual=True)
    refused_bwd(dev, "f16", "one-workgroup-per-group", 64, 1, 64, "group", virt=True)
    for C in (8, 24, 48, 512):
        for path in ("separate", "fold", "group", "coop"):
            refused_bwd(dev, "f16", "C must be", C, 1, 40, path)
    for rq, rs in ((0, 4), (33, 4), (4, 0), (4, 33), (-1, 4)):
        refused_bwd(dev, "f32", "rep_q / rep_s", 16, 1, 40, "fold", rep_q=rq, rep_s=rs)
    for drop in ("gamma", "Q", "dr", "dgamma", "dbeta"):
        refused_bwd(dev, "f32", "null pointer", 16, 1, 40, "fold", drop=drop)
    refused_bwd(dev, "f32", "null pointer", 16, 1, 40, "separate", drop="coef")
    refused_bwd(dev, "f32", "null pointer", 16, 1, 40, "fold", dual=True, drop="dr2")
    refused_bwd(dev, "f32", "unknown path", 16, 1, 40, 4)


def refused_fwd(dev, dtype, match, C, N, V, path, rep=4, dual=False, drop=None):
    z = lambda *s: dev_f(torch.zeros(*s), dev)
    r = to_dev(torch.zeros(N, V, C), dtype, dev)
    stats = dev_f(torch.zeros(32, N, C, 2), dev, torch.float64)
    bufs = {"out": to_dev(torch.full((N, V, C), 7.0), dtype, dev)}
    for s in ("1", "2") if dual else ("1",):
        bufs.update({"scale" + s: dev_f(torch.full((N, C), 7.0), dev), "shift" + s: dev_f(torch.full((N, C), 7.0), dev),
                     "mean" + s: dev_f(torch.full((N, 8), 7.0), dev), "rstd" + s: dev_f(torch.full((N, 8), 7.0), dev)})
    if drop in bufs:
        bufs[drop] = None
    kw = dict(r2=r, stats2=stats, gamma2=z(C), beta2=z(C)) if dual else {}
    with pytest.raises(RuntimeError, match=match):
        ops.gn_forward(r, None if drop == "stats" else stats, z(C), None if drop == "beta" else z(C), dtype, path, rep, bufs=bufs, **kw)
    for k, t in bufs.items():
        if t is not None:
            assert bool((t.float() == 7.0).all()), k


def test_refusals_forward(dev):
    refused_fwd(dev, "f16", "one-workgroup-per-group", 64, 1, 1025, "group")
    refused_fwd(dev, "f16", "one-workgroup-per-group", 32, 1, 64, "group")
    refused_fwd(dev, "f16", "second branch", 64, 1, 64, "group", dual=True)
    for C in (8, 24, 48, 512):
        for path in ("finalize", "fold", "group"):
            refused_fwd(dev, "bf16", "C must be", C, 1, 40, path)
    for rep in (0, 33, -4):
        refused_fwd(dev, "f32", "rep must be", 16, 1, 40, "fold", rep=rep)
    for drop in ("stats", "beta", "out", "scale1", "rstd1"):
        refused_fwd(dev, "f32", "null pointer", 16, 1, 40, "finalize", drop=drop)
    refused_fwd(dev, "f32", "null pointer", 16, 1, 40, "fold", dual=True, drop="mean2")
    refused_fwd(dev, "f32", "unknown path", 16, 1, 40, 3)


def test_refusals_maxpool(dev):
    lib = _capi.lib_for(dev)
    x = to_dev(torch.zeros(1, 4, 6, 8, 16), "f16", dev)
    out = to_dev(torch.full((1, 4, 6, 8, 16), 7.0), "f16", dev)
    st = _capi.stream_for(dev)
    for args in ((x.data_ptr(), None, None, None, 1, 4, 6, 8, 16, 2, 2, 2, 0),             # no output
                 (x.data_ptr(), out.data_ptr(), None, None, 1, 4, 6, 8, 16, 2, 2, 2, 1),   # backward without gradients
                 (x.data_ptr(), out.data_ptr(), None, None, 1, 4, 6, 8, 12, 2, 2, 2, 0),   # channels not in chunks of 8
                 (x.data_ptr(), out.data_ptr(), None, None, 1, 4, 6, 8, 16, 3, 2, 2, 0),   # window 3
                 (x.data_ptr(), out.data_ptr(), None, None, 1, 3, 6, 8, 16, 2, 2, 2, 0)):  # extent not divisible
        assert lib.seg_op_maxpool(*args, _capi.DTYPE["f16"], st) < 0
        assert lib.seg_last_error().decode().startswith("seg_op_maxpool")
    assert bool((out.float() == 7.0).all())
