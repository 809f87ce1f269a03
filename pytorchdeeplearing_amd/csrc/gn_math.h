// The GroupNorm(8) + dropout + ReLU arithmetic: the moments and scale / shift of the forward, the per-channel terms and the A / B / Cc coefficients of
// the backward, each defined ONCE and used by all five forward / backward forms of norm.hip, which differ only in how they reduce across lanes
// (wave_sum_d in the finalize kernels and the group finish, a butterfly over the cpg lanes of a group in the fold blocks).  Also here: the replica
// fold, the per-element gate / activation / gradient point (conv.hip, wgrad.hip and stemx.hip use them where they activate or gate on the fly), their
// 8-channel chunk forms and the two per-workgroup prologues (gn_fold_block, gn_bwd_fold_block).
// NOT on the helpers, on purpose (tools/isa_audit.py, parent against new): gn_bwd_reduce_kernel and gn_bwd_apply_kernel keep their own gate /
// accumulate / apply loops - with gn_gate or the chunk forms gn_bwd_reduce_kernel<16-bit, single, NDY 4> (the 96^3 units under the head) goes from 96
// to 114 VGPRs and from 5 to 4 waves per SIMD, gn_bwd_apply_kernel<bf16, DUAL, FOLD, NDY 5> from 4 to 3; and the two three-value replica loops
// (gn_bwd_finalize_kernel, gn_bwd_fold_block) stay written out - through gn_fold_replicas each gains a serial load chain (a branch around the load).
#pragma once
#include "kernels.h"

namespace seg {

// ---- per element ------------------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ float gn_relu(float sc, float x, float sh) { return fmaxf(fmaf(sc, x, sh), 0.f); }
// the ReLU gate on the forward pre-activation; `ok` = false: a slot that re-read a valid element and contributes nothing
__device__ __forceinline__ float gn_gate(float sc, float x, float sh, float dy, bool ok = true) { return (ok && fmaf(sc, x, sh) > 0.f) ? dy : 0.f; }
__device__ __forceinline__ float gn_bwd_point(float A, float d, float B, float x, float Cc) { return fmaf(A, d, fmaf(B, x, Cc)); }

// ---- 8-channel chunks (sc / sh / coefficients: anything indexable, vec<float, 8> or float[8]) ---------------------------------------------
// q1 += dz, q2 += dz * r
template <class T, class S>
__device__ __forceinline__ void gn_bwd_accum8(const S& sc, const S& sh, const vec<T, 8>& x, const float* dy, bool ok, float* q1, float* q2) {
#pragma unroll
    for (int j = 0; j < 8; ++j) {
        const float xv = to_f(x[j]);
        const float d = gn_gate(sc[j], xv, sh[j], dy[j], ok);
        q1[j] += d;
        q2[j] = fmaf(d, xv, q2[j]);
    }
}
template <class T, class S>
__device__ __forceinline__ vec<T, 8> gn_bwd_apply8(const S& sc, const S& sh, const vec<T, 8>& x, const float* dy, const float* cA, const float* cB,
                                                   const float* cC) {
    vec<T, 8> o;
#pragma unroll
    for (int j = 0; j < 8; ++j) {
        const float xv = to_f(x[j]);
        o[j] = from_f<T>(gn_bwd_point(cA[j], gn_gate(sc[j], xv, sh[j], dy[j]), cB[j], xv, cC[j]));
    }
    return o;
}

// ---- forward statistics (fp64) ------------------------------------------------------------------------------------------------------------
// group sums (sum, sum of squares over cnt elements) -> mean, 1 / sqrt(biased variance + eps)
__device__ __forceinline__ void gn_moments(double s, double ss, double cnt, double eps, double& mean, double& rstd) {
    mean = s / cnt;
    double var = ss / cnt - mean * mean;
    if (var < 0.0) var = 0.0;
    rstd = 1.0 / sqrt(var + eps);
}
// in fp64, rounded once: beta - gamma * mean * rstd cancels where a channel's output is centred near zero, and in fp32 the shift
// then carries the rounding of its (much larger) terms into every activation of the channel
__device__ __forceinline__ void gn_scale_shift(double mk, double ga, double be, double mean, double rstd, float& sc, float& sh) {
    sc = (float)(mk * ga * rstd);
    sh = (float)(mk * (be - ga * mean * rstd));
}

// ---- backward coefficients (fp64) -----------------------------------------------------------------------------------------------------------
// per channel, from its sums Q1 = sum dzr, Q2 = sum dzr * r: q1 = sum dz, qx = sum dz * xhat (the beta / gamma gradients of the sample)
__device__ __forceinline__ void gn_bwd_terms(double mk, double Q1, double Q2, double mu, double rs, double& q1, double& qx) {
    q1 = mk * Q1;
    qx = (mk * Q2 - mu * q1) * rs;
}
// dr = A * dzr + B * r + Cc; S1 / S2 = sum over the group's channels of gamma * q1 / gamma * qx, Mg = elements per (sample, group)
__device__ __forceinline__ void gn_bwd_coefs(double rs, double ga, double mk, double mu, double S1, double S2, double Mg, double& A, double& B, double& Cc) {
    A = rs * ga * mk;
    B = -rs * rs * S2 / Mg;
    Cc = -rs * S1 / Mg + rs * rs * S2 * mu / Mg;
}
// sum_v dr = A * sum(dzr) + B * sum(r) + Cc * V   (sum(r) from the forward statistics): the conv-bias gradient of the sample
__device__ __forceinline__ double gn_bwd_dbias(double A, double B, double Cc, double Q1, double R1, double V) { return A * Q1 + B * R1 + Cc * V; }

// ---- replica fold -----------------------------------------------------------------------------------------------------------------------------
// element offset of (replica, n, c) in a [rep][N][C][2] fp64 array
__device__ __forceinline__ long long gn_rep_at(int rep, int N, int n, int C, int c) { return (((long long)rep * N + n) * C + c) * 2; }
// acc[0 .. NV) += the values of replicas first, first + stride, ... < count.  load(rep, v) fetches the NV values of one replica; batches of U
// independent loads, all issued before the first add: a load -> add loop serialises one L2 round trip per replica.  Slots past `count` re-read replica
// `first` (no branch around a load) and add nothing.  The add is guarded by the slot's number, the address by the replica index: written as ONE
// condition the compiler turns the pair into a branch around the load and the batch into a chain of round trips (tools/isa_audit.py: "chains").
template <int U, int NV, class Load>
__device__ __forceinline__ void gn_fold_replicas(int first, int stride, int count, double* acc, Load load) {
    const int trips = (count - first + stride - 1) / stride;
    for (int j0 = 0; j0 < trips; j0 += U) {
        double v[U][NV];
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const int rep = first + (j0 + u) * stride;
            load(rep < count ? rep : first, v[u]);
        }
#pragma unroll
        for (int u = 0; u < U; ++u)
            if (j0 + u < trips) {
#pragma unroll
                for (int k = 0; k < NV; ++k) acc[k] += v[u][k];
            }
    }
}

// ---- one wave finishes a (sample, group) of the backward: cpg <= 32 channels, one per lane ----------------------------------------------------------
// what the finish needs besides the sums: mean / rstd of the group, multiplier and gamma of the lane's channel (0 on the lanes past cpg)
__device__ __forceinline__ void gn_bwd_group_params(const GnBwdFinArgs& f, int n, int g, int lane, double& mu, double& rs, double& mk, double& ga) {
    const int cpg = f.C / GN_GROUPS, c = g * cpg + (lane < cpg ? lane : 0);
    mu = f.mean[n * GN_GROUPS + g]; rs = f.rstd[n * GN_GROUPS + g];
    mk = 0.0; ga = 0.0;
    if (lane < cpg) {
        mk = f.mask ? (double)f.mask[(long long)n * f.mask_ld + c] : 1.0;
        ga = (double)f.gamma[c];
    }
}
// chan[lane] = {Q1, Q2, R1} of the lane's channel -> coef[lane] = {A, B, Cc}; `publish`: adds the gamma / beta / conv-bias gradients of the sample.
// Called by all 64 lanes of one wave.
__device__ __forceinline__ void gn_bwd_group_finish(const GnBwdFinArgs& f, int g, int lane, double mu, double rs, double mk, double ga,
                                                    const double (*chan)[3], float (*coef)[3], bool publish) {
    const int cpg = f.C / GN_GROUPS, c = g * cpg + (lane < cpg ? lane : 0);
    const bool act = lane < cpg;
    const double V = (double)f.V;
    const double Q1 = act ? chan[lane][0] : 0.0, Q2 = act ? chan[lane][1] : 0.0, R1 = act ? chan[lane][2] : 0.0;
    double q1, qx;
    gn_bwd_terms(mk, Q1, Q2, mu, rs, q1, qx);
    const double S1 = wave_sum_d(ga * q1), S2 = wave_sum_d(ga * qx);
    if (act) {
        double A, B, Cc;
        gn_bwd_coefs(rs, ga, mk, mu, S1, S2, (double)cpg * V, A, B, Cc);
        coef[lane][0] = (float)A; coef[lane][1] = (float)B; coef[lane][2] = (float)Cc;
        if (publish) {
            atomicAdd(&f.dbeta[c], (float)q1);
            atomicAdd(&f.dgamma[c], (float)qx);
            if (f.dbias) atomicAdd(&f.dbias[c], (float)gn_bwd_dbias(A, B, Cc, Q1, R1, V));
        }
    }
}
// forward sum(r) of one channel (the conv-bias gradient needs it): fold of the `rep_s` statistic replicas the forward producer wrote
__device__ __forceinline__ double gn_fold_sum_r(const GnBwdFinArgs& f, int n, int c) {
    double r1 = 0.0;
    gn_fold_replicas<4, 1>(0, 1, f.rep_s > 0 ? f.rep_s : STAT_REP, &r1, [&](int rep, double* v) { v[0] = f.stats[gn_rep_at(rep, f.N, n, f.C, c)]; });
    return r1;
}

// ---- head weight gradient collected by a reduce pass (GnHeadW): the fold of one sample, by the workgroup that publishes the sample's other gradients -------
// h.Q: the sums area, shaped like Q - slot [c][0] = sum_v dl * activation[c], slot [0][1] = sum_v dl - over h.rep_q replicas; h.dgamma: the head's weight
// gradient [C], h.dbias: its bias gradient or null (the pass that did not collect it).  C + 1 threads, no barrier.
__device__ __forceinline__ void gn_head_w_fold(const GnBwdFinArgs& h, int n) {
    const int tid = threadIdx.x, C = h.C;
    if (tid > C || (tid == C && !h.dbias)) return;
    const int c = tid < C ? tid : 0, which = tid < C ? 0 : 1;
    double s = 0.0;
    gn_fold_replicas<8, 1>(0, 1, h.rep_q > 0 ? h.rep_q : STAT_REP, &s, [&](int rep, double* v) { v[0] = h.Q[gn_rep_at(rep, h.N, n, C, c) + which]; });
    atomicAdd(which ? h.dbias : &h.dgamma[c], (float)s);
}

// ---- the finalize of one sample inside a consumer workgroup (256 threads, C = 16..256) ---------------------------------------------------------------
// Forward: fold the `rep` replica partial sums, reduce the channels of a group with lane butterflies (the cpg = C/8 channels of a group are
// neighbouring lanes) and leave scale / shift of every channel in LDS.  `publish`: this workgroup also writes the per-(n, c) coefficients and
// per-(n, g) moments the backward pass reads.  Ends with a barrier.
__device__ __forceinline__ void gn_fold_block(const GnFinArgs& f, int n, bool publish, double (*part)[2], float* sc_s, float* sh_s) {
    const int tid = threadIdx.x, C = f.C, cpg = C / GN_GROUPS;
    const int S = 256 / C;                              // replica slices folded side by side (C <= 256)
    const int c = tid % C, sl = tid / C;
    // the per-channel parameters do not depend on the statistics: their loads travel together with the first replica loads instead of
    // forming a second L2 round trip behind the barrier (every workgroup of every elementwise launch runs this prologue)
    float mk = 1.f, ga = 0.f, be = 0.f;
    if (tid < C) {
        mk = f.mask ? f.mask[(long long)n * f.mask_ld + tid] : 1.f;
        ga = f.gamma[tid]; be = f.beta[tid];
    }
    double acc[2] = {0.0, 0.0};
    gn_fold_replicas<4, 2>(sl, S, f.rep > 0 ? f.rep : STAT_REP, acc, [&](int rep, double* v) {
        const double* st = f.stats + gn_rep_at(rep, f.N, n, C, c);
        v[0] = st[0]; v[1] = st[1];
    });
    part[tid][0] = acc[0]; part[tid][1] = acc[1];
    __syncthreads();
    double s = 0.0, ss = 0.0;
    if (tid < C)
        for (int k = 0; k < S; ++k) { s += part[tid + k * C][0]; ss += part[tid + k * C][1]; }
    for (int o = cpg >> 1; o >= 1; o >>= 1) { s += __shfl_xor(s, o); ss += __shfl_xor(ss, o); }
    if (tid < C) {
        double mean, rstd;
        gn_moments(s, ss, (double)cpg * (double)f.V, (double)f.eps, mean, rstd);
        float sc, sh;
        gn_scale_shift((double)mk, (double)ga, (double)be, mean, rstd, sc, sh);
        sc_s[c] = sc; sh_s[c] = sh;
        if (publish) {
            f.scale[(long long)n * C + c] = sc;
            f.shift[(long long)n * C + c] = sh;
            if (c % cpg == 0) { f.mean[n * GN_GROUPS + c / cpg] = (float)mean; f.rstd[n * GN_GROUPS + c / cpg] = (float)rstd; }
        }
    }
    __syncthreads();
}

// Backward (same decomposition): folds the replica partials of Q (sum dz, sum dz*r) and of the forward channel sums, and leaves the A / B / Cc
// coefficients of every channel in LDS.  `publish`: this workgroup adds the gamma / beta / conv-bias gradients of its sample.  Ends with a barrier.
__device__ __forceinline__ void gn_bwd_fold_block(const GnBwdFinArgs& f, int n, bool publish, double (*part)[3], float* A_s, float* B_s,
                                                  float* C_s) {
    const int tid = threadIdx.x, C = f.C, cpg = C / GN_GROUPS;
    const int S = 256 / C;
    const int c = tid % C, sl = tid / C;
    const int nq = f.rep_q > 0 ? f.rep_q : STAT_REP, ns = f.rep_s > 0 ? f.rep_s : STAT_REP;
    const int nrep = nq > ns ? nq : ns;
    // loads that do not depend on the folded sums are issued up front (one L2 round trip for the prologue, not two)
    double mu = 0.0, rs = 0.0, mk = 1.0, ga = 0.0;
    if (tid < C) {
        mu = f.mean[n * GN_GROUPS + tid / cpg]; rs = f.rstd[n * GN_GROUPS + tid / cpg];
        mk = f.mask ? (double)f.mask[(long long)n * f.mask_ld + tid] : 1.0;
        ga = f.gamma[tid];
    }
    double f1 = 0.0, f2 = 0.0, f3 = 0.0;
    for (int r0 = sl; r0 < nrep; r0 += 4 * S) {
        double v1[4], v2[4], v3[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const int rep = r0 + u * S;
            const long long o = (((long long)(rep < nrep ? rep : sl) * f.N + n) * C + c) * 2;
            v1[u] = f.Q[o]; v2[u] = f.Q[o + 1]; v3[u] = f.stats[o];
        }
#pragma unroll
        for (int u = 0; u < 4; ++u)
            if (r0 + u * S < nrep) { f1 += v1[u]; f2 += v2[u]; f3 += v3[u]; }
    }
    part[tid][0] = f1; part[tid][1] = f2; part[tid][2] = f3;
    __syncthreads();
    double Q1 = 0.0, Q2 = 0.0, R1 = 0.0, q1 = 0.0, qx = 0.0;
    if (tid < C) {
        for (int k = 0; k < S; ++k) { Q1 += part[tid + k * C][0]; Q2 += part[tid + k * C][1]; R1 += part[tid + k * C][2]; }
        gn_bwd_terms(mk, Q1, Q2, mu, rs, q1, qx);
        if (publish) {
            atomicAdd(&f.dbeta[c], (float)q1);
            atomicAdd(&f.dgamma[c], (float)qx);
        }
    }
    double S1 = ga * q1, S2 = ga * qx;
    for (int o = cpg >> 1; o >= 1; o >>= 1) { S1 += __shfl_xor(S1, o); S2 += __shfl_xor(S2, o); }
    if (tid < C) {
        double A, B, Cc;
        gn_bwd_coefs(rs, ga, mk, mu, S1, S2, (double)cpg * (double)f.V, A, B, Cc);
        A_s[c] = (float)A; B_s[c] = (float)B; C_s[c] = (float)Cc;
        if (publish) {
            if (f.coef) { float* co = f.coef + ((long long)n * C + c) * 3; co[0] = (float)A; co[1] = (float)B; co[2] = (float)Cc; }
            if (f.dbias) atomicAdd(&f.dbias[c], (float)gn_bwd_dbias(A, B, Cc, Q1, R1, (double)f.V));
        }
    }
    __syncthreads();
}

}  // namespace seg
