// GroupNorm(8) + channel dropout + ReLU (+ residual add), forward and backward, channels-last.
// Reference semantics: relu(dropout3d(group_norm(conv(x)))) — networks/VNet3d.py:13-15,34-43,55-59,72-80;
// networks/Unet3d.py:64-86.  Statistics are per (sample, group) over (C/8)*V elements, biased
// variance, eps 1e-5 (torch.nn.GroupNorm).  The conv epilogues deliver per-(n,c) sum / sum-of-squares
// in fp64, so the whole GN forward is: finalize (tiny) + one elementwise pass; the backward is one
// reduction pass + finalize (tiny) + one elementwise pass.
#include <cstdio>
#include <cstdlib>

#include "kernels.h"
#include "dispatch.h"
#include "gn_math.h"

namespace seg {
namespace {

// GroupNorm statistics are independent per (sample, group): grid = (8 groups, N), 64 threads.  Every thread folds
// the STAT_REP replicas of (channel, replica-slice) pairs of its group; a wave reduction gives the group moments.
// (grid.z = 2: the two branches of the fused input block in one launch)
__global__ __launch_bounds__(64) void gn_finalize_kernel(GnFinArgs a0, GnFinArgs a1) {
    const GnFinArgs a = blockIdx.z ? a1 : a0;
    const int g = blockIdx.x, n = blockIdx.y, tid = threadIdx.x;
    const int cpg = a.C / GN_GROUPS;                    // 2..32 channels per group
    const int RG = 64 / cpg;                            // replica slices per channel
    const int cl = tid % cpg, rg = tid / cpg, c = g * cpg + cl;
    double acc[2] = {0.0, 0.0};
    if (rg < RG)                                        // batches of 8: 16 replicas per thread for C = 256
        gn_fold_replicas<8, 2>(rg, RG, STAT_REP, acc, [&](int rep, double* v) {
            const double* st = a.stats + gn_rep_at(rep, a.N, n, a.C, c);
            v[0] = st[0]; v[1] = st[1];
        });
    double mean, rstd;
    gn_moments(wave_sum_d(acc[0]), wave_sum_d(acc[1]), (double)cpg * (double)a.V, (double)a.eps, mean, rstd);
    if (tid == 0) {
        a.mean[n * GN_GROUPS + g] = (float)mean;
        a.rstd[n * GN_GROUPS + g] = (float)rstd;
    }
    if (tid < cpg) {
        const double mk = a.mask ? (double)a.mask[(long long)n * a.mask_ld + c] : 1.0;
        gn_scale_shift(mk, a.gamma[c], a.beta[c], mean, rstd, a.scale[(long long)n * a.C + c], a.shift[(long long)n * a.C + c]);
    }
}

// elementwise; one thread = one 8-channel chunk.  FOLD: the statistics finalize runs as a per-workgroup prologue
// (gn_fold_block) instead of a launch of its own - a kernel boundary costs 4-5 us on this part, the fold 1-2.
// R2 / RES: which optional sources exist, as template flags: the loop body has no branches between its loads, so a thread issues the
// loads of UNR chunks back to back and waits ONCE (with runtime `if (r2)` tests the compiler emitted load -> s_waitcnt vmcnt(0) ->
// load -> ... : up to three serial HBM round trips per 16 bytes, memory-level parallelism left to occupancy alone - and next to the
// weight-gradient stream's register-heavy workgroups a streaming kernel gets few waves per SIMD).
// HC > 0 (C == 16: two neighbouring lanes hold a voxel): the 1^d head on this activation in the same pass.  The even lane starts head_fwd_kernel's fmaf chain
// (bias, channels 0 .. 7) on the values as stored, the odd lane continues it (channels 8 .. 15) and writes the voxel's logits / probabilities: same operations
// in the same order as the separate launch.
// HCF = classes + 16 (GN_ACT_NO_STORE): the same pass without the store of `out` - the train step where the head was the tensor's only reader and its weight
// gradient comes out of the GroupNorm-backward reduce passes (GnHeadW): 113 MB less written at 4 x 96^3.
constexpr int GN_ACT_NO_STORE = 16;
template <class T, bool FOLD, bool R2, bool RES, int HCF = 0>
__global__ __launch_bounds__(256) void gn_act_kernel(ActArgs a) {
    constexpr int HC = HCF & (GN_ACT_NO_STORE - 1);
    constexpr bool STORE = HCF < GN_ACT_NO_STORE;
    __shared__ double part[FOLD ? 256 : 1][2];
    __shared__ float coef_s[FOLD ? 4 : 1][256];
    if (HC > 0 && a.zero_ptr && blockIdx.x == 0 && blockIdx.y == 0)
        for (long long i = threadIdx.x; i < a.zero_n; i += 256) a.zero_ptr[i] = 0.0;
    // grid.y = sample; chunk index inside the sample in 32 bits, C/8 a power of two: no 64-bit division per element
    const int CPR = a.C / 8, n = blockIdx.y;
    const int per_n = (int)(a.V * CPR);
    const long long base = (long long)n * per_n;
    const T* r1 = (const T*)a.r1;
    const T* r2 = (const T*)a.r2;
    const T* res = (const T*)a.res;
    T* out = (T*)a.out;
    // the grid stride is a multiple of C/8: a thread keeps its channel chunk, the coefficients live in registers
    const int c0 = ((blockIdx.x * 256 + threadIdx.x) & (CPR - 1)) * 8;
    vec<float, 8> sc, sh, sc2, sh2;
    if (FOLD) {
        gn_fold_block(a.fin1, n, blockIdx.x == 0, part, coef_s[0], coef_s[1]);
        if (R2) gn_fold_block(a.fin2, n, blockIdx.x == 0, part, coef_s[2], coef_s[3]);
        sc = *(const vec<float, 8>*)&coef_s[0][c0];
        sh = *(const vec<float, 8>*)&coef_s[1][c0];
        if (R2) { sc2 = *(const vec<float, 8>*)&coef_s[2][c0]; sh2 = *(const vec<float, 8>*)&coef_s[3][c0]; }
    } else {
        sc = *(const vec<float, 8>*)(a.scale1 + (long long)n * a.C + c0);
        sh = *(const vec<float, 8>*)(a.shift1 + (long long)n * a.C + c0);
        if (R2) {
            sc2 = *(const vec<float, 8>*)(a.scale2 + (long long)n * a.C + c0);
            sh2 = *(const vec<float, 8>*)(a.shift2 + (long long)n * a.C + c0);
        }
    }
    constexpr int UNR = (R2 || RES) ? 2 : 4;
    const int stride = gridDim.x * 256;
    float hw[HC > 0 ? HC : 1][8], hb[HC > 0 ? HC : 1];
    if (HC > 0) {
#pragma unroll
        for (int c = 0; c < HC; ++c) {
            hb[c] = a.head_b ? a.head_b[c] : 0.f;
#pragma unroll
            for (int j = 0; j < 8; ++j) hw[c][j] = a.head_w[c * 16 + c0 + j];
        }
    }
    for (int ii = blockIdx.x * 256 + threadIdx.x; ii < per_n; ii += stride * UNR) {
        long long iu[UNR];
        bool ok[UNR];
        vec<T, 8> x[UNR], x2[UNR], rr[UNR];
#pragma unroll
        for (int u = 0; u < UNR; ++u) {                 // out-of-range slots re-read slot 0 (no branch around a load) and store nothing
            const int t = ii + u * stride;
            ok[u] = t < per_n;
            iu[u] = base + (ok[u] ? t : ii);
        }
#pragma unroll
        for (int u = 0; u < UNR; ++u) {
            x[u] = load8(r1 + iu[u] * 8);
            if (R2) x2[u] = load8(r2 + iu[u] * 8);
            if (RES) rr[u] = load8(res + iu[u] * 8);
        }
#pragma unroll
        for (int u = 0; u < UNR; ++u) {
            float y[8];
#pragma unroll
            for (int j = 0; j < 8; ++j) y[j] = gn_relu(sc[j], to_f(x[u][j]), sh[j]);
            if (R2) {
#pragma unroll
                for (int j = 0; j < 8; ++j) y[j] += gn_relu(sc2[j], to_f(x2[u][j]), sh2[j]);
            }
            if (RES) {
#pragma unroll
                for (int j = 0; j < 8; ++j) y[j] += to_f(rr[u][j]);
            }
            vec<T, 8> o;
#pragma unroll
            for (int j = 0; j < 8; ++j) o[j] = from_f<T>(y[j]);
            if (STORE && ok[u]) store8(out + iu[u] * 8, o);
            if constexpr (HC > 0) {
                // (per_n is even and the trip stride a multiple of 256: both lanes of a voxel take the same trips)
                const bool hi = threadIdx.x & 1;
                float z[HC > 0 ? HC : 1];
#pragma unroll
                for (int c = 0; c < HC; ++c) {
                    float s = hb[c];
#pragma unroll
                    for (int j = 0; j < 8; ++j) s = fmaf(to_f(o[j]), hw[c][j], s);          // even lane: bias + channels 0 .. 7
                    const float lo = __shfl_xor(s, 1);                                    // odd lane: the even lane's partial chain
                    float t = lo;
#pragma unroll
                    for (int j = 0; j < 8; ++j) t = fmaf(to_f(o[j]), hw[c][j], t);          // ... continued with channels 8 .. 15
                    z[c] = t;
                }
                if (hi && ok[u]) {
                    const long long v = (long long)((ok[u] ? (int)(iu[u] - base) : 0) >> 1);
                    if (HC == 1) {
                        a.logits[(long long)n * a.V + v] = z[0];
                        a.probs[(long long)n * a.V + v] = 1.f / (1.f + expf(-z[0]));
                    } else {
                        float mx = z[0];
#pragma unroll
                        for (int c = 1; c < HC; ++c) mx = fmaxf(mx, z[c]);
                        float e[HC > 0 ? HC : 1], se = 0.f;
#pragma unroll
                        for (int c = 0; c < HC; ++c) { e[c] = expf(z[c] - mx); se += e[c]; }
                        const float inv = 1.f / se;
#pragma unroll
                        for (int c = 0; c < HC; ++c) {
                            const long long o2 = ((long long)n * HC + c) * a.V + v;
                            a.logits[o2] = z[c];
                            a.probs[o2] = e[c] * inv;
                        }
                    }
                }
            }
        }
    }
}

// i = 8-channel chunk index ((n*V + v)*C/8 + c0/8); (n, v, c0) only matter for the virtual head source
template <class T>
__device__ __forceinline__ void load_dy_sum(const GnBwdArgs& a, long long i, float* g, int n = 0, long long v = 0, int c0 = 0) {
#pragma unroll
    for (int j = 0; j < 8; ++j) g[j] = 0.f;
    if (a.vdl) {
        for (int k = 0; k < a.vK; ++k) {
            const float dl = a.vdl[((long long)n * a.vK + k) * a.V + v];
            const vec<float, 8> w = *(const vec<float, 8>*)(a.vw + (long long)k * a.C + c0);
#pragma unroll
            for (int j = 0; j < 8; ++j) g[j] = fmaf(dl, w[j], g[j]);
        }
    }
    if (a.ndy > 0) {
        const vec<T, 8> d0 = load8((const T*)a.dy[0] + i * 8);
#pragma unroll
        for (int j = 0; j < 8; ++j) g[j] += to_f(d0[j]);
    }
    if (a.ndy > 1) {
        const vec<T, 8> d1 = load8((const T*)a.dy[1] + i * 8);
#pragma unroll
        for (int j = 0; j < 8; ++j) g[j] += to_f(d1[j]);
    }
    if (a.ndy > 2) {
        const vec<T, 8> d2 = load8((const T*)a.dy[2] + i * 8);
#pragma unroll
        for (int j = 0; j < 8; ++j) g[j] += to_f(d2[j]);
    }
}

// NDY = 1..3: exactly that many stored gradient sources and no virtual one - issue() is branch-free, so callers can put the loads of
// several chunks in flight before the first use; NDY = 0: anything else (the unit below the head), through load_dy_sum.
// NDY = 4 / 5: the virtual head source of a one-class head (vK == 1: dy[v][c] += dl[n][v] * w[c]) plus 0 / 1 stored sources - the two
// 96^3 units under the head, the largest GroupNorm-backward launches of the step; one scalar load per chunk, the head weights of the
// thread's channels are loop-invariant (vw8, loaded by the caller)
// NDY = 6 / 7: as 4 / 5, and the pass also forms the head's weight gradient (GnHeadW, kernels.h) from what it holds anyway - dl and the unit's activation:
//   6 (the unit under the head, no stored source): sum_v dl * relu(GN(r)) per channel in fp32, and sum_v dl (the head's bias gradient)
//   7 (the unit whose activation is that unit's residual, one stored source): sum_v dl * round_T(relu(GN(r))), the activation as gn_act_kernel stored it
template <class T, int NDY> struct DySrc {
    static constexpr bool VH = NDY >= 4;
    static constexpr bool HW = NDY >= 6;
    static constexpr int NS = VH ? (NDY - 4) % 2 : NDY;
    vec<T, 8> d[NS > 0 ? NS : 1];
    float g0[8];
    float dl;
    __device__ __forceinline__ void issue(const GnBwdArgs& a, long long i, int n, long long v, int c0) {
        if (NDY == 0) { load_dy_sum<T>(a, i, g0, n, v, c0); return; }
        if (VH) dl = a.vdl[(long long)n * a.V + v];
#pragma unroll
        for (int k = 0; k < NS; ++k) d[k] = load8((const T*)a.dy[k] + i * 8);
    }
    __device__ __forceinline__ void sum(float* g, const vec<float, 8>& vw8) const {
#pragma unroll
        for (int j = 0; j < 8; ++j) g[j] = NDY == 0 ? g0[j] : (VH ? fmaf(dl, vw8[j], 0.f) : 0.f);
#pragma unroll
        for (int k = 0; k < NS; ++k)
#pragma unroll
            for (int j = 0; j < 8; ++j) g[j] += to_f(d[k][j]);          // same order as load_dy_sum: ((head + d0) + d1) + d2
    }
};
__host__ inline int dy_variant(const GnBwdArgs& a, const GnHeadW* hw = nullptr) {
    if (hw) {
        if (!gn_head_w_supported(a)) { fprintf(stderr, "segengine: head weight gradient on a GroupNorm-backward pass: unsupported arguments (internal error)\n"); abort(); }
        return 6 + a.ndy;
    }
    if (a.vdl) return (a.vK == 1 && a.ndy >= 0 && a.ndy <= 1) ? 4 + a.ndy : 0;
    return (a.ndy >= 1 && a.ndy <= 3) ? a.ndy : 0;
}

// pass 1.  grid = (slabs, N); a block reduces `rows_per_block` voxels of one sample over all channels.
// thread = (chunk column cc, row group g); LDS tree over row groups; fp64 atomics per (n,c).
#ifndef SEG_EMU
#define SEG_GNB_WAVES(x) __attribute__((amdgpu_waves_per_eu(x)))     // lower bound on resident waves per SIMD = upper bound on VGPRs
#else
#define SEG_GNB_WAVES(x)
#endif
// (NDY 6 / 7: nine more accumulators; left alone hipcc takes 130 - 136 registers for the 16-bit types, three waves per SIMD where NDY 4 has five.  Not for f32:
// four rows of 32-byte chunks in flight do not fit 128 registers, <float, 7> would spill)
template <class T, bool DUAL, int NDY>
__global__ __launch_bounds__(256) SEG_GNB_WAVES(NDY >= 6 && sizeof(T) == 2 ? 4 : 1) void gn_bwd_reduce_kernel(GnBwdArgs a, int GNB_ROWS) {
    constexpr int RS = NDY >= 6 ? 25 : 16;      // floats per thread in the LDS tree: q1, q2 (+ the head sums: 8 channels and dl)
    __shared__ float red[256 * RS];
    const int tid = threadIdx.x, n = blockIdx.y;
    const int CPR = a.C / 8;                  // 2..32 (power of two)
    const int G = 256 / CPR;
    const int cc = tid % CPR, g = tid / CPR;
    const long long v0 = (long long)blockIdx.x * GNB_ROWS;
    const long long v1 = (v0 + GNB_ROWS < a.V) ? v0 + GNB_ROWS : a.V;
    const T* r = (const T*)a.r;
    const T* r2 = (const T*)a.r2;
    const vec<float, 8> sc = *(const vec<float, 8>*)(a.scale + (long long)n * a.C + cc * 8);
    const vec<float, 8> sh = *(const vec<float, 8>*)(a.shift + (long long)n * a.C + cc * 8);
    vec<float, 8> sc2 = sc, sh2 = sh;
    if (DUAL) {
        sc2 = *(const vec<float, 8>*)(a.scale2 + (long long)n * a.C + cc * 8);
        sh2 = *(const vec<float, 8>*)(a.shift2 + (long long)n * a.C + cc * 8);
    }
    float q1[8], q2[8], p1[8], p2[8];          // p*: second branch
#pragma unroll
    for (int j = 0; j < 8; ++j) { q1[j] = 0.f; q2[j] = 0.f; p1[j] = 0.f; p2[j] = 0.f; }
    // RW rows in flight per thread, every load issued before the first use (pure streaming: 2-4 x 16 B loads per row)
    constexpr int RW = (NDY == 0) ? 1 : ((DUAL || DySrc<T, NDY>::NS > 1) ? 2 : 4);
    vec<float, 8> vw8;
#pragma unroll
    for (int j = 0; j < 8; ++j) vw8[j] = 0.f;
    if (DySrc<T, NDY>::VH) vw8 = *(const vec<float, 8>*)(a.vw + cc * 8);
    constexpr bool HW = DySrc<T, NDY>::HW;
    float hw8[HW ? 8 : 1], hb = 0.f;          // head weight gradient of the thread's channels; sum of dl (used from the cc == 0 column)
#pragma unroll
    for (int j = 0; j < (HW ? 8 : 1); ++j) hw8[j] = 0.f;
    long long v = v0 + g;
    for (; v < v1; v += (long long)RW * G) {
        long long iu[RW];
        bool ok[RW];
        DySrc<T, NDY> src[RW];
        vec<T, 8> x[RW], z[RW];
#pragma unroll
        for (int u = 0; u < RW; ++u) {                  // rows past the slab re-read row 0 and contribute nothing
            const long long vv = v + (long long)u * G;
            ok[u] = vv < v1;
            iu[u] = ((long long)n * a.V + (ok[u] ? vv : v)) * CPR + cc;
        }
#pragma unroll
        for (int u = 0; u < RW; ++u) {
            src[u].issue(a, iu[u], n, ok[u] ? v + (long long)u * G : v, cc * 8);
            x[u] = load8(r + iu[u] * 8);
            if (DUAL) z[u] = load8(r2 + iu[u] * 8);
        }
#pragma unroll
        for (int u = 0; u < RW; ++u) {
            float dy[8];
            src[u].sum(dy, vw8);
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                const float xv = to_f(x[u][j]);
                const float d = (ok[u] && fmaf(sc[j], xv, sh[j]) > 0.f) ? dy[j] : 0.f;
                q1[j] += d;
                q2[j] = fmaf(d, xv, q2[j]);
                if (DUAL) {
                    const float zv = to_f(z[u][j]);
                    const float e = (ok[u] && fmaf(sc2[j], zv, sh2[j]) > 0.f) ? dy[j] : 0.f;
                    p1[j] += e;
                    p2[j] = fmaf(e, zv, p2[j]);
                }
            }
            if constexpr (HW) {
                const float dlu = ok[u] ? src[u].dl : 0.f;
#pragma unroll
                for (int j = 0; j < 8; ++j) {
                    float av = gn_relu(sc[j], to_f(x[u][j]), sh[j]);
                    if (NDY == 7) av = to_f(from_f<T>(av));
                    hw8[j] = fmaf(dlu, av, hw8[j]);
                }
                if (NDY == 6) hb += dlu;
            }
        }
    }
#pragma unroll                  // (unrolled: `br ? p1 : q1` under a run-time branch index sent all four accumulator arrays to scratch, 144 B per lane)
    for (int br = 0; br < (DUAL ? 2 : 1); ++br) {
        if (br) __syncthreads();
#pragma unroll
        for (int j = 0; j < 8; ++j) { red[tid * RS + j] = br ? p1[j] : q1[j]; red[tid * RS + 8 + j] = br ? p2[j] : q2[j]; }
        if constexpr (HW) {
#pragma unroll
            for (int j = 0; j < 8; ++j) red[tid * RS + 16 + j] = hw8[j];
            red[tid * RS + 24] = hb;
        }
        __syncthreads();
        // column (cc, j, which) summed over the G row groups by one thread each: CPR*16 <= 512 columns
        double* Q = br ? a.Q2 : a.Q;
        for (int col = tid; col < CPR * 16; col += 256) {
            const int ccx = col / 16, jj = col % 16;
            double s = 0.0;
            for (int k = 0; k < G; ++k) s += red[(k * CPR + ccx) * RS + jj];
            const int c = ccx * 8 + (jj & 7), which = jj >> 3;
            atomicAdd(Q + (((long long)(blockIdx.x % (a.rep_q > 0 ? a.rep_q : STAT_REP)) * a.N + n) * a.C + c) * 2 + which, s);
        }
    }
    if constexpr (HW) {
        // the head sums take the same road, out of the same LDS pass (C + 1 <= 129 columns), into an area shaped like Q (a.Q2 of these variants:
        // launch_gn_bwd_reduce), spread over the same replicas - not straight onto the head's gradient: a few thousand workgroups adding to 17 words would
        // serialise.  Slot [c][0]: channel c; slot [0][1]: sum of dl (NDY 6 only).
        const int col = 255 - tid;                                   // from the last wave down: those threads are idle in the loop above while C <= 64
        if (col < CPR * 8 + (NDY == 6 ? 1 : 0)) {
            const int ccx = col < CPR * 8 ? col / 8 : 0, jj = col < CPR * 8 ? 16 + col % 8 : 24;
            double s = 0.0;
            for (int k = 0; k < G; ++k) s += red[(k * CPR + ccx) * RS + jj];
            const int c = jj < 24 ? ccx * 8 + (jj - 16) : 0, which = jj < 24 ? 0 : 1;
            atomicAdd(a.Q2 + (((long long)(blockIdx.x % (a.rep_q > 0 ? a.rep_q : STAT_REP)) * a.N + n) * a.C + c) * 2 + which, s);
        }
    }
}

// backward finalize: grid = (8 groups, N), 64 threads — same decomposition as the forward finalize
__global__ __launch_bounds__(64) void gn_bwd_finalize_kernel(GnBwdFinArgs a0, GnBwdFinArgs a1) {
    const GnBwdFinArgs a = blockIdx.z ? a1 : a0;
    __shared__ double sh[64][3];
    const int g = blockIdx.x, n = blockIdx.y, tid = threadIdx.x;
    const int cpg = a.C / GN_GROUPS, RG = 64 / cpg;
    const int cl = tid % cpg, rg = tid / cpg, c = g * cpg + cl;
    double f1 = 0.0, f2 = 0.0, f3 = 0.0;
    if (rg < RG) {
        const int trips = STAT_REP / RG;
        for (int j0 = 0; j0 < trips; j0 += 8) {
            double v1[8], v2[8], v3[8];
#pragma unroll
            for (int u = 0; u < 8; ++u) {
                const int rep = rg + (j0 + u) * RG;
                const long long o = (((long long)(rep < STAT_REP ? rep : rg) * a.N + n) * a.C + c) * 2;
                v1[u] = a.Q[o]; v2[u] = a.Q[o + 1]; v3[u] = a.stats[o];
            }
#pragma unroll
            for (int u = 0; u < 8; ++u)
                if (j0 + u < trips) { f1 += v1[u]; f2 += v2[u]; f3 += v3[u]; }
        }
    }
    sh[tid][0] = f1; sh[tid][1] = f2; sh[tid][2] = f3;
    __syncthreads();
    double Q1 = 0.0, Q2 = 0.0, R1 = 0.0;                 // per-channel totals (valid for tid < cpg)
    if (tid < cpg)
        for (int k = 0; k < RG; ++k) { Q1 += sh[tid + k * cpg][0]; Q2 += sh[tid + k * cpg][1]; R1 += sh[tid + k * cpg][2]; }
    const double mu = a.mean[n * GN_GROUPS + g], rs = a.rstd[n * GN_GROUPS + g];
    double mk = 1.0, ga = 0.0, q1 = 0.0, qx = 0.0;
    if (tid < cpg) {
        mk = a.mask ? (double)a.mask[(long long)n * a.mask_ld + c] : 1.0;
        ga = a.gamma[c];
        gn_bwd_terms(mk, Q1, Q2, mu, rs, q1, qx);
        atomicAdd(&a.dbeta[c], (float)q1);
        atomicAdd(&a.dgamma[c], (float)qx);
    }
    const double S1 = wave_sum_d(tid < cpg ? ga * q1 : 0.0);
    const double S2 = wave_sum_d(tid < cpg ? ga * qx : 0.0);
    if (tid < cpg) {
        double A, B, Cc;
        gn_bwd_coefs(rs, ga, mk, mu, S1, S2, (double)cpg * (double)a.V, A, B, Cc);
        float* co = a.coef + ((long long)n * a.C + c) * 3;
        co[0] = (float)A; co[1] = (float)B; co[2] = (float)Cc;
        if (a.dbias) atomicAdd(&a.dbias[c], (float)gn_bwd_dbias(A, B, Cc, Q1, R1, (double)a.V));
    }
}

// FOLD: the backward finalize runs as a per-workgroup prologue (gn_bwd_fold_block); fa / fb are the finalize arguments of the branches
template <class T, bool DUAL, bool FOLD, int NDY>
__global__ __launch_bounds__(256) void gn_bwd_apply_kernel(GnBwdArgs a, GnBwdFinArgs fa, GnBwdFinArgs fb) {
    __shared__ double part[FOLD ? 256 : 1][3];
    __shared__ float coef_s[FOLD ? (DUAL ? 6 : 3) : 1][256];
    const int CPR = a.C / 8, n = blockIdx.y;       // grid.y = sample, 32-bit chunk index inside it (C/8 is a power of two)
    const int per_n = (int)(a.V * CPR), lc = 31 - __builtin_clz(CPR);
    const long long base = (long long)n * per_n;
    const T* r = (const T*)a.r;
    T* dr = (T*)a.dr;
    // the grid stride is a multiple of C/8: a thread keeps its channel chunk, all coefficients live in registers
    const int c0 = ((blockIdx.x * 256 + threadIdx.x) & (CPR - 1)) * 8;
    float co[24], co2[24];
    if (FOLD) {
        gn_bwd_fold_block(fa, n, blockIdx.x == 0, part, coef_s[0], coef_s[1], coef_s[2]);
        if (DUAL) gn_bwd_fold_block(fb, n, blockIdx.x == 0, part, coef_s[DUAL ? 3 : 0], coef_s[DUAL ? 4 : 0], coef_s[DUAL ? 5 : 0]);
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            co[j * 3] = coef_s[0][c0 + j]; co[j * 3 + 1] = coef_s[1][c0 + j]; co[j * 3 + 2] = coef_s[2][c0 + j];
            if (DUAL) { co2[j * 3] = coef_s[DUAL ? 3 : 0][c0 + j]; co2[j * 3 + 1] = coef_s[DUAL ? 4 : 0][c0 + j]; co2[j * 3 + 2] = coef_s[DUAL ? 5 : 0][c0 + j]; }
        }
    } else {
        // per-(n, c) coefficients as wide loads (the small levels are latency-bound)
        const vec<float, 8>* cop = (const vec<float, 8>*)(a.coef + ((long long)n * a.C + c0) * 3);
        const vec<float, 8> ca = cop[0], cb = cop[1], cc = cop[2];
#pragma unroll
        for (int j = 0; j < 8; ++j) { co[j] = ca[j]; co[8 + j] = cb[j]; co[16 + j] = cc[j]; }
        if (DUAL) {
            const vec<float, 8>* cop2 = (const vec<float, 8>*)(a.coef2 + ((long long)n * a.C + c0) * 3);
            const vec<float, 8> da = cop2[0], db = cop2[1], dc = cop2[2];
#pragma unroll
            for (int j = 0; j < 8; ++j) { co2[j] = da[j]; co2[8 + j] = db[j]; co2[16 + j] = dc[j]; }
        }
    }
    // NDY 6 / 7 (never DUAL): fb describes the head sums the reduce launch left (launch_gn_bwd_apply); workgroup 0 of the sample adds them to the head's gradient
    if constexpr (DySrc<T, NDY>::HW) {
        if (blockIdx.x == 0) gn_head_w_fold(fb, n);
    }
    const vec<float, 8> sc = *(const vec<float, 8>*)(a.scale + (long long)n * a.C + c0);
    const vec<float, 8> sh = *(const vec<float, 8>*)(a.shift + (long long)n * a.C + c0);
    vec<float, 8> sc2 = sc, sh2 = sh;
    if (DUAL) {
        sc2 = *(const vec<float, 8>*)(a.scale2 + (long long)n * a.C + c0);
        sh2 = *(const vec<float, 8>*)(a.shift2 + (long long)n * a.C + c0);
    }
    // UNR chunks per trip, all loads in front (see gn_act_kernel)
    constexpr int UNR = (NDY == 0) ? 1 : ((DUAL || DySrc<T, NDY>::NS > 1) ? 2 : 4);
    vec<float, 8> vw8;
#pragma unroll
    for (int j = 0; j < 8; ++j) vw8[j] = 0.f;
    if (DySrc<T, NDY>::VH) vw8 = *(const vec<float, 8>*)(a.vw + c0);
    const int stride = gridDim.x * 256;
    for (int ii = blockIdx.x * 256 + threadIdx.x; ii < per_n; ii += stride * UNR) {
        long long iu[UNR];
        int tu[UNR];
        bool ok[UNR];
        DySrc<T, NDY> src[UNR];
        vec<T, 8> x[UNR], z[UNR];
#pragma unroll
        for (int u = 0; u < UNR; ++u) {
            const int t = ii + u * stride;
            ok[u] = t < per_n;
            tu[u] = ok[u] ? t : ii;
            iu[u] = base + tu[u];
        }
#pragma unroll
        for (int u = 0; u < UNR; ++u) {
            src[u].issue(a, iu[u], n, tu[u] >> lc, c0);
            x[u] = load8(r + iu[u] * 8);
            if (DUAL) z[u] = load8((const T*)a.r2 + iu[u] * 8);
        }
#pragma unroll
        for (int u = 0; u < UNR; ++u) {
            float dy[8];
            src[u].sum(dy, vw8);
            vec<T, 8> o;
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                const float xv = to_f(x[u][j]);
                const float d = (fmaf(sc[j], xv, sh[j]) > 0.f) ? dy[j] : 0.f;
                o[j] = from_f<T>(fmaf(co[j * 3], d, fmaf(co[j * 3 + 1], xv, co[j * 3 + 2])));
            }
            if (ok[u]) store8(dr + iu[u] * 8, o);
            if (DUAL) {
#pragma unroll
                for (int j = 0; j < 8; ++j) {
                    const float zv = to_f(z[u][j]);
                    const float d = (fmaf(sc2[j], zv, sh2[j]) > 0.f) ? dy[j] : 0.f;
                    o[j] = from_f<T>(fmaf(co2[j * 3], d, fmaf(co2[j * 3 + 1], zv, co2[j * 3 + 2])));
                }
                if (ok[u]) store8((T*)a.dr2 + iu[u] * 8, o);
            }
        }
    }
}

// ------------------------------------------------------------------------------------------------
// Small-tensor GroupNorm backward (C >= 64, i.e. the 24^3 / 12^3 / 6^3 levels whose tensors sit in L2):
// GroupNorm is independent per (sample, group), so ONE 1024-thread workgroup per (n, g) does the
// reduction pass, the coefficient math (incl. gamma/beta/bias gradients) and the elementwise pass
// back to back — one launch instead of reduce + finalize + apply (3 x ~8 us of launch/latency each).
// ------------------------------------------------------------------------------------------------
struct GnBwdGroupArgs {
    GnBwdArgs e;          // dy sources, r, forward scale/shift, dr
    GnBwdFinArgs f;       // stats, gamma, mask, mean/rstd, dgamma/dbeta/dbias
};

template <class T>
__global__ __launch_bounds__(1024) void gn_bwd_group_kernel(GnBwdGroupArgs a) {
    __shared__ float wsum[16][4][16];        // [wave][chunk-in-group][q1 0..7 | q2 0..7]
    __shared__ double chan[32][3];           // per channel of the group: Q1, Q2, R1
    __shared__ float coef[32][3];
    const int g = blockIdx.x, n = blockIdx.y, tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const int C = a.e.C, cpg = C / GN_GROUPS, CG = cpg / 8, CPR = C / 8;     // CG = 16-B chunks per voxel in this group: 1, 2 or 4
    const long long V = a.e.V;
    const int cg = tid % CG, c0 = g * cpg + cg * 8;
    const T* r = (const T*)a.e.r;
    T* dr = (T*)a.e.dr;
    const vec<float, 8> sc = *(const vec<float, 8>*)(a.e.scale + (long long)n * C + c0);
    const vec<float, 8> sh = *(const vec<float, 8>*)(a.e.shift + (long long)n * C + c0);
    float q1[8], q2[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) { q1[j] = 0.f; q2[j] = 0.f; }
    const long long items = V * CG;
    for (long long it = tid; it < items; it += 1024) {
        const long long i = ((long long)n * V + it / CG) * CPR + g * CG + cg;
        float dy[8];
        load_dy_sum<T>(a.e, i, dy);
        gn_bwd_accum8(sc, sh, load8(r + i * 8), dy, true, q1, q2);
    }
    // lanes with equal (lane % CG) hold the same channels: butterfly over the remaining lane bits
#pragma unroll
    for (int j = 0; j < 8; ++j) {
        for (int m = 32; m >= CG; m >>= 1) { q1[j] += __shfl_xor(q1[j], m); q2[j] += __shfl_xor(q2[j], m); }
    }
    if (lane < CG) {
#pragma unroll
        for (int j = 0; j < 8; ++j) { wsum[wv][lane][j] = q1[j]; wsum[wv][lane][8 + j] = q2[j]; }
    }
    // forward sum(r) of the group's channels (bias gradient): fold the statistic replicas
    if (tid < cpg) chan[tid][2] = gn_fold_sum_r(a.f, n, g * cpg + tid);
    __syncthreads();
    if (tid < cpg) {
        double s1 = 0.0, s2 = 0.0;
        for (int w = 0; w < 16; ++w) { s1 += wsum[w][tid >> 3][tid & 7]; s2 += wsum[w][tid >> 3][8 + (tid & 7)]; }
        chan[tid][0] = s1; chan[tid][1] = s2;
    }
    __syncthreads();
    if (wv == 0) {
        double mu, rs, mk, ga;
        gn_bwd_group_params(a.f, n, g, lane, mu, rs, mk, ga);
        gn_bwd_group_finish(a.f, g, lane, mu, rs, mk, ga, chan, coef, true);
    }
    __syncthreads();
    float cA[8], cB[8], cC[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) { cA[j] = coef[cg * 8 + j][0]; cB[j] = coef[cg * 8 + j][1]; cC[j] = coef[cg * 8 + j][2]; }
    for (long long it = tid; it < items; it += 1024) {
        const long long i = ((long long)n * V + it / CG) * CPR + g * CG + cg;
        float dy[8];
        load_dy_sum<T>(a.e, i, dy);
        store8(dr + i * 8, gn_bwd_apply8(sc, sh, load8(r + i * 8), dy, cA, cB, cC));
    }
}

// forward twin: statistics fold -> mean/rstd/scale/shift (stored for the backward) -> y = relu(scale*r+shift) [+ residual]
struct GnFwdGroupArgs {
    GnFinArgs f;
    const void* r; const void* res; void* out;
};

template <class T>
__global__ __launch_bounds__(1024) void gn_fwd_group_kernel(GnFwdGroupArgs a) {
    __shared__ float ssc[32], ssh[32];
    const int g = blockIdx.x, n = blockIdx.y, tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const int C = a.f.C, cpg = C / GN_GROUPS, CG = cpg / 8, CPR = C / 8;
    const long long V = a.f.V;
    if (wv == 0) {
        const int RG = 64 / cpg, cl = lane % cpg, rg = lane / cpg, c = g * cpg + cl;
        // only the replicas the producer wrote (f.rep; 4 at this level, not all 32), four independent 16-B loads per trip: the first version walked
        // all 32 replicas with one dependent L2 round trip per trip - 16 of them, ~10 of this kernel's 11 us (round-4 single-queue trace)
        double acc[2] = {0.0, 0.0};
        if (rg < RG)
            gn_fold_replicas<4, 2>(rg, RG, a.f.rep > 0 ? a.f.rep : STAT_REP, acc, [&](int rep, double* v) {
                const double* st = a.f.stats + gn_rep_at(rep, a.f.N, n, C, c);
                v[0] = st[0]; v[1] = st[1];
            });
        double mean, rstd;
        gn_moments(wave_sum_d(acc[0]), wave_sum_d(acc[1]), (double)cpg * (double)V, (double)a.f.eps, mean, rstd);
        if (lane == 0) { a.f.mean[n * GN_GROUPS + g] = (float)mean; a.f.rstd[n * GN_GROUPS + g] = (float)rstd; }
        if (lane < cpg) {
            const double mk = a.f.mask ? (double)a.f.mask[(long long)n * a.f.mask_ld + c] : 1.0;
            float sc, sh;
            gn_scale_shift(mk, a.f.gamma[c], a.f.beta[c], mean, rstd, sc, sh);
            ssc[lane] = sc; ssh[lane] = sh;
            a.f.scale[(long long)n * C + c] = sc;
            a.f.shift[(long long)n * C + c] = sh;
        }
    }
    __syncthreads();
    const int cg = tid % CG;
    float sc[8], sh[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) { sc[j] = ssc[cg * 8 + j]; sh[j] = ssh[cg * 8 + j]; }
    const T* r = (const T*)a.r;
    const T* res = (const T*)a.res;
    T* out = (T*)a.out;
    const long long items = V * CG;
    for (long long it = tid; it < items; it += 1024) {
        const long long i = ((long long)n * V + it / CG) * CPR + g * CG + cg;
        const vec<T, 8> x = load8(r + i * 8);
        float y[8];
#pragma unroll
        for (int j = 0; j < 8; ++j) y[j] = gn_relu(sc[j], to_f(x[j]), sh[j]);
        if (res) {
            const vec<T, 8> rr = load8(res + i * 8);
#pragma unroll
            for (int j = 0; j < 8; ++j) y[j] += to_f(rr[j]);
        }
        vec<T, 8> o;
#pragma unroll
        for (int j = 0; j < 8; ++j) o[j] = from_f<T>(y[j]);
        store8(out + i * 8, o);
    }
}

// ------------------------------------------------------------------------------------------------
// Deep-level GroupNorm backward in ONE launch on MANY workgroups (C >= 64: the 24^3 / 12^3 / 6^3 levels).  The two-pass form costs two latency-bound
// launches per unit there (5 - 10 us each for a tensor of <= 7 MB), the one-workgroup-per-group form above pulls a group through 1024 threads (32
// workgroups: 11 - 14 us at 6^3, 4x slower than two passes at 24^3).  Here the S workgroups of a (sample, group) each load a slice ONCE and keep it in
// registers (<= K chunks of 8 channels per thread), hand their partial sums (sum dz, sum dz*r per channel: two floats in one 8-byte word) to one another
// through memory (xwg_store / xwg_load: no fence, no atomics on data), every workgroup folds the S partials in slot order (deterministic) into the
// group's coefficients and applies them to the registers it kept.  A word is "there" when it is non-zero (+0.0 is stored as -0.0); the slot area is the
// unit's Q region, which every backward pass starts with zeros.  Workgroups of a group have consecutive ids and the dispatcher hands out ids in order, so
// the earliest unfinished group is always resident as a whole: the wait cannot starve as long as S workgroups fit on the device at once (S <= 32).
// The poll gives up after ~0.3 s and poisons the output with NaN (the gradient check of the step then reports it) instead of hanging the queue.
// PH: 0 = the kernel; 1 / 2 = its two halves as separate launches (host checker: workgroups run one after another there).
// ------------------------------------------------------------------------------------------------
struct GnBwdCoopArgs {
    GnBwdArgs e;
    GnBwdFinArgs f;
    unsigned long long* slots;      // [N][8][S][cpg] words, zero at launch
    int S, ku;                      // workgroups per (sample, group); chunks per thread (<= K)
};

template <class T, int NDY, int K, int PH>
__global__ __launch_bounds__(256, 2) void gn_bwd_coop_kernel(GnBwdCoopArgs a) {      // (two waves per SIMD: left alone hipcc takes 258 registers for <f16, 1, 8>)
    __shared__ float wsum[16][4][16];        // [DPP row of the workgroup][chunk-in-group][q1 0..7 | q2 0..7]
    __shared__ float part[256][2];           // [slot * cpg + channel]: the partial sums of every workgroup of the group
    __shared__ double chan[32][3];           // per channel of the group: Q1, Q2, R1
    __shared__ float coef[32][3];
    const int S = a.S;
    const int g = blockIdx.x / S, sl = blockIdx.x - g * S, n = blockIdx.y;
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const int C = a.e.C, cpg = C / GN_GROUPS, CG = cpg / 8, CPR = C / 8;     // CG = 16-B chunks per voxel in this group: 1, 2 or 4
    const int V = (int)a.e.V;
    const int cg = tid % CG, c0 = g * cpg + cg * 8;
    const int items = V * CG, it0 = sl * a.ku * 256;       // (a slice starts at a multiple of 256: a thread keeps its chunk column cg)
    const T* r = (const T*)a.e.r;
    T* dr = (T*)a.e.dr;
    unsigned long long* slot = a.slots + (long long)((n * GN_GROUPS + g) * S) * cpg;
    const vec<float, 8> sc = *(const vec<float, 8>*)(a.e.scale + (long long)n * C + c0);
    const vec<float, 8> sh = *(const vec<float, 8>*)(a.e.shift + (long long)n * C + c0);
    // the slice: every load in front of the first use (slots past the slice re-read a valid chunk and contribute / store nothing)
    unsigned okm = 0u;
    DySrc<T, NDY> src[K];
    vec<T, 8> x[K];
    vec<float, 8> vw8;
#pragma unroll
    for (int j = 0; j < 8; ++j) vw8[j] = 0.f;
    // chunk index of slot k = i0 + k * dI (consecutive slots lie 256 items = 256 / CG voxels apart): two registers instead of K across the exchange
    const int ifall = n * V * CPR + g * CG + cg;                       // (voxel 0: what a slot past the slice reads)
    const int i0 = ifall + ((it0 + tid) / CG) * CPR, dI = (256 / CG) * CPR;
    auto chunk_of = [&](int k) { return ((okm >> k) & 1u) ? i0 + k * dI : ifall; };
#pragma unroll
    for (int k = 0; k < K; ++k) {
        const int it = it0 + tid + k * 256;
        const bool ok = k < a.ku && it < items;
        okm |= ok ? (1u << k) : 0u;
    }
#pragma unroll
    for (int k = 0; k < K; ++k) {
        const int ic = chunk_of(k);
        src[k].issue(a.e, ic, n, 0, c0);
        x[k] = load8(r + (long long)ic * 8);
    }
    // what the coefficient math needs besides the sums travels with the slice (not as a round trip of its own behind the exchange)
    double f_mu = 0.0, f_rs = 0.0, f_mk = 0.0, f_ga = 0.0;
    if (wv == 0 && PH != 1) gn_bwd_group_params(a.f, n, g, lane, f_mu, f_rs, f_mk, f_ga);
    // forward sum(r) of the group's channels (conv-bias gradient): only the publishing workgroup needs it
    double r1 = 0.0;
    if (sl == 0 && tid < cpg && PH != 1) r1 = gn_fold_sum_r(a.f, n, g * cpg + tid);
    if (PH != 2) {
        float q1[8], q2[8];
#pragma unroll
        for (int j = 0; j < 8; ++j) { q1[j] = 0.f; q2[j] = 0.f; }
#pragma unroll
        for (int k = 0; k < K; ++k) {
            float dy[8];
            src[k].sum(dy, vw8);
            gn_bwd_accum8(sc, sh, x[k], dy, (okm >> k) & 1u, q1, q2);
        }
        // lanes with equal (lane % CG) hold the same channels: DPP sums inside the 16-lane rows, the 16 rows of the workgroup meet in LDS
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            if (CG == 1) { q1[j] = row_sum_mod<1>(q1[j]); q2[j] = row_sum_mod<1>(q2[j]); }
            else if (CG == 2) { q1[j] = row_sum_mod<2>(q1[j]); q2[j] = row_sum_mod<2>(q2[j]); }
            else { q1[j] = row_sum_mod<4>(q1[j]); q2[j] = row_sum_mod<4>(q2[j]); }
        }
        if ((lane & 15) < CG) {
#pragma unroll
            for (int j = 0; j < 8; ++j) { wsum[tid >> 4][lane & 15][j] = q1[j]; wsum[tid >> 4][lane & 15][8 + j] = q2[j]; }
        }
        __syncthreads();
        if (tid < cpg) {
            double d1 = 0.0, d2 = 0.0;                      // (fp64 like gn_bwd_group_kernel: sixteen fp32 additions in a row cost B and Cc a few ulp)
#pragma unroll
            for (int w = 0; w < 16; ++w) { d1 += wsum[w][tid >> 3][tid & 7]; d2 += wsum[w][tid >> 3][8 + (tid & 7)]; }
            const float s1 = (float)d1, s2 = (float)d2;
            unsigned long long w = ((unsigned long long)__builtin_bit_cast(unsigned, s2) << 32) | (unsigned long long)__builtin_bit_cast(unsigned, s1);
            if (w == 0ull) w = 0x80000000ull;                 // "there": +0.0 travels as -0.0
            xwg_store(slot + sl * cpg + tid, w);
        }
        if (PH == 1) return;
    }
    // every thread fetches one (workgroup, channel) word of the group (S * cpg <= 256)
    {
        const int lc = 31 - __builtin_clz(cpg);
        const int ps = tid >> lc, pc = tid & (cpg - 1);
        float v1 = 0.f, v2 = 0.f;
        if (ps < S) {
            unsigned long long w = xwg_load(slot + ps * cpg + pc);
            for (int spin = 0; w == 0ull && spin < (1 << 18); ++spin) { xwg_pause(); w = xwg_load(slot + ps * cpg + pc); }
            v1 = __builtin_bit_cast(float, (unsigned)(w & 0xffffffffull));
            v2 = __builtin_bit_cast(float, (unsigned)(w >> 32));
            if (w == 0ull) { v1 = __builtin_nanf(""); v2 = v1; }
        }
        part[tid][0] = v1; part[tid][1] = v2;
    }
    __syncthreads();
    if (tid < cpg) {
        double s1 = 0.0, s2 = 0.0;
        for (int s = 0; s < S; ++s) { s1 += (double)part[s * cpg + tid][0]; s2 += (double)part[s * cpg + tid][1]; }
        chan[tid][0] = s1; chan[tid][1] = s2; chan[tid][2] = r1;
    }
    __syncthreads();
    if (wv == 0) gn_bwd_group_finish(a.f, g, lane, f_mu, f_rs, f_mk, f_ga, chan, coef, sl == 0);
    __syncthreads();
    float cA[8], cB[8], cC[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) { cA[j] = coef[cg * 8 + j][0]; cB[j] = coef[cg * 8 + j][1]; cC[j] = coef[cg * 8 + j][2]; }
#pragma unroll
    for (int k = 0; k < K; ++k) {
        float dy[8];
        src[k].sum(dy, vw8);
        if ((okm >> k) & 1u) store8(dr + (long long)chunk_of(k) * 8, gn_bwd_apply8(sc, sh, x[k], dy, cA, cB, cC));
    }
}

inline int ew_blocks(long long total_threads) {
    long long b = (total_threads + 255) / 256;
    return (int)(b > 16384 ? 16384 : (b < 1 ? 1 : b));
}
// grid.x of the elementwise passes, per sample; fold: every workgroup repeats the finalize prologue - fewer, longer-running workgroups on the big
// levels (at most ~2048 in all)
inline int ew_blocks_per_sample(long long total_threads, bool fold, int N) {
    const int bx = ew_blocks(total_threads);
    if (!fold) return bx;
    constexpr int cap = 2048;
    const int per_n = cap / N > 0 ? cap / N : 1;
    return bx > per_n ? per_n : bx;
}

}  // namespace

void launch_gn_finalize(const GnFinArgs& a, hipStream_t s, const GnFinArgs* b) {
    hipLaunchKernelGGL(gn_finalize_kernel, dim3(GN_GROUPS, a.N, b ? 2 : 1), dim3(64), 0, s, a, b ? *b : a);
}

void launch_gn_act(const ActArgs& a, int dtype, hipStream_t s, bool no_store) {
    dim3 grid(ew_blocks_per_sample(a.V * (a.C / 8), a.fold != 0, a.N), a.N);
    if (a.head_w && !gn_act_head_supported(a.C, a.head_C, a.r2 != nullptr)) { fprintf(stderr, "segengine: head in the activation pass: unsupported shape (internal error)\n"); abort(); }
    if (no_store && !(a.head_w && a.head_C == 1)) { fprintf(stderr, "segengine: activation pass without its store: one-class head only (internal error)\n"); abort(); }
    // HC: the head's classes computed in this pass (1, 2, else 4), 0 without a head; the head forms exist for one branch (no R2) only
    const int hc = !a.head_w ? 0 : no_store ? 1 + GN_ACT_NO_STORE : a.head_C == 1 ? 1 : a.head_C == 2 ? 2 : 4;
    by_dtype(dtype, [&](auto t) { by_bool(a.fold, [&](auto fold) { by_bool(a.r2 && !hc, [&](auto r2) { by_bool(a.res != nullptr, [&](auto rs) {
        by_int<0, 1, 2, 4, 1 + GN_ACT_NO_STORE>(hc, [&](auto h) {
            if constexpr (!(r2() && h()))
                hipLaunchKernelGGL(HIP_KERNEL_NAME(gn_act_kernel<tag_type<decltype(t)>, fold(), r2(), rs(), h()>), grid, dim3(256), 0, s, a);
        });
    }); }); }); });
}

bool gn_head_w_supported(const GnBwdArgs& a) {
    return a.vdl && a.vK == 1 && !a.r2 && a.ndy >= 0 && a.ndy <= 1 && a.C >= 16 && a.C <= 128;      // (the fold takes C + 1 threads of one wave quartet)
}

void launch_gn_bwd_reduce(const GnBwdArgs& a0, int dtype, hipStream_t s, const GnHeadW* hw) {
    const int nv = dy_variant(a0, hw);
    // head sums: the kernel argument block keeps its layout - the variants without a second branch find their area in its Q slot
    GnBwdArgs a = a0;
    if (hw) a.Q2 = hw->sums;
    // slab size: ~2048 workgroups in total, at least two rows per thread, at most 1024 rows (small tensors were
    // latency-bound with the fixed 512-row slabs: 16 workgroups x 16 serial round trips)
    const int G = 256 / (a.C / 8);
    long long rows = ((long long)a.N * a.V + 2047) / 2048;
    rows = (rows + G - 1) / G * G;
    if (rows < 2 * G) rows = 2 * G;
    constexpr int max_rows = 1024;   // measured: 256 -> 686, 512 -> 688, 1024..4096 -> 690.5 volumes/s
    if (rows > max_rows) rows = max_rows / G * G;
    const int GNB_ROWS = (int)rows;
    dim3 grid(cdiv(a.V, GNB_ROWS), a.N);
    by_dtype(dtype, [&](auto t) { by_bool(a.r2 != nullptr, [&](auto dual) { by_int<1, 2, 3, 4, 5, 6, 7, 0>(nv, [&](auto k) {
        if constexpr (!(dual() && k() >= 6))
            hipLaunchKernelGGL(HIP_KERNEL_NAME(gn_bwd_reduce_kernel<tag_type<decltype(t)>, dual(), k()>), grid, dim3(256), 0, s, a, GNB_ROWS);
    }); }); });
}

// measured on MI355X: one workgroup per (n,g) only wins while the per-sample tensor is <= ~128 KB (the 6^3 level:
// 12 us vs 22 us for three launches); at 12^3 it ties, at 24^3 it is 4x slower (32 workgroups cannot pull 7 MB)
bool gn_bwd_group_eligible(int C, long long V, int esz) { return C >= 64 && C <= 256 && (long long)C * V * esz <= (128ll << 10); }

void launch_gn_fwd_group(const GnFinArgs& f, const void* r, const void* res, void* out, int dtype, hipStream_t s) {
    GnFwdGroupArgs a; a.f = f; a.r = r; a.res = res; a.out = out;
    dim3 grid(GN_GROUPS, f.N);
    by_dtype(dtype, [&](auto t) { hipLaunchKernelGGL(HIP_KERNEL_NAME(gn_fwd_group_kernel<tag_type<decltype(t)>>), grid, dim3(1024), 0, s, a); });
}

void launch_gn_bwd_group(const GnBwdArgs& e, const GnBwdFinArgs& f, int dtype, hipStream_t s) {
    GnBwdGroupArgs a; a.e = e; a.f = f;
    dim3 grid(GN_GROUPS, e.N);
    by_dtype(dtype, [&](auto t) { hipLaunchKernelGGL(HIP_KERNEL_NAME(gn_bwd_group_kernel<tag_type<decltype(t)>>), grid, dim3(1024), 0, s, a); });
}

// S workgroups of 256 threads per (sample, group), ku <= K chunks per thread: about one workgroup per CU in all, more where a slice would not fit the
// registers (K = 8 chunks of 16-bit data, 4 of f32), never more than 1024 workgroups or 32 per group, S * cpg <= 256 (one polled word per thread).
// Only tensors of a few MB: the reduce + apply launches are latency-bound there; on a larger tensor they stream at the copy rate and one launch that holds the
// tensor in registers is slower (MI355X, round 6, in-call A/B of VNet3d 4 x 96^3: every >= 64-channel level 1052 - 1055 volumes/s, only <= 4 MB 1048 - 1050, none
// 1042 - 1044 - 7 MB at 24^3, 1.8 MB at 12^3 11 us against 13, 0.44 MB at 6^3 8 us against 12.5; 512 instead of 256 workgroups 1030 - 1044; VNet2d 16 x 512^2 with
// its 8 - 34 MB tensors 6.58 ms with the one-launch form against 6.33 ms without)
bool gn_bwd_coop_plan(int C, long long V, int N, int esz, int* S_out, int* ku_out) {
    const int cpg = C / GN_GROUPS;
    if (C % 64 || cpg < 8 || cpg > 32 || N < 1 || V < 1) return false;
    constexpr long long max_bytes = 8000000;
    constexpr int target = 256;
    if ((long long)N * V * C * esz > max_bytes) return false;
    const int CG = cpg / 8, kmax = esz == 2 ? 8 : 4;
    const long long items = V * CG;
    int smax = 256 / cpg;
    if (smax > 32) smax = 32;
    while (smax > 1 && GN_GROUPS * N * smax > 1024) smax >>= 1;
    int S = target / (GN_GROUPS * N);
    if (S < 1) S = 1;
    if (S > smax) S = smax;
    int ku = (int)((items + (long long)S * 256 - 1) / ((long long)S * 256));
    while (ku > kmax && S < smax) { S *= 2; if (S > smax) S = smax; ku = (int)((items + (long long)S * 256 - 1) / ((long long)S * 256)); }
    if (ku > kmax) return false;
    S = (int)((items + (long long)ku * 256 - 1) / ((long long)ku * 256));      // (no empty slices)
    if (S_out) *S_out = S;
    if (ku_out) *ku_out = ku;
    return true;
}
bool gn_bwd_coop_eligible(const GnBwdArgs& e, int esz) {
    return !e.vdl && !e.r2 && e.ndy >= 1 && e.ndy <= 3 && gn_bwd_coop_plan(e.C, e.V, e.N, esz, nullptr, nullptr);
}

void launch_gn_bwd_coop(const GnBwdArgs& e, const GnBwdFinArgs& f, int dtype, hipStream_t s) {
    GnBwdCoopArgs a; a.e = e; a.f = f;
    a.slots = (unsigned long long*)e.Q;
    gn_bwd_coop_plan(e.C, e.V, e.N, dtype == DT_F32 ? 4 : 2, &a.S, &a.ku);
    dim3 grid(GN_GROUPS * a.S, e.N);
    // K: chunks per thread, the smallest of 2 / 4 / 8 that holds ku (8 only for the 16-bit types: the plan keeps ku <= 4 for f32); NDY: 1, 2, else 3
    const int ndy = e.ndy == 1 ? 1 : e.ndy == 2 ? 2 : 3;
    by_dtype(dtype, [&](auto t) {
        using T = tag_type<decltype(t)>;
        const int kk = a.ku <= 2 ? 2 : (a.ku <= 4 || sizeof(T) != 2) ? 4 : 8;
        by_int<1, 2, 3>(ndy, [&](auto d) { by_int<2, 4, 8>(kk, [&](auto k) {
            if constexpr (k() != 8 || sizeof(T) == 2) {
#ifdef SEG_EMU
                hipLaunchKernelGGL(HIP_KERNEL_NAME(gn_bwd_coop_kernel<T, d(), k(), 1>), grid, dim3(256), 0, s, a);
                hipLaunchKernelGGL(HIP_KERNEL_NAME(gn_bwd_coop_kernel<T, d(), k(), 2>), grid, dim3(256), 0, s, a);
#else
                hipLaunchKernelGGL(HIP_KERNEL_NAME(gn_bwd_coop_kernel<T, d(), k(), 0>), grid, dim3(256), 0, s, a);
#endif
            }
        }); });
    });
}

void launch_gn_bwd_finalize(const GnBwdFinArgs& a, hipStream_t s, const GnBwdFinArgs* b) {
    hipLaunchKernelGGL(gn_bwd_finalize_kernel, dim3(GN_GROUPS, a.N, b ? 2 : 1), dim3(64), 0, s, a, b ? *b : a);
}


void launch_gn_bwd_apply(const GnBwdArgs& a, int dtype, hipStream_t s, const GnBwdFinArgs* fa, const GnBwdFinArgs* fb, const GnHeadW* hw) {
    const bool fold = fa != nullptr;
    dim3 grid(ew_blocks_per_sample(a.V * (a.C / 8), fold, a.N), a.N);
    const GnBwdFinArgs za = fa ? *fa : GnBwdFinArgs{};
    GnBwdFinArgs zb = fb ? *fb : GnBwdFinArgs{};
    const int nv = dy_variant(a, hw);
    if (hw) {          // the second branch's finalize block (these variants have none) carries the head sums: gn_head_w_fold
        zb = GnBwdFinArgs{};
        zb.Q = hw->sums; zb.dgamma = hw->dw; zb.dbias = a.ndy == 0 ? hw->db : nullptr;
        zb.N = a.N; zb.C = a.C; zb.rep_q = a.rep_q;
    }
    by_dtype(dtype, [&](auto t) { by_bool(a.r2 != nullptr, [&](auto dual) { by_bool(fold, [&](auto fd) { by_int<1, 2, 3, 4, 5, 6, 7, 0>(nv, [&](auto k) {
        if constexpr (!(dual() && k() >= 6))
            hipLaunchKernelGGL(HIP_KERNEL_NAME(gn_bwd_apply_kernel<tag_type<decltype(t)>, dual(), fd(), k()>), grid, dim3(256), 0, s, a, za, zb);
    }); }); }); });
}

}  // namespace seg
