// Classification head of the ResNet2d / ResNet3d classifiers (networks/ResNet3d.py:61-69,91-96,114-116 of the reference): global average pooling over the
// last encoder activation, Linear(256, 128) + ReLU, Linear(128, numclass), and their backward.  The reference's DownTransition reads an undefined module
// global `prob` (it cannot be constructed as shipped); the engine uses p = 0.2, the VNet value, for the four dropout calls in front of this head.
//
// Everything here is small (N x 256 pooled values, 33 K + 128 C weights) and latency-bound; the design goal is determinism, not throughput:
//   * no floating-point atomics, no grid that depends on data, nothing read back;
//   * voxel sum: fp64, one workgroup per (sample, 64-voxel slab) adds its voxels in ascending order, the FC kernel folds the slabs in ascending order;
//   * FC dot products: fp32 fmaf chains, lane l of a wave takes k = l, l + 64, ..., then the xor butterfly of wave_sum (a fixed tree), then + bias;
//   * sums over samples (parameter gradients): ascending n in one thread.
// The FC weights are read from the flat fp32 master buffer in PyTorch's [out][in] layout - nothing is packed for this head.
#include "kernels.h"
#include "dispatch.h"

namespace seg {

namespace {

inline int cls_slabs(long long V) { return (int)((V + CLS_SLAB - 1) / CLS_SLAB); }

// slab[n][sb][k] = sum of act[n][v][k] over the voxels of slab sb (fp64, ascending v); thread = channel
template <class T>
__global__ __launch_bounds__(CLS_K) void cls_pool_kernel(const T* __restrict__ act, double* __restrict__ slab, long long V, int nslab) {
    const int k = threadIdx.x, sb = blockIdx.x, n = blockIdx.y;
    const long long v0 = (long long)sb * CLS_SLAB;
    const long long v1 = v0 + CLS_SLAB < V ? v0 + CLS_SLAB : V;
    const T* p = act + ((long long)n * V + v0) * CLS_K + k;
    double s = 0.0;
    for (long long v = v0; v < v1; ++v, p += CLS_K) s += (double)to_f(*p);
    slab[((long long)n * nslab + sb) * CLS_K + k] = s;
}

// one workgroup per sample: pooled -> h -> logits -> probs
__global__ __launch_bounds__(CLS_K) void cls_fc_fwd_kernel(const double* __restrict__ slab, int nslab, long long V, const float* __restrict__ w1,
                                                           const float* __restrict__ b1, const float* __restrict__ w2, const float* __restrict__ b2,
                                                           float* __restrict__ pooled, float* __restrict__ h, float* __restrict__ logits,
                                                           float* __restrict__ probs, int C) {
    __shared__ float sp[CLS_K];
    __shared__ float sh[CLS_H];
    __shared__ float sz[16];
    const int t = threadIdx.x, n = blockIdx.x, lane = t & 63, wv = t >> 6;
    double s = 0.0;
    for (int i = 0; i < nslab; ++i) s += slab[((long long)n * nslab + i) * CLS_K + t];
    const float pv = (float)(s / (double)V);
    sp[t] = pv;
    pooled[(long long)n * CLS_K + t] = pv;
    __syncthreads();
    for (int j = wv; j < CLS_H; j += CLS_K / 64) {
        const float* w = w1 + (long long)j * CLS_K;
        float acc = 0.f;
#pragma unroll
        for (int q = 0; q < CLS_K / 64; ++q) acc = fmaf(w[lane + 64 * q], sp[lane + 64 * q], acc);
        acc = wave_sum(acc);
        if (lane == 0) {
            const float hv = fmaxf(acc + b1[j], 0.f);
            sh[j] = hv;
            h[(long long)n * CLS_H + j] = hv;
        }
    }
    __syncthreads();
    for (int c = wv; c < C; c += CLS_K / 64) {
        const float* w = w2 + (long long)c * CLS_H;
        float acc = 0.f;
#pragma unroll
        for (int q = 0; q < CLS_H / 64; ++q) acc = fmaf(w[lane + 64 * q], sh[lane + 64 * q], acc);
        acc = wave_sum(acc);
        if (lane == 0) sz[c] = acc + b2[c];
    }
    __syncthreads();
    if (t < C) logits[(long long)n * C + t] = sz[t];
    if (t == 0) {
        float* pr = probs + (long long)n * C;
        if (C == 1) pr[0] = 1.f / (1.f + expf(-sz[0]));
        else {
            float mx = sz[0];
            for (int c = 1; c < C; ++c) mx = fmaxf(mx, sz[c]);
            float e[16], se = 0.f;
            for (int c = 0; c < C; ++c) { e[c] = expf(sz[c] - mx); se += e[c]; }
            for (int c = 0; c < C; ++c) pr[c] = e[c] / se;
        }
    }
}

// one workgroup per sample: dh[n][j] = (sum_c W2[c][j] dl[n][c]) [h > 0], then dpooled[n][k] = sum_j W1[j][k] dh[n][j] (ascending c / j)
__global__ __launch_bounds__(CLS_K) void cls_bwd_data_kernel(const float* __restrict__ dl, const float* __restrict__ w1, const float* __restrict__ w2,
                                                             const float* __restrict__ h, float* __restrict__ dh, float* __restrict__ dpooled, int C) {
    __shared__ float sdh[CLS_H];
    const int t = threadIdx.x, n = blockIdx.x;
    if (t < CLS_H) {
        float acc = 0.f;
        for (int c = 0; c < C; ++c) acc = fmaf(w2[c * CLS_H + t], dl[(long long)n * C + c], acc);
        const float g = h[(long long)n * CLS_H + t] > 0.f ? acc : 0.f;
        sdh[t] = g;
        dh[(long long)n * CLS_H + t] = g;
    }
    __syncthreads();
    float acc = 0.f;
    for (int j = 0; j < CLS_H; ++j) acc = fmaf(w1[j * CLS_K + t], sdh[j], acc);
    dpooled[(long long)n * CLS_K + t] = acc;
}

// parameter gradients: chains over ascending n that start from the value the buffer holds (accumulate) or from 0.
// Workgroups 0 .. 127: row j of dW1 (thread = k) and db1[j]; workgroups 128 .. 127 + C: row c of dW2 and db2[c]
__global__ __launch_bounds__(CLS_K) void cls_bwd_param_kernel(const float* __restrict__ dl, const float* __restrict__ pooled, const float* __restrict__ h,
                                                              const float* __restrict__ dh, float* __restrict__ dw1, float* __restrict__ db1,
                                                              float* __restrict__ dw2, float* __restrict__ db2, int N, int C, int accumulate) {
    const int t = threadIdx.x, b = blockIdx.x;
    if (b < CLS_H) {
        float* o = dw1 + b * CLS_K + t;
        float acc = accumulate ? *o : 0.f;
        for (int n = 0; n < N; ++n) acc = fmaf(dh[(long long)n * CLS_H + b], pooled[(long long)n * CLS_K + t], acc);
        *o = acc;
        if (t == 0) {
            float sb = accumulate ? db1[b] : 0.f;
            for (int n = 0; n < N; ++n) sb += dh[(long long)n * CLS_H + b];
            db1[b] = sb;
        }
    } else {
        const int c = b - CLS_H;
        if (t < CLS_H) {
            float* o = dw2 + c * CLS_H + t;
            float acc = accumulate ? *o : 0.f;
            for (int n = 0; n < N; ++n) acc = fmaf(dl[(long long)n * C + c], h[(long long)n * CLS_H + t], acc);
            *o = acc;
        } else if (t == CLS_H) {
            float sb = accumulate ? db2[c] : 0.f;
            for (int n = 0; n < N; ++n) sb += dl[(long long)n * C + c];
            db2[c] = sb;
        }
    }
}

// dact[n][v][k] = dpooled[n][k] / V for the voxels of one slab
template <class T>
__global__ __launch_bounds__(CLS_K) void cls_bwd_spread_kernel(const float* __restrict__ dpooled, T* __restrict__ dact, long long V) {
    const int k = threadIdx.x, sb = blockIdx.x, n = blockIdx.y;
    const long long v0 = (long long)sb * CLS_SLAB;
    const long long v1 = v0 + CLS_SLAB < V ? v0 + CLS_SLAB : V;
    const T g = from_f<T>(dpooled[(long long)n * CLS_K + k] / (float)V);
    T* p = dact + ((long long)n * V + v0) * CLS_K + k;
    for (long long v = v0; v < v1; ++v, p += CLS_K) *p = g;
}

}  // namespace

size_t cls_head_ws_offset(int N, long long V, int what) {
    const size_t np = ((size_t)N * CLS_K * 4 + 255) / 256 * 256, nh = ((size_t)N * CLS_H * 4 + 255) / 256 * 256;
    const size_t off[6] = {0, np, np + nh, np + 2 * nh, 2 * np + 2 * nh, 2 * np + 2 * nh + (size_t)N * cls_slabs(V) * CLS_K * 8};
    return off[what < 0 ? 0 : what > 5 ? 5 : what];
}
size_t cls_head_ws_bytes(int N, long long V) { return cls_head_ws_offset(N, V, 5); }

void launch_cls_head_fwd(const ClsHeadArgs& a, int dtype, hipStream_t s) {
    const int nslab = cls_slabs(a.V);
    double* slab = (double*)(a.ws + cls_head_ws_offset(a.N, a.V, 4));
    float* pooled = (float*)(a.ws + cls_head_ws_offset(a.N, a.V, 0));
    float* h = (float*)(a.ws + cls_head_ws_offset(a.N, a.V, 1));
    const dim3 grid(nslab, a.N);
    by_dtype(dtype, [&](auto t) {
        using T = tag_type<decltype(t)>;
        hipLaunchKernelGGL(HIP_KERNEL_NAME(cls_pool_kernel<T>), grid, dim3(CLS_K), 0, s, (const T*)a.act, slab, a.V, nslab);
    });
    hipLaunchKernelGGL(cls_fc_fwd_kernel, dim3(a.N), dim3(CLS_K), 0, s, (const double*)slab, nslab, a.V, a.w1, a.b1, a.w2, a.b2, pooled, h, a.logits, a.probs,
                       a.C);
}

void launch_cls_head_bwd(const ClsHeadArgs& a, int dtype, hipStream_t s) {
    const float* pooled = (const float*)(a.ws + cls_head_ws_offset(a.N, a.V, 0));
    const float* h = (const float*)(a.ws + cls_head_ws_offset(a.N, a.V, 1));
    float* dh = (float*)(a.ws + cls_head_ws_offset(a.N, a.V, 2));
    float* dpooled = (float*)(a.ws + cls_head_ws_offset(a.N, a.V, 3));
    hipLaunchKernelGGL(cls_bwd_data_kernel, dim3(a.N), dim3(CLS_K), 0, s, a.dlogits, a.w1, a.w2, h, dh, dpooled, a.C);
    hipLaunchKernelGGL(cls_bwd_param_kernel, dim3(CLS_H + a.C), dim3(CLS_K), 0, s, a.dlogits, pooled, h, (const float*)dh, a.dw1, a.db1, a.dw2, a.db2, a.N,
                       a.C, a.accumulate);
    const dim3 grid(cls_slabs(a.V), a.N);
    by_dtype(dtype, [&](auto t) {
        using T = tag_type<decltype(t)>;
        hipLaunchKernelGGL(HIP_KERNEL_NAME(cls_bwd_spread_kernel<T>), grid, dim3(CLS_K), 0, s, (const float*)dpooled, (T*)a.dact, a.V);
    });
}

}  // namespace seg
