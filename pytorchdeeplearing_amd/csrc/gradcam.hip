// Grad-CAM of the classifiers (model/visualization.py:135-193 of the reference: get_cam_weights, get_cam_image, compute_cam_per_layer, scale_cam_image,
// aggregate_multi_layers) on the engine's channels-last tensors, and the export of a feature tap (seg_feature_read).  Per sample n and layer:
//   w[c]   = mean_v g[n][v][c] / loss scale                         fp64 slab sums (one workgroup per GC_SLAB voxels), folded over ascending slabs
//   cam[v] = max(0, sum_c w[c] a[n][v][c])                          fp32 fmaf chain; a lane group per voxel reads its channels contiguously
//   s      = (cam - min) / (1e-7 + (max - min))                     min / max over the sample: per-workgroup partials, folded by their readers
//   out   += weight * resize(s)                                     linear, half-pixel centres, clamped edges (cv2 INTER_LINEAR / trilinear)
// and after the last layer out = minmax(max(0, out)) per sample.  2-D is the 3-D case with one plane (the depth taps then have weight 0 exactly).
// Nothing is read back, no grid depends on data and there are no floating-point atomics: every sum has a fixed order (min and max have none to fix:
// they are exact), so two calls on the same input agree bit for bit.
#include <cmath>

#include "kernels.h"
#include "dispatch.h"

namespace seg {

namespace {

constexpr int GC_T = 256;      // threads per workgroup

inline int gc_slabs(long long V) { return (int)((V + GC_SLAB - 1) / GC_SLAB); }
inline int gc_oslabs(long long OV) { return (int)((OV + GC_OSLAB - 1) / GC_OSLAB); }

// the xor butterfly of wave_sum / wave_sum_d over the masks lo .. hi / 2 only: the sum over the lanes that differ in those bits (lo = 1, hi = 64: the wave)
template <class F> __device__ __forceinline__ F lanes_sum(F v, int lo, int hi) {
    for (int m = hi >> 1; m >= lo; m >>= 1) v += __shfl_xor(v, m);
    return v;
}

// min and max over the workgroup, in every thread.  Exact operations: the result does not depend on the order
__device__ __forceinline__ void block_minmax(float& mn, float& mx) {
    __shared__ float sm[GC_T / 64][2];
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) {
        mn = fminf(mn, __shfl_xor(mn, m));
        mx = fmaxf(mx, __shfl_xor(mx, m));
    }
    if (lane_id() == 0) { sm[wave_id()][0] = mn; sm[wave_id()][1] = mx; }
    __syncthreads();
    mn = fminf(fminf(sm[0][0], sm[1][0]), fminf(sm[2][0], sm[3][0]));
    mx = fmaxf(fmaxf(sm[0][1], sm[1][1]), fmaxf(sm[2][1], sm[3][1]));
    __syncthreads();
}
// ... over `count` {min, max} partials left by the workgroups of an earlier launch
__device__ __forceinline__ void fold_minmax(const float* __restrict__ mm, int count, float& mn, float& mx) {
    mn = INFINITY; mx = -INFINITY;
    for (int i = threadIdx.x; i < count; i += GC_T) {
        mn = fminf(mn, mm[2 * i]);
        mx = fmaxf(mx, mm[2 * i + 1]);
    }
    block_minmax(mn, mx);
}

// scale_cam_image (visualization.py:183-187): the one definition of the min-max scaling (per layer and of the aggregate)
__device__ __forceinline__ float minmax_scale(float v, float mn, float mx) { return (v - mn) / (1e-7f + (mx - mn)); }
__device__ __forceinline__ float relu(float v) { return v > 0.f ? v : 0.f; }      // +0 for -0, negatives and NaN

// Linear resize along one axis, the one definition of the interpolation weights: output index o of `out` samples of an axis with `in` samples reads
// i0 and i1 with weights 1 - w1 and w1; source coordinate (o + 0.5) * in / out - 0.5, clamped to the axis (cv2 INTER_LINEAR as published; equal to
// F.interpolate(mode = "bilinear" / "trilinear", align_corners = False) when enlarging).  in == out: i0 = o, w1 = 0; in == 1: i0 = i1 = 0, w1 = 0.
struct LinTap { int i0, i1; float w1; };
__device__ __forceinline__ LinTap lin_tap(int o, int in, int out) {
    const float f = (float)(((double)o + 0.5) * ((double)in / (double)out) - 0.5);
    LinTap t;
    t.i0 = (int)floorf(f);
    t.w1 = f - (float)t.i0;
    if (t.i0 < 0) { t.i0 = 0; t.w1 = 0.f; }
    if (t.i0 >= in - 1) { t.i0 = in - 1; t.w1 = 0.f; }
    t.i1 = t.i0 + 1 < in ? t.i0 + 1 : in - 1;
    return t;
}
__device__ __forceinline__ float lerp(float a, float b, float w1) { return a * (1.f - w1) + b * w1; }

// part[n][sb][c] = sum over the voxels of slab sb of (g0 + g1 + g2)[n][v][c] in fp64.  Thread t holds the 8 channels 8 * (t % cg) .. + 7 (cg = C / 8 lanes
// per voxel, so a wave reads 64 / cg whole rows) and adds its voxels v0 + t / cg, + GC_T / cg, ... in ascending order; then the butterfly over the lanes of
// a wave that hold the same channels, then the four waves in ascending order.
template <class T>
__global__ __launch_bounds__(GC_T) void gc_wpart_kernel(const T* __restrict__ g0, const T* __restrict__ g1, const T* __restrict__ g2,
                                                        double* __restrict__ part, long long V, int C, int nslab) {
    __shared__ double sw[GC_T / 64][256];
    const int t = threadIdx.x, cg = C >> 3, cq = t & (cg - 1), vstep = GC_T / cg;
    const int sb = blockIdx.x, n = blockIdx.y;
    const long long v0 = (long long)sb * GC_SLAB;
    const long long v1 = v0 + GC_SLAB < V ? v0 + GC_SLAB : V;
    double s[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) s[j] = 0.0;
    for (long long v = v0 + t / cg; v < v1; v += vstep) {
        const long long o = ((long long)n * V + v) * C + 8 * cq;
        const vec<T, 8> a = load8(g0 + o);
#pragma unroll
        for (int j = 0; j < 8; ++j) s[j] += (double)to_f(a[j]);
        if (g1) {
            const vec<T, 8> b = load8(g1 + o);
#pragma unroll
            for (int j = 0; j < 8; ++j) s[j] += (double)to_f(b[j]);
        }
        if (g2) {
            const vec<T, 8> b = load8(g2 + o);
#pragma unroll
            for (int j = 0; j < 8; ++j) s[j] += (double)to_f(b[j]);
        }
    }
#pragma unroll
    for (int j = 0; j < 8; ++j) s[j] = lanes_sum(s[j], cg, 64);
    if (lane_id() < cg) {
#pragma unroll
        for (int j = 0; j < 8; ++j) sw[wave_id()][8 * cq + j] = s[j];
    }
    __syncthreads();
    if (t < C) part[((long long)n * nslab + sb) * C + t] = ((sw[0][t] + sw[1][t]) + sw[2][t]) + sw[3][t];
}

// w[n][c] = (sum over ascending slabs) / V * inv_scale; thread = channel
__global__ __launch_bounds__(GC_T) void gc_wfold_kernel(const double* __restrict__ part, float* __restrict__ w, long long V, int C, int nslab, float inv_scale) {
    const int c = threadIdx.x, n = blockIdx.x;
    if (c >= C) return;
    double s = 0.0;
    for (int i = 0; i < nslab; ++i) s += part[((long long)n * nslab + i) * C + c];
    w[(long long)n * C + c] = (float)(s / (double)V * (double)inv_scale);
}

// cam[n][v] = max(0, sum_c w[n][c] act[n][v][c]) for the voxels of one slab, and the slab's {min, max}.  The thread layout of gc_wpart_kernel: a lane
// keeps its 8 weights in registers, multiplies them into its 8 channels of a voxel (fp32 fmaf chain), the butterfly over the cg lanes of the voxel adds up.
// Every lane runs every pass (the butterfly needs the whole wave); the passes past the end of a ragged slab are skipped by the whole workgroup.
template <class T>
__global__ __launch_bounds__(GC_T) void gc_cam_kernel(const T* __restrict__ act, const float* __restrict__ w, float* __restrict__ cam,
                                                      float* __restrict__ mm, long long V, int C, int nslab) {
    const int t = threadIdx.x, cg = C >> 3, cq = t & (cg - 1), vstep = GC_T / cg;
    const int sb = blockIdx.x, n = blockIdx.y;
    const long long v0 = (long long)sb * GC_SLAB;
    const long long v1 = v0 + GC_SLAB < V ? v0 + GC_SLAB : V;
    float wr[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) wr[j] = w[(long long)n * C + 8 * cq + j];
    float mn = INFINITY, mx = -INFINITY;
    for (long long vb = v0; vb < v1; vb += vstep) {
        const long long v = vb + t / cg;
        const bool in = v < v1;
        float acc = 0.f;
        if (in) {
            const vec<T, 8> a = load8(act + ((long long)n * V + v) * C + 8 * cq);
#pragma unroll
            for (int j = 0; j < 8; ++j) acc = fmaf(wr[j], to_f(a[j]), acc);
        }
        acc = relu(lanes_sum(acc, 1, cg));
        if (in) {
            if (cq == 0) cam[(long long)n * V + v] = acc;
            mn = fminf(mn, acc);
            mx = fmaxf(mx, acc);
        }
    }
    block_minmax(mn, mx);
    if (t == 0) {
        mm[2 * ((long long)n * nslab + sb)] = mn;
        mm[2 * ((long long)n * nslab + sb) + 1] = mx;
    }
}

// out[n][o] (+)= weight * resize(minmax(cam[n]))[o] for GC_OSLAB output voxels; finalize: also the {min, max} of max(0, out) over them
__global__ __launch_bounds__(GC_T) void gc_resize_kernel(const float* __restrict__ cam, const float* __restrict__ mm, int nslab, float* __restrict__ out,
                                                         float* __restrict__ fm, int ID, int IH, int IW, int OD, int OH, int OW, float weight,
                                                         int accumulate, int finalize) {
    const int t = threadIdx.x, n = blockIdx.y;
    const long long IV = (long long)ID * IH * IW, OV = (long long)OD * OH * OW;
    float mn, mx;
    fold_minmax(mm + 2 * (long long)n * nslab, nslab, mn, mx);
    const float* cn = cam + (long long)n * IV;
    float fmn = INFINITY, fmx = -INFINITY;
    for (int i = 0; i < GC_OSLAB / GC_T; ++i) {
        const long long o = (long long)blockIdx.x * GC_OSLAB + i * GC_T + t;
        if (o >= OV) break;
        const LinTap tx = lin_tap((int)(o % OW), IW, OW), ty = lin_tap((int)(o / OW % OH), IH, OH), tz = lin_tap((int)(o / ((long long)OW * OH)), ID, OD);
        float plane[2];
#pragma unroll
        for (int p = 0; p < 2; ++p) {
            const float* cz = cn + (long long)(p ? tz.i1 : tz.i0) * IH * IW;
            const float* r0 = cz + (long long)ty.i0 * IW;
            const float* r1 = cz + (long long)ty.i1 * IW;
            const float h0 = lerp(minmax_scale(r0[tx.i0], mn, mx), minmax_scale(r0[tx.i1], mn, mx), tx.w1);
            const float h1 = lerp(minmax_scale(r1[tx.i0], mn, mx), minmax_scale(r1[tx.i1], mn, mx), tx.w1);
            plane[p] = lerp(h0, h1, ty.w1);
        }
        float* po = out + (long long)n * OV + o;
        float a = weight * lerp(plane[0], plane[1], tz.w1);
        if (accumulate) a += *po;
        *po = a;
        fmn = fminf(fmn, relu(a));
        fmx = fmaxf(fmx, relu(a));
    }
    if (finalize) {
        block_minmax(fmn, fmx);
        if (t == 0) {
            fm[2 * ((long long)n * gridDim.x + blockIdx.x)] = fmn;
            fm[2 * ((long long)n * gridDim.x + blockIdx.x) + 1] = fmx;
        }
    }
}

// aggregate_multi_layers (visualization.py:176-180): out = minmax(max(0, out)) per sample
__global__ __launch_bounds__(GC_T) void gc_final_kernel(float* __restrict__ out, const float* __restrict__ fm, int nblk, long long OV) {
    const int t = threadIdx.x, n = blockIdx.y;
    float mn, mx;
    fold_minmax(fm + 2 * (long long)n * nblk, nblk, mn, mx);
    for (int i = 0; i < GC_OSLAB / GC_T; ++i) {
        const long long o = (long long)blockIdx.x * GC_OSLAB + i * GC_T + t;
        if (o >= OV) break;
        float* po = out + (long long)n * OV + o;
        *po = minmax_scale(relu(*po), mn, mx);
    }
}

// out[n][c][v] = scale * (s0 + s1 + s2)[n][v][c]: a tile of 64 voxels x 16 channels goes through the LDS - the reads follow the channels-last rows
// (4 channels per thread), the writes the planar rows (64 consecutive voxels per channel)
template <class T>
__global__ __launch_bounds__(GC_T) void feature_unpack_kernel(const T* __restrict__ s0, const T* __restrict__ s1, const T* __restrict__ s2,
                                                              float* __restrict__ out, long long V, int C, float scale) {
    __shared__ float tile[16][65];
    const int t = threadIdx.x, n = blockIdx.z, c0 = blockIdx.y * 16;
    const long long v0 = (long long)blockIdx.x * 64;
    {
        const int vl = t >> 2, cq = (t & 3) * 4;
        if (v0 + vl < V) {
            const long long o = ((long long)n * V + v0 + vl) * C + c0 + cq;
            const vec<T, 4> a = *(const vec<T, 4>*)(s0 + o);
            float f[4];
#pragma unroll
            for (int j = 0; j < 4; ++j) f[j] = to_f(a[j]);
            if (s1) {
                const vec<T, 4> b = *(const vec<T, 4>*)(s1 + o);
#pragma unroll
                for (int j = 0; j < 4; ++j) f[j] += to_f(b[j]);
            }
            if (s2) {
                const vec<T, 4> b = *(const vec<T, 4>*)(s2 + o);
#pragma unroll
                for (int j = 0; j < 4; ++j) f[j] += to_f(b[j]);
            }
#pragma unroll
            for (int j = 0; j < 4; ++j) tile[cq + j][vl] = f[j] * scale;
        }
    }
    __syncthreads();
    const int vl = t & 63;
    if (v0 + vl < V) {
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int c = (t >> 6) + 4 * i;
            out[((long long)n * C + c0 + c) * V + v0 + vl] = tile[c][vl];
        }
    }
}

// workspace: 0 slab sums fp64 [N][slabs][C], 1 w [N][C], 2 cam [N][V], 3 slab {min, max} [N][slabs][2], 4 output-slab {min, max} [N][oslabs][2], 5 the end
size_t gc_ws_offset(int N, int C, long long V, long long OV, int what) {
    const size_t ns = (size_t)N * gc_slabs(V);
    const size_t bytes[5] = {ns * C * 8, (size_t)N * C * 4, (size_t)N * V * 4, ns * 2 * 4, (size_t)N * gc_oslabs(OV) * 2 * 4};
    size_t off = 0;
    for (int i = 0; i < what; ++i) off += (bytes[i] + 255) / 256 * 256;
    return off;
}

}  // namespace

size_t gradcam_ws_bytes(int N, int C, long long V, long long OV) { return gc_ws_offset(N, C, V, OV, 5); }

void launch_gradcam_layer(const GradCamArgs& a, int dtype, hipStream_t s) {
    const long long V = (long long)a.ID * a.IH * a.IW, OV = (long long)a.OD * a.OH * a.OW;
    const int nslab = gc_slabs(V), nblk = gc_oslabs(OV);
    double* part = (double*)(a.ws + gc_ws_offset(a.N, a.C, V, OV, 0));
    float* w = (float*)(a.ws + gc_ws_offset(a.N, a.C, V, OV, 1));
    float* cam = (float*)(a.ws + gc_ws_offset(a.N, a.C, V, OV, 2));
    float* mm = (float*)(a.ws + gc_ws_offset(a.N, a.C, V, OV, 3));
    float* fm = (float*)(a.ws + gc_ws_offset(a.N, a.C, V, OV, 4));
    const dim3 grid(nslab, a.N);
    by_dtype(dtype, [&](auto t) {
        using T = tag_type<decltype(t)>;
        hipLaunchKernelGGL(HIP_KERNEL_NAME(gc_wpart_kernel<T>), grid, dim3(GC_T), 0, s, (const T*)a.grad[0], (const T*)(a.ngrad > 1 ? a.grad[1] : nullptr),
                           (const T*)(a.ngrad > 2 ? a.grad[2] : nullptr), part, V, a.C, nslab);
    });
    hipLaunchKernelGGL(gc_wfold_kernel, dim3(a.N), dim3(GC_T), 0, s, (const double*)part, w, V, a.C, nslab, a.inv_scale);
    by_dtype(dtype, [&](auto t) {
        using T = tag_type<decltype(t)>;
        hipLaunchKernelGGL(HIP_KERNEL_NAME(gc_cam_kernel<T>), grid, dim3(GC_T), 0, s, (const T*)a.act, (const float*)w, cam, mm, V, a.C, nslab);
    });
    hipLaunchKernelGGL(gc_resize_kernel, dim3(nblk, a.N), dim3(GC_T), 0, s, (const float*)cam, (const float*)mm, nslab, a.out, fm, a.ID, a.IH, a.IW, a.OD,
                       a.OH, a.OW, a.weight, a.accumulate, a.finalize);
    if (a.finalize) hipLaunchKernelGGL(gc_final_kernel, dim3(nblk, a.N), dim3(GC_T), 0, s, a.out, (const float*)fm, nblk, OV);
}

void launch_feature_unpack(const void* const* src, int nsrc, float* out, int N, int C, long long V, float scale, int dtype, hipStream_t s) {
    const dim3 grid((unsigned)((V + 63) / 64), C / 16, N);
    by_dtype(dtype, [&](auto t) {
        using T = tag_type<decltype(t)>;
        hipLaunchKernelGGL(HIP_KERNEL_NAME(feature_unpack_kernel<T>), grid, dim3(GC_T), 0, s, (const T*)src[0], (const T*)(nsrc > 1 ? src[1] : nullptr),
                           (const T*)(nsrc > 2 ? src[2] : nullptr), out, V, C, scale);
    });
}

}  // namespace seg
