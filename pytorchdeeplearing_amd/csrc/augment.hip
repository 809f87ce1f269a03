// ImageDataGenerator3D of the reference (dataprocess/Augmentation/images_masks_3dtransform.py) on the device: a random affine transform of an image and its
// label volume together (scipy.ndimage.affine_transform with order = 0 per channel there), the three flips, channel shift and rescale.
//
//   aug_gather_kernel   one launch per batch.  A thread produces AG_VEC consecutive voxels of the innermost axis: the source index of each is computed
//                       once, in double and in scipy's summation order, and serves every image channel and the label; the flips are folded into the
//                       store address (a flip of the innermost axis reverses the four values inside the wide store).  Without a channel shift the
//                       rescale is applied here; with one, the extrema of the transformed sample are collected instead: workgroup fold, then one integer
//                       atomicMin / atomicMax per workgroup on an order-preserving image of the float bits, spread over AG_REP replicas per sample
//                       (min / max do not depend on the order of the atomics: deterministic)
//   aug_shift_kernel    in place: clip(x + (float)u_c, min, max) with the folded extrema, then the rescale (random_channel_shift after apply_transform,
//                       then standardize); without parameters only the rescale
//
// Every output value is a copy of an input value (or cval): the comparison with the reference is exact.  No readback, no synchronisation.
#include <math.h>

#include "kernels.h"

// the coordinate sums must round like scipy's C loop: a multiply, then an add - never a fused multiply-add
#pragma clang fp contract(off)

namespace seg {

namespace {

constexpr int AG_BLOCK = 256;
constexpr int AG_VEC = 4;                        // voxels per thread: one 16-byte store of f32
constexpr int AG_REP = AUG_EXTREMA_REP;          // replicas of a sample's extrema: same-address atomics serialise

__device__ __forceinline__ unsigned umin(unsigned a, unsigned b) { return a < b ? a : b; }
__device__ __forceinline__ unsigned umax(unsigned a, unsigned b) { return a > b ? a : b; }

// floats order like these keys as unsigned integers (negative: all bits flipped, non-negative: sign bit set)
__device__ __forceinline__ unsigned f32_key(float f) {
    const unsigned b = __builtin_bit_cast(unsigned, f);
    return (b & 0x80000000u) ? ~b : (b | 0x80000000u);
}
__device__ __forceinline__ float key_f32(unsigned k) { return __builtin_bit_cast(float, (k & 0x80000000u) ? (k & 0x7fffffffu) : ~k); }

// cnt values to cnt consecutive voxels starting at dst (element stride `stride`); rev: the first value goes to the last voxel
template <class T>
__device__ __forceinline__ void store_seg(T* dst, long long stride, const T (&v)[AG_VEC], int cnt, bool rev) {
    if (cnt == AG_VEC && stride == 1 && ((unsigned long long)dst % (sizeof(T) * AG_VEC)) == 0) {
        vec<T, AG_VEC> w;
#pragma unroll
        for (int m = 0; m < AG_VEC; ++m) w[m] = rev ? v[AG_VEC - 1 - m] : v[m];
        *(vec<T, AG_VEC>*)dst = w;
    } else {
#pragma unroll
        for (int m = 0; m < AG_VEC; ++m)
            if (m < cnt) dst[m * stride] = v[rev ? cnt - 1 - m : m];
    }
}

// grid (segments of the sample / AG_BLOCK, N); L: label element type
template <class L>
__global__ __launch_bounds__(AG_BLOCK) void aug_gather_kernel(Augment3dArgs a) {
    __shared__ unsigned sh[2][AG_BLOCK / 64];
    const int n = blockIdx.y;
    const long long t = (long long)blockIdx.x * AG_BLOCK + threadIdx.x;
    const int kseg = (a.n2 + AG_VEC - 1) / AG_VEC;
    float mn = __builtin_inff(), mx = -__builtin_inff();
    if (t < (long long)a.n0 * a.n1 * kseg) {
        const int x0 = (int)(t % kseg) * AG_VEC;
        const long long row = t / kseg;
        const int i1 = (int)(row % a.n1), i0 = (int)(row / a.n1);
        const int cnt = a.n2 - x0 < AG_VEC ? a.n2 - x0 : AG_VEC;
        const double* p = a.params + (size_t)n * AUG_PARAM_DOUBLES;
        const int flips = (int)p[12];
        const int ext[3] = {a.n0, a.n1, a.n2};
        double part[3];                           // the sum over the two outer indices: constant along the row
#pragma unroll
        for (int ax = 0; ax < 3; ++ax) part[ax] = (double)i0 * p[3 * ax] + (double)i1 * p[3 * ax + 1];
        long long src[AG_VEC];                    // linear source voxel, -1: outside (mode constant)
#pragma unroll
        for (int j = 0; j < AG_VEC; ++j) {
            const double i2 = (double)(x0 + j);
            bool outside = false;
            int s[3];
#pragma unroll
            for (int ax = 0; ax < 3; ++ax) {
                double cc = (part[ax] + i2 * p[3 * ax + 2]) + p[9 + ax];
                const double hi = (double)(ext[ax] - 1);
                if (a.constant && (cc < 0.0 || cc > hi)) outside = true;
                cc = cc > 0.0 ? cc : 0.0;         // (a NaN ends at 0)
                cc = cc < hi ? cc : hi;
                int si = (int)floor(cc + 0.5);    // 0 <= cc <= n - 1 < 2^31: the conversion is defined
                si = si < 0 ? 0 : si;
                s[ax] = si > ext[ax] - 1 ? ext[ax] - 1 : si;
            }
            src[j] = outside ? -1 : ((long long)s[0] * a.n1 + s[1]) * a.n2 + s[2];
        }
        const int d0 = (flips & 1) ? a.n0 - 1 - i0 : i0, d1 = (flips & 2) ? a.n1 - 1 - i1 : i1;
        const bool rev = (flips & 4) != 0;
        // the lowest destination voxel of the segment: x0 .. x0 + cnt - 1 land on n2 - 1 - x0 - (cnt - 1) .. n2 - 1 - x0 when the innermost axis is flipped
        const long long dlo = ((long long)d0 * a.n1 + d1) * a.n2 + (rev ? a.n2 - x0 - cnt : x0);
        const long long xbase = (long long)n * a.C * a.V;
        for (int c = 0; c < a.C; ++c) {
            const float* xs = a.x + xbase + c * a.xs_c;
            float v[AG_VEC];
#pragma unroll
            for (int j = 0; j < AG_VEC; ++j) {
                v[j] = (j < cnt && src[j] >= 0) ? xs[src[j] * a.xs_v] : a.cval;
                if (j < cnt) { mn = fminf(mn, v[j]); mx = fmaxf(mx, v[j]); }
                if (a.has_scale) v[j] *= a.scale;
            }
            store_seg(a.out + xbase + c * a.xs_c + dlo * a.xs_v, a.xs_v, v, cnt, rev);
        }
        if (a.label) {
            const long long lbase = (long long)n * a.LC * a.V;
            const L lcval = (L)a.label_cval;
            for (int c = 0; c < a.LC; ++c) {
                const L* ls = (const L*)a.label + lbase + c * a.ls_c;
                L v[AG_VEC];
#pragma unroll
                for (int j = 0; j < AG_VEC; ++j) v[j] = (j < cnt && src[j] >= 0) ? ls[src[j] * a.ls_v] : lcval;
                store_seg((L*)a.label_out + lbase + c * a.ls_c + dlo * a.ls_v, a.ls_v, v, cnt, rev);
            }
        }
    }
    if (a.extrema) {                              // (uniform over the launch: every lane reaches the shuffles and the barrier)
        unsigned kmn = f32_key(mn), kmx = f32_key(mx);
#pragma unroll
        for (int m = 32; m >= 1; m >>= 1) {
            kmn = umin(kmn, __shfl_xor(kmn, m));
            kmx = umax(kmx, __shfl_xor(kmx, m));
        }
        if (lane_id() == 0) { sh[0][wave_id()] = kmn; sh[1][wave_id()] = kmx; }
        __syncthreads();
        if (threadIdx.x == 0) {
            for (int w = 1; w < AG_BLOCK / 64; ++w) { kmn = umin(kmn, sh[0][w]); kmx = umax(kmx, sh[1][w]); }
            const int slot = n * AG_REP + (int)(blockIdx.x % AG_REP);
            atomicMin(a.ws_min + slot, kmn);
            atomicMax(a.ws_max + slot, kmx);
        }
    }
}

// grid (segments of a channel / AG_BLOCK, C, N); in place
__global__ __launch_bounds__(AG_BLOCK) void aug_shift_kernel(float* x, int C, long long V, long long xs_c, long long xs_v, const double* params,
                                                             const unsigned* ws_min, const unsigned* ws_max, float scale, int has_scale) {
    const int c = blockIdx.y, n = blockIdx.z, lane = lane_id();
    float lo = -__builtin_inff(), hi = __builtin_inff(), u = 0.f;
    if (params) {                                 // every wave folds the sample's replicas itself: lanes 0..31 the minima, 32..63 the maxima
        unsigned k = lane < AG_REP ? ws_min[n * AG_REP + lane] : ws_max[n * AG_REP + lane - AG_REP];
#pragma unroll
        for (int m = AG_REP / 2; m >= 1; m >>= 1) {
            const unsigned o = __shfl_xor(k, m);
            k = lane < AG_REP ? umin(k, o) : umax(k, o);
        }
        lo = key_f32(__shfl(k, 0));
        hi = key_f32(__shfl(k, AG_REP));
        u = (float)params[(size_t)n * AUG_PARAM_DOUBLES + 16 + c];
    }
    const long long v0 = ((long long)blockIdx.x * AG_BLOCK + threadIdx.x) * AG_VEC;
    if (v0 >= V) return;
    const int cnt = V - v0 < AG_VEC ? (int)(V - v0) : AG_VEC;
    float* px = x + (long long)n * C * V + c * xs_c + v0 * xs_v;
    float v[AG_VEC];
    const bool wide = cnt == AG_VEC && xs_v == 1 && ((unsigned long long)px % (sizeof(float) * AG_VEC)) == 0;
    if (wide) {
        const f32x4 w = *(const f32x4*)px;
#pragma unroll
        for (int j = 0; j < AG_VEC; ++j) v[j] = w[j];
    } else {
#pragma unroll
        for (int j = 0; j < AG_VEC; ++j) v[j] = j < cnt ? px[j * xs_v] : 0.f;
    }
#pragma unroll
    for (int j = 0; j < AG_VEC; ++j) {
        if (params) v[j] = fminf(fmaxf(v[j] + u, lo), hi);
        if (has_scale) v[j] *= scale;
    }
    store_seg(px, xs_v, v, cnt, false);
}

static_assert(AG_REP * 2 == 64, "aug_shift_kernel folds the replicas of both extrema in one wave");

}  // namespace

size_t augment3d_ws_bytes(int N) { return 2 * (((size_t)N * AG_REP * sizeof(unsigned) + 255) / 256 * 256); }

void launch_augment3d(Augment3dArgs a, int label_type, void* ws, hipStream_t s) {
    const size_t half = augment3d_ws_bytes(a.N) / 2;
    a.ws_min = (unsigned*)ws;
    a.ws_max = (unsigned*)((char*)ws + half);
    if (a.extrema) {
        (void)hipMemsetAsync(a.ws_min, 0xff, half, s);
        (void)hipMemsetAsync(a.ws_max, 0x00, half, s);
    }
    const long long segs = (long long)a.n0 * a.n1 * ((a.n2 + AG_VEC - 1) / AG_VEC);
    const dim3 grid((unsigned)((segs + AG_BLOCK - 1) / AG_BLOCK), (unsigned)a.N);
    switch (label_type) {
        case LT_U8: hipLaunchKernelGGL(aug_gather_kernel<unsigned char>, grid, dim3(AG_BLOCK), 0, s, a); break;
        case LT_I64: hipLaunchKernelGGL(aug_gather_kernel<long long>, grid, dim3(AG_BLOCK), 0, s, a); break;
        default: hipLaunchKernelGGL(aug_gather_kernel<float>, grid, dim3(AG_BLOCK), 0, s, a); break;
    }
}

void launch_augment3d_shift(float* x, int N, int C, long long V, long long xs_c, long long xs_v, const double* params, const void* ws, float scale,
                            int has_scale, hipStream_t s) {
    const unsigned* ws_min = (const unsigned*)ws;
    const unsigned* ws_max = ws ? (const unsigned*)((const char*)ws + augment3d_ws_bytes(N) / 2) : nullptr;      // (no workspace without a shift)
    const dim3 grid((unsigned)(((V + AG_VEC - 1) / AG_VEC + AG_BLOCK - 1) / AG_BLOCK), (unsigned)C, (unsigned)N);
    hipLaunchKernelGGL(aug_shift_kernel, grid, dim3(AG_BLOCK), 0, s, x, C, V, xs_c, xs_v, params, ws_min, ws_max, scale, has_scale);
}

}  // namespace seg
