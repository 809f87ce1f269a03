// Segmenation_Aug of the reference (dataprocess/AugData.py: an albumentations Compose of flips, one of three blurs, shift-scale-rotate and brightness /
// contrast) on the device, for a batch of 2-D images and their label images in ONE launch.  The arithmetic is the contract written down at seg_augment2d in
// include/segengine.h (it is NOT pinned to an albumentations / cv2 version: neither can run here, and their draw order and uint8 fixed-point interpolation
// differ between their own versions); tests/aug2d_oracle.py restates it in float64 numpy.
//
//   aug2d_kernel   grid (segments of a sample / A2_BLOCK, N): a workgroup belongs to one sample, so the sample's parameter block - which steps run - is
//                  uniform over the workgroup and chosen ONCE, in front of the pixel work.  A thread produces A2_VEC consecutive pixels of a row for every
//                  channel and the label.  All steps are gathers on the stored input: out(y, x) interpolates the blurred image G at (at most) four
//                  taps, G correlates the flipped image F with the kernel's non-zero weights, F reads the source at the flipped position; nothing
//                  intermediate goes to memory.
//                  copy path (no blur, no warp): 16-byte loads and stores; a horizontal flip reads the mirrored segment and reverses it in registers.
//                  blur weights: wave 0 compacts the k*k weights of the block into a list of the non-zero taps in LDS (a motion kernel has at most k of
//                  k*k), in row-major order.
#include <math.h>

#include "kernels.h"

// the coordinate sums round as the contract says: a multiply, then an add - never a fused multiply-add
#pragma clang fp contract(off)

namespace seg {

namespace {

constexpr int A2_BLOCK = 256;
constexpr int A2_VEC = 4;                        // pixels per thread: one 16-byte store of f32
constexpr int A2_MAXTAP = 49;                    // 7 x 7

// mirror without the edge pixel (d c b | a b c d): period 2(n - 1), 0 for n == 1; any i
__device__ __forceinline__ int fold_mirror(long long i, int n) {
    if (i >= 0 && i < n) return (int)i;
    if (n == 1) return 0;
    const long long period = 2ll * (n - 1);
    long long m = i % period;
    if (m < 0) m += period;
    return (int)(m > n - 1 ? period - m : m);
}

// the same for an integer-valued double however far out (fmod is exact)
__device__ __forceinline__ int fold_mirror(double i, int n) {
    const double hi = (double)(n - 1);
    if (i >= 0.0 && i <= hi) return (int)i;
    if (n == 1) return 0;
    const double period = 2.0 * hi;
    double m = fmod(i, period);
    if (m < 0.0) m += period;
    if (m > hi) m = period - m;
    const int r = (int)m;                         // 0 <= m <= n - 1
    return r < 0 ? 0 : (r > n - 1 ? n - 1 : r);
}

// source index of the integer-valued coordinate i on an axis of n pixels; -1: outside (mode constant)
__device__ __forceinline__ int border_index(double i, int n, int border) {
    const double hi = (double)(n - 1);
    if (i >= 0.0 && i <= hi) return (int)i;
    if (border == SEG_AUGMENT_CONSTANT) return -1;
    if (border == SEG_AUGMENT_NEAREST) return i < 0.0 ? 0 : n - 1;
    return fold_mirror(i, n);
}

__device__ __forceinline__ double finite_or_zero(double v) { return fabs(v) <= 1.7e308 ? v : 0.0; }      // (an overflowed sum or a NaN reads pixel 0)

// one plane of one sample behind the flip: F(y, x)
template <class T>
struct Flipped {
    const T* p;
    long long xs_v;
    int h, w;
    bool vf, hf;
    __device__ __forceinline__ T at(int y, int x) const {
        const int yy = vf ? h - 1 - y : y, xx = hf ? w - 1 - x : x;
        return p[((long long)yy * w + xx) * xs_v];
    }
};

struct TapList {                                  // the non-zero weights of the blur kernel (LDS), offsets from the anchor
    const float* w;
    const int* dy;
    const int* dx;
    int n;
};

__device__ __forceinline__ void order2(float& a, float& b) {           // a selection, no arithmetic
    const float lo = b < a ? b : a, hi = b < a ? a : b;
    a = lo; b = hi;
}

// BLUR 0: F itself; 1: correlation with the tap list, mirror indexing, f32 accumulation; 2: 3 x 3 median, replicated edges
template <int BLUR>
__device__ __forceinline__ float blurred(const Flipped<float>& f, const TapList& taps, int y, int x) {
    if (BLUR == 0) return f.at(y, x);
    if (BLUR == 1) {
        float acc = 0.f;
        for (int t = 0; t < taps.n; ++t)
            acc += taps.w[t] * f.at(fold_mirror((long long)y + taps.dy[t], f.h), fold_mirror((long long)x + taps.dx[t], f.w));
        return acc;
    }
    float v[9];
#pragma unroll
    for (int j = 0; j < 3; ++j) {
        int yy = y + j - 1;
        yy = yy < 0 ? 0 : (yy > f.h - 1 ? f.h - 1 : yy);
#pragma unroll
        for (int i = 0; i < 3; ++i) {
            int xx = x + i - 1;
            xx = xx < 0 ? 0 : (xx > f.w - 1 ? f.w - 1 : xx);
            v[3 * j + i] = f.at(yy, xx);
        }
    }
    // the 19-exchange median-of-nine network
    order2(v[1], v[2]); order2(v[4], v[5]); order2(v[7], v[8]); order2(v[0], v[1]); order2(v[3], v[4]); order2(v[6], v[7]);
    order2(v[1], v[2]); order2(v[4], v[5]); order2(v[7], v[8]); order2(v[0], v[3]); order2(v[5], v[8]); order2(v[4], v[7]);
    order2(v[3], v[6]); order2(v[1], v[4]); order2(v[2], v[5]); order2(v[4], v[7]); order2(v[4], v[2]); order2(v[6], v[4]);
    order2(v[4], v[2]);
    return v[4];
}

// cnt values to cnt consecutive pixels starting at dst (element stride `stride`)
template <class T>
__device__ __forceinline__ void store_seg(T* dst, long long stride, const T (&v)[A2_VEC], int cnt) {
    if (cnt == A2_VEC && stride == 1 && ((unsigned long long)dst % (sizeof(T) * A2_VEC)) == 0) {
        vec<T, A2_VEC> w;
#pragma unroll
        for (int m = 0; m < A2_VEC; ++m) w[m] = v[m];
        *(vec<T, A2_VEC>*)dst = w;
    } else {
#pragma unroll
        for (int m = 0; m < A2_VEC; ++m)
            if (m < cnt) dst[m * stride] = v[m];
    }
}

// cnt consecutive pixels starting at src into v; rev: the first pixel read becomes the last value
template <class T>
__device__ __forceinline__ void load_seg(const T* src, long long stride, T (&v)[A2_VEC], int cnt, bool rev) {
    if (cnt == A2_VEC && stride == 1 && ((unsigned long long)src % (sizeof(T) * A2_VEC)) == 0) {
        const vec<T, A2_VEC> w = *(const vec<T, A2_VEC>*)src;
#pragma unroll
        for (int m = 0; m < A2_VEC; ++m) v[m] = rev ? w[A2_VEC - 1 - m] : w[m];
    } else {
#pragma unroll
        for (int m = 0; m < A2_VEC; ++m)
            if (m < cnt) v[m] = src[(rev ? cnt - 1 - m : m) * stride];
    }
}

struct Tone {                                     // brightness / contrast and the clip of one sample
    float alpha, beta, lo, hi;
    bool affine, clip;
    __device__ __forceinline__ float run(float v) const {
        if (affine) v = alpha * v + beta;
        if (clip) v = fminf(fmaxf(v, lo), hi);
        return v;
    }
};

struct Pixel {                                    // where the segment lies
    int s, y, x0, cnt;
};

// no blur and no warp: every value is moved (and toned); wide loads and stores
template <class L>
__device__ __forceinline__ void copy_segment(const Augment2dArgs& a, const Pixel& px, bool vf, bool hf, const Tone& tone) {
    const int ys = vf ? a.H - 1 - px.y : px.y;
    const int xs = hf ? a.W - px.x0 - px.cnt : px.x0;     // the lowest source pixel of the segment
    const long long src = (long long)ys * a.W + xs, dst = (long long)px.y * a.W + px.x0;
    for (int c = 0; c < a.C; ++c) {
        float v[A2_VEC];
        load_seg(a.x + px.s * a.xs_n + c * a.xs_c + src * a.xs_v, a.xs_v, v, px.cnt, hf);
        if (tone.affine || tone.clip) {
#pragma unroll
            for (int j = 0; j < A2_VEC; ++j) v[j] = tone.run(v[j]);
        }
        store_seg(a.out + (long long)px.s * a.C * a.V + c * a.xs_c + dst * a.xs_v, a.xs_v, v, px.cnt);
    }
    if (a.label) {
        L v[A2_VEC];
        load_seg((const L*)a.label + px.s * a.ls_n + src, 1, v, px.cnt, hf);
        store_seg((L*)a.label_out + (long long)px.s * a.V + dst, 1, v, px.cnt);
    }
}

struct Taps {                                     // the bilinear taps of one output pixel and its label pixel; an index of -1: outside (mode constant)
    int iy[2], ix[2], ly, lx;
    float wy, wx;
};

template <bool WARP>
__device__ __forceinline__ Taps taps_of(const Augment2dArgs& a, const double* p, int yo, int xo) {
    Taps t;
    if (WARP) {
        const double y = (double)yo, x = (double)xo;
        const double sy = finite_or_zero((y * p[0] + x * p[1]) + p[2]), sx = finite_or_zero((y * p[3] + x * p[4]) + p[5]);
        const double fy = floor(sy), fx = floor(sx);
        t.wy = (float)(sy - fy); t.wx = (float)(sx - fx);
        t.iy[0] = border_index(fy, a.H, a.border); t.iy[1] = border_index(fy + 1.0, a.H, a.border);
        t.ix[0] = border_index(fx, a.W, a.border); t.ix[1] = border_index(fx + 1.0, a.W, a.border);
        t.ly = border_index(floor(sy + 0.5), a.H, a.border); t.lx = border_index(floor(sx + 0.5), a.W, a.border);
    } else {
        t.iy[0] = t.iy[1] = t.ly = yo;
        t.ix[0] = t.ix[1] = t.lx = xo < a.W ? xo : a.W - 1;          // (a lane past the row end computes a value nobody stores)
        t.wy = t.wx = 0.f;
    }
    return t;
}

// v[j] = val with j a loop variable: selects, so that v stays in registers
template <class T>
__device__ __forceinline__ void put(T (&v)[A2_VEC], int j, T val) {
#pragma unroll
    for (int m = 0; m < A2_VEC; ++m) v[m] = m == j ? val : v[m];
}

// The pixels of a segment are produced one after the other (the loops over j are NOT unrolled): a pixel of the median under a warp holds 36 loaded
// values, four of them at once would take the kernel - and with it the copy path - down to one wave per SIMD.  The coordinates of a pixel are
// recomputed per plane instead of being kept for all four pixels, for the same reason.
template <class L, int BLUR, bool WARP>
__device__ __forceinline__ void gather_segment(const Augment2dArgs& a, const double* p, const Pixel& px, bool vf, bool hf, const TapList& taps,
                                               const Tone& tone) {
    const long long dst = (long long)px.y * a.W + px.x0;
    for (int c = 0; c < a.C; ++c) {
        const Flipped<float> f = {a.x + px.s * a.xs_n + c * a.xs_c, a.xs_v, a.H, a.W, vf, hf};
        float v[A2_VEC] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll 1
        for (int j = 0; j < A2_VEC; ++j) {
            const Taps t = taps_of<WARP>(a, p, px.y, px.x0 + j);
            float val;
            if (WARP) {
                float g[2][2];
#pragma unroll
                for (int r = 0; r < 2; ++r)
#pragma unroll
                    for (int q = 0; q < 2; ++q) g[r][q] = (t.iy[r] < 0 || t.ix[q] < 0) ? a.cval : blurred<BLUR>(f, taps, t.iy[r], t.ix[q]);
                const float top = (1.f - t.wx) * g[0][0] + t.wx * g[0][1], bot = (1.f - t.wx) * g[1][0] + t.wx * g[1][1];
                val = (1.f - t.wy) * top + t.wy * bot;
            } else {
                val = blurred<BLUR>(f, taps, t.iy[0], t.ix[0]);
            }
            put(v, j, tone.run(val));
        }
        store_seg(a.out + (long long)px.s * a.C * a.V + c * a.xs_c + dst * a.xs_v, a.xs_v, v, px.cnt);
    }
    if (a.label) {
        const Flipped<L> f = {(const L*)a.label + px.s * a.ls_n, 1, a.H, a.W, vf, hf};
        const L lcval = (L)a.label_cval;
        L v[A2_VEC] = {};
#pragma unroll 1
        for (int j = 0; j < A2_VEC; ++j) {
            const Taps t = taps_of<WARP>(a, p, px.y, px.x0 + j);
            put(v, j, (t.ly < 0 || t.lx < 0) ? lcval : f.at(t.ly, t.lx));
        }
        store_seg((L*)a.label_out + (long long)px.s * a.V + dst, 1, v, px.cnt);
    }
}

// grid (segments of the sample / A2_BLOCK, N); L: label element type
template <class L>
__global__ __launch_bounds__(A2_BLOCK) void aug2d_kernel(Augment2dArgs a) {
    __shared__ float tap_w[A2_MAXTAP];
    __shared__ int tap_dy[A2_MAXTAP], tap_dx[A2_MAXTAP];
    __shared__ int tap_n;
    const int s = blockIdx.y;
    const double* p = a.params + (size_t)s * AUG2D_PARAM_DOUBLES;
    const int flips = (int)p[6], blur = (int)p[8];
    const bool warp = p[7] != 0.0;
    if (blur == 1) {                              // (uniform over the workgroup: every wave reaches the barrier)
        if (wave_id() == 0) {
            const int k = (int)p[9], lane = lane_id();
            const float wgt = lane < k * k ? (float)p[lane < 48 ? 16 + lane : 15] : 0.f;      // (weight 48 of a 7 x 7 kernel: slot 15)
            const unsigned long long mask = __ballot(wgt != 0.f);
            if (wgt != 0.f) {
                const int slot = __builtin_popcountll(mask & ((1ull << lane) - 1ull));
                tap_w[slot] = wgt;
                tap_dy[slot] = lane / k - k / 2;
                tap_dx[slot] = lane % k - k / 2;
            }
            if (lane == 0) tap_n = __builtin_popcountll(mask);
        }
        __syncthreads();
    }
    const long long t = (long long)blockIdx.x * A2_BLOCK + threadIdx.x;
    const int kseg = (a.W + A2_VEC - 1) / A2_VEC;
    if (t >= (long long)a.H * kseg) return;
    Pixel px;
    px.s = s; px.y = (int)((unsigned)t / (unsigned)kseg); px.x0 = (int)((unsigned)t % (unsigned)kseg) * A2_VEC;      // (t < h*kseg <= 2^31)
    px.cnt = a.W - px.x0 < A2_VEC ? a.W - px.x0 : A2_VEC;
    const bool hf = (flips & 1) != 0, vf = (flips & 2) != 0;
    Tone tone;
    tone.alpha = (float)p[10]; tone.beta = (float)p[11]; tone.lo = (float)p[13]; tone.hi = (float)p[14];
    tone.affine = !(p[10] == 1.0 && p[11] == 0.0); tone.clip = p[12] != 0.0;
    TapList taps = {tap_w, tap_dy, tap_dx, 0};
    if (blur == 1) taps.n = __builtin_amdgcn_readfirstlane(tap_n);
    // the sample's branch, taken once
    if (!warp) {
        if (blur == 0) copy_segment<L>(a, px, vf, hf, tone);
        else if (blur == 1) gather_segment<L, 1, false>(a, p, px, vf, hf, taps, tone);
        else gather_segment<L, 2, false>(a, p, px, vf, hf, taps, tone);
    } else {
        if (blur == 0) gather_segment<L, 0, true>(a, p, px, vf, hf, taps, tone);
        else if (blur == 1) gather_segment<L, 1, true>(a, p, px, vf, hf, taps, tone);
        else gather_segment<L, 2, true>(a, p, px, vf, hf, taps, tone);
    }
}

}  // namespace

void launch_augment2d(const Augment2dArgs& a, int label_type, hipStream_t s) {
    const long long segs = (long long)a.H * ((a.W + A2_VEC - 1) / A2_VEC);
    const dim3 grid((unsigned)((segs + A2_BLOCK - 1) / A2_BLOCK), (unsigned)a.N);
    switch (label_type) {
        case LT_U8: hipLaunchKernelGGL(aug2d_kernel<unsigned char>, grid, dim3(A2_BLOCK), 0, s, a); break;
        case LT_I64: hipLaunchKernelGGL(aug2d_kernel<long long>, grid, dim3(A2_BLOCK), 0, s, a); break;
        default: hipLaunchKernelGGL(aug2d_kernel<float>, grid, dim3(A2_BLOCK), 0, s, a); break;
    }
}

}  // namespace seg
