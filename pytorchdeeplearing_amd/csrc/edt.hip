// Exact Euclidean distance transform of n independent uint8 volumes [n][d][h][w] (scipy.ndimage.distance_transform_edt's convention: nothing outside the
// volume counts as background) and the boundary loss of Kervadec et al. that consumes its maps.  Separable, linear time per row / column (Meijster,
// Roerdink & Hesselink; Felzenszwalb & Huttenlocher):
//
//   edt_pack_kernel    ballot words of the mask (one 64-bit word per 64 voxels of a row, as postproc.hip packs them) + per sample "has foreground" /
//                      "has background" bits
//   edt_row_kernel     axis x from the words: nearest zero bit to the left and right by clz / ctz across the words of the row -> (dx * sx)^2, or "none"
//   edt_col_kernel     axis y, then axis z: lower envelope of the parabolas (u - i)^2 s^2 + f[i] of one column per LANE, lane index = x, so that every load
//                      and store of a wave is a contiguous row segment.  Forward scan builds the envelope (entries {i, first u it wins at} packed in one
//                      word) on a stack in the workspace laid out like the volume ([k][x]: entry k of a column lies where voxel k of it lies), backward
//                      scan evaluates it.  Columns entries without any background in their row ("none") never enter the envelope; an empty envelope gives
//                      +inf.  The top of the stack is kept in registers; nothing is indexed dynamically in registers, so nothing goes to scratch.
//                      The last axis writes the result in the caller's mode straight into `out` (sample stride out_stride_n).
//
// Unit spacing: every value is an integer (int32, d^2 <= 3 * 2047^2 < 2^24) and the intersection of two parabolas is Meijster's integer Sep - no float
// comparison decides a winner; the f32 written is the exact integer.  Other spacings: f32 values (dx * s)^2 + f, winners compared in f32 on the values
// that would be written, the intersection in double and forced to keep the stack's "first u" strictly increasing, so that every output is the value of a
// true candidate whatever the rounding does.
// SEG_EDT_SIGNED / _BOUNDARY run the passes twice, on the mask and on its complement (a voxel needs only the one it is foreground of); the per sample bits
// give the all-zero map of a sample whose mask is empty or full.
//
// No allocation, no host synchronisation, no grid that depends on the data, no floating-point atomics (one integer atomicOr per wave at most, bits only ever
// set): two calls on the same input agree bit for bit.
#include "kernels.h"

namespace seg {

namespace {

typedef unsigned long long u64;

constexpr int EDT_BLOCK = 256;
constexpr int EDT_WORDS = 8;                     // words a wave of the pack / row kernels walks
constexpr int EDT_COLS = 64;                     // columns (lanes) per workgroup of the column kernel: one wave, so that small volumes spread over the CUs
constexpr int EDT_INF_I = 0x7fffffff;            // "no background in this row / column" of the integer path
constexpr unsigned EDT_HAS_FG = 1u, EDT_HAS_BG = 2u;

struct EdtGeom {
    int n, d, h, w, rw;      // rw: words per row
    unsigned V;              // voxels per sample (< 2^31)
    unsigned wps;            // words per sample: d * h * rw
};

struct EdtWs {
    unsigned* flags;         // [n]       EDT_HAS_FG | EDT_HAS_BG
    u64* bits;               // [n][wps]
    void* a;                 // [n][V]    after axis x (int32 or f32)
    void* b;                 // [n][V]    after axis y
    unsigned* stack;         // [n][V]    envelope entries, i << 16 | first u
};

// relaxed agent-scope load of a flag word another workgroup may be setting bits in (the host checker runs one thread at a time: a plain load)
#ifdef SEG_EMU
#define EDT_FLAG_LOAD(p) (*(p))
#else
#define EDT_FLAG_LOAD(p) __hip_atomic_load((p), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)
#endif

__host__ __device__ inline size_t edt_align(size_t v) { return (v + 255) / 256 * 256; }

inline EdtGeom edt_geom(int n, int d, int h, int w) {
    EdtGeom g;
    g.n = n; g.d = d; g.h = h; g.w = w; g.rw = (w + 63) / 64;
    g.V = (unsigned)d * (unsigned)h * (unsigned)w;
    g.wps = (unsigned)d * (unsigned)h * (unsigned)g.rw;
    return g;
}

inline EdtWs edt_carve(void* ws, const EdtGeom& g) {
    const size_t NV = (size_t)g.n * g.V;
    char* p = (char*)ws;
    EdtWs c;
    c.flags = (unsigned*)p; p += edt_align((size_t)g.n * 4);
    c.bits = (u64*)p; p += edt_align((size_t)g.n * g.wps * 8);
    c.a = p; p += edt_align(NV * 4);
    c.b = p; p += edt_align(NV * 4);
    c.stack = (unsigned*)p;
    return c;
}

// ---- axis x ----------------------------------------------------------------------------------------------------------------------------------------

// grid (words of a sample / words per workgroup, n)
__global__ __launch_bounds__(EDT_BLOCK) void edt_pack_kernel(const unsigned char* labels, EdtGeom g, int cls, u64* bits, unsigned* flags) {
    const int lane = lane_id();
    const unsigned s = blockIdx.y;
    const unsigned first = (blockIdx.x * (EDT_BLOCK / 64) + wave_id()) * EDT_WORDS;
    const unsigned char* vol = labels + (size_t)s * g.V;
    const int tail = g.w & 63;
    unsigned seen = 0u;
    for (int i = 0; i < EDT_WORDS; ++i) {
        const unsigned t = first + i;
        if (t >= g.wps) break;                                 // wave-uniform
        const unsigned row = t / (unsigned)g.rw;
        const int k = (int)(t - row * (unsigned)g.rw), x = k * 64 + lane;
        bool fg = false;
        if (x < g.w) {
            const int v = vol[row * (unsigned)g.w + (unsigned)x];
            fg = cls < 0 ? v != 0 : v == cls;
        }
        const u64 b = __ballot(fg);
        const u64 valid = (k == g.rw - 1 && tail) ? (1ull << tail) - 1ull : ~0ull;
        seen |= (b ? EDT_HAS_FG : 0u) | (b != valid ? EDT_HAS_BG : 0u);
        if (lane == 0) bits[(size_t)s * g.wps + t] = b;
    }
    // bits are only ever set: a stale value read here costs one redundant atomic, never a wrong result
    if (lane == 0 && (seen & ~EDT_FLAG_LOAD(&flags[s])) != 0u) atomicOr(&flags[s], seen);
}

__device__ __forceinline__ void edt_store_row(int* p, int dist, float) { *p = dist < 0 ? EDT_INF_I : dist * dist; }
__device__ __forceinline__ void edt_store_row(float* p, int dist, float sx) {
    const float dx = (float)dist * sx;
    *p = dist < 0 ? __builtin_inff() : dx * dx;
}

// word j of the row as the pass sees it: complemented for the transform of the complement, the padding bits of the last word set (padding is no background)
__device__ __forceinline__ u64 edt_word(const u64* rowbits, int j, int rw, int tail, int inv) {
    u64 v = rowbits[j];
    if (inv) v = ~v;
    if (j == rw - 1 && tail) v |= ~0ull << tail;
    return v;
}

// one wave per word, lane = bit: squared distance along x to the nearest zero bit of the row
template <typename T>
__global__ __launch_bounds__(EDT_BLOCK) void edt_row_kernel(const u64* bits, EdtGeom g, int inv, float sx, T* dst) {
    const int lane = lane_id();
    const unsigned s = blockIdx.y;
    const unsigned first = (blockIdx.x * (EDT_BLOCK / 64) + wave_id()) * EDT_WORDS;
    const int tail = g.w & 63;
    for (int i = 0; i < EDT_WORDS; ++i) {
        const unsigned t = first + i;
        if (t >= g.wps) break;                                 // wave-uniform
        const unsigned row = t / (unsigned)g.rw;
        const int k = (int)(t - row * (unsigned)g.rw), x = k * 64 + lane;
        const u64* rowbits = bits + (size_t)s * g.wps + (size_t)row * (unsigned)g.rw;
        const u64 zc = ~edt_word(rowbits, k, g.rw, tail, inv);
        // the nearest zero in the words to the left / right of this one: the same for every lane
        int pl = -1, pr = -1;
        for (int j = k - 1; j >= 0; --j) {
            const u64 z = ~edt_word(rowbits, j, g.rw, tail, inv);
            if (z) { pl = j * 64 + 63 - __builtin_clzll(z); break; }
        }
        for (int j = k + 1; j < g.rw; ++j) {
            const u64 z = ~edt_word(rowbits, j, g.rw, tail, inv);
            if (z) { pr = j * 64 + __builtin_ctzll(z); break; }
        }
        const u64 zl = zc & (lane == 63 ? ~0ull : (2ull << lane) - 1ull);      // zeros at or below the lane's bit
        const u64 zr = zc & (~0ull << lane);                                   // at or above
        if (zl) pl = k * 64 + 63 - __builtin_clzll(zl);
        if (zr) pr = k * 64 + __builtin_ctzll(zr);
        int dist = -1;
        if (pl >= 0) dist = x - pl;
        if (pr >= 0 && (dist < 0 || pr - x < dist)) dist = pr - x;
        if (x < g.w) edt_store_row(dst + (size_t)s * g.V + row * (unsigned)g.w + (unsigned)x, dist, sx);
    }
}

// ---- axes y and z ----------------------------------------------------------------------------------------------------------------------------------

__device__ __forceinline__ bool edt_is_inf(int f) { return f == EDT_INF_I; }
__device__ __forceinline__ bool edt_is_inf(float f) { return f == __builtin_inff(); }
__device__ __forceinline__ int edt_inf(int) { return EDT_INF_I; }
__device__ __forceinline__ float edt_inf(float) { return __builtin_inff(); }
__device__ __forceinline__ float edt_f32(int f) { return f == EDT_INF_I ? __builtin_inff() : (float)f; }
__device__ __forceinline__ float edt_f32(float f) { return f; }

// value at u of the parabola rooted at i with height fi
__device__ __forceinline__ int edt_para(int u, int i, int fi, float) { return (u - i) * (u - i) + fi; }
__device__ __forceinline__ float edt_para(int u, int i, float fi, float sp) {
    const float dx = (float)(u - i) * sp;
    return dx * dx + fi;
}

// first u at which the parabola at j beats the one at i < j: 1 + Sep(i, j), at most m ("never inside the column").  The caller has established
// para(t, i) <= para(t, j) for the t the entry of i starts at, so the integer numerator is not negative and the result lies beyond t.
__device__ __forceinline__ int edt_first(int i, int j, int fi, int fj, int m, float, double) {
    const unsigned num = (unsigned)(j * j - i * i + fj - fi), den = (unsigned)(2 * (j - i));
    const unsigned q = num / den;
    return q >= (unsigned)m ? m : (int)q + 1;
}
__device__ __forceinline__ int edt_first(int i, int j, float fi, float fj, int m, float, double sp2) {
    const double num = (double)(j * j - i * i) * sp2 + ((double)fj - (double)fi), den = 2.0 * (double)(j - i) * sp2;
    const double q = floor(num / den);
    return q >= (double)m ? m : (q < 0.0 ? 0 : (int)q + 1);
}

// the value the call returns for a voxel whose squared distance is d2; false: the voxel is left alone (second run of the two-sided modes)
__device__ __forceinline__ bool edt_result(float d2, int mode, int inv, bool no_boundary, float& o) {
    if (mode == SEG_EDT_SQUARED) { o = d2; return true; }
    if (mode == SEG_EDT_DISTANCE) { o = sqrtf(d2); return true; }
    if (inv) {                                                 // outside the mask: + distance to the foreground
        if (no_boundary || !(d2 > 0.f)) return false;
        o = sqrtf(d2);
        return true;
    }
    o = (no_boundary || !(d2 > 0.f)) ? 0.f : (mode == SEG_EDT_SIGNED ? -sqrtf(d2) : 1.f - sqrtf(d2));
    return true;
}

struct EdtCol {
    int m;                   // length of a column
    unsigned stride;         // elements between its consecutive voxels
    unsigned ncols;          // columns per sample
    int w;                   // axis y: column c -> plane c / w, x = c % w; axis z (w = 0): the column starts at element c
    unsigned plane;          // h * w
    float sp; double sp2;    // spacing of the axis (rounded to f32) and its square
    int last, mode, inv;     // last: the result goes to `out` in the caller's mode
    long long out_stride;
};

// grid (columns of a sample / EDT_COLS, n); one lane per column
template <typename T>
__global__ __launch_bounds__(EDT_COLS) void edt_col_kernel(const T* src, T* dst, unsigned* stack, EdtGeom g, EdtCol a, const unsigned* flags, float* out) {
    const unsigned c = blockIdx.x * EDT_COLS + threadIdx.x;
    const unsigned s = blockIdx.y;
    if (c >= a.ncols) return;
    unsigned base = c;
    if (a.w) { const unsigned z = c / (unsigned)a.w; base = z * a.plane + (c - z * (unsigned)a.w); }
    const T* f = src + (size_t)s * g.V + base;
    unsigned* st = stack + (size_t)s * g.V + base;
    const int m = a.m;
    const size_t S = a.stride;
    // forward: the lower envelope.  Entry q = {i, t}: the parabola at i wins from u = t on (t strictly increasing with q); (ti, tt, tf) is the top entry
    int q = -1, ti = 0, tt = 0;
    T tf = 0;
    for (int u = 0; u < m; ++u) {
        const T fu = f[u * S];
        if (edt_is_inf(fu)) continue;
        while (q >= 0 && edt_para(tt, ti, tf, a.sp) > edt_para(tt, u, fu, a.sp)) {
            if (--q < 0) break;
            const unsigned e = st[q * S];
            ti = (int)(e >> 16); tt = (int)(e & 0xffffu);
            tf = f[ti * S];
        }
        if (q < 0) {
            q = 0; ti = u; tt = 0; tf = fu;
            st[0] = (unsigned)u << 16;
        } else {
            int t = edt_first(ti, u, tf, fu, m, a.sp, a.sp2);
            if (t <= tt) t = tt + 1;                            // (f32 path: rounding must not break the order of the stack)
            if (t < m) {
                ++q; ti = u; tt = t; tf = fu;
                st[q * S] = ((unsigned)u << 16) | (unsigned)t;
            }
        }
    }
    // backward: evaluate
    const bool no_boundary = a.last && a.mode >= SEG_EDT_SIGNED && flags[s] != (EDT_HAS_FG | EDT_HAS_BG);
    float* o = a.last ? out + (size_t)s * (size_t)a.out_stride + base : nullptr;
    T* dp = a.last ? nullptr : dst + (size_t)s * g.V + base;
    for (int u = m - 1; u >= 0; --u) {
        const T val = q < 0 ? edt_inf(tf) : edt_para(u, ti, tf, a.sp);
        if (a.last) {
            float r;
            if (edt_result(edt_f32(val), a.mode, a.inv, no_boundary, r)) o[u * S] = r;
        } else {
            dp[u * S] = val;
        }
        if (q >= 0 && u == tt && --q >= 0) {
            const unsigned e = st[q * S];
            ti = (int)(e >> 16); tt = (int)(e & 0xffffu);
            tf = f[ti * S];
        }
    }
}

template <typename T>
void edt_run(const EdtGeom& g, const EdtWs& c, int inv, float sz, float sy, float sx, int mode, float* out, long long out_stride, hipStream_t s) {
    const dim3 wgrid((g.wps + (EDT_BLOCK / 64) * EDT_WORDS - 1) / ((EDT_BLOCK / 64) * EDT_WORDS), g.n);
    hipLaunchKernelGGL(HIP_KERNEL_NAME(edt_row_kernel<T>), wgrid, dim3(EDT_BLOCK), 0, s, (const u64*)c.bits, g, inv, sx, (T*)c.a);
    EdtCol a;
    a.plane = (unsigned)g.h * (unsigned)g.w;
    a.mode = mode; a.inv = inv; a.out_stride = out_stride;
    // axis y: columns (z, x)
    a.m = g.h; a.stride = (unsigned)g.w; a.ncols = (unsigned)g.d * (unsigned)g.w; a.w = g.w;
    a.sp = sy; a.sp2 = (double)sy * (double)sy; a.last = g.d == 1;
    hipLaunchKernelGGL(HIP_KERNEL_NAME(edt_col_kernel<T>), dim3((a.ncols + EDT_COLS - 1) / EDT_COLS, g.n), dim3(EDT_COLS), 0, s, (const T*)c.a, (T*)c.b, c.stack,
                       g, a, (const unsigned*)c.flags, out);
    if (g.d == 1) return;
    // axis z: columns (y, x)
    a.m = g.d; a.stride = a.plane; a.ncols = a.plane; a.w = 0;
    a.sp = sz; a.sp2 = (double)sz * (double)sz; a.last = 1;
    hipLaunchKernelGGL(HIP_KERNEL_NAME(edt_col_kernel<T>), dim3((a.ncols + EDT_COLS - 1) / EDT_COLS, g.n), dim3(EDT_COLS), 0, s, (const T*)c.b, (T*)c.a, c.stack,
                       g, a, (const unsigned*)c.flags, out);
}

// ---- boundary loss ---------------------------------------------------------------------------------------------------------------------------------

constexpr int BL_BLOCK = 256;
constexpr int BL_GRID = 1024;                    // partial sums (four workgroups per CU)

// workgroup-wide sum in a fixed order: xor butterfly inside the wave, then the waves in index order
__device__ __forceinline__ double bl_block_sum(double v, double* sh) {
#pragma unroll
    for (int msk = 32; msk >= 1; msk >>= 1) v += __shfl_xor(v, msk);
    if (lane_id() == 0) sh[wave_id()] = v;
    __syncthreads();
    double r = sh[0];
    for (int w = 1; w < BL_BLOCK / 64; ++w) r += sh[w];
    return r;
}

// one thread per (sample, voxel), grid-stride: the probabilities, the products p * dist of the planes >= first_class in double, and the gradient
__global__ __launch_bounds__(BL_BLOCK) void bl_kernel(const float* logits, const float* dist, int c, long long v, long long total, int first_class,
                                                      float inv_m, float grad_scale, double* part, float* dlogits) {
    __shared__ double sh[BL_BLOCK / 64];
    double acc = 0.0;
    for (long long idx = (long long)blockIdx.x * BL_BLOCK + threadIdx.x; idx < total; idx += (long long)gridDim.x * BL_BLOCK) {
        const long long smp = idx / v, i = idx - smp * v;
        const size_t at = (size_t)smp * (size_t)c * (size_t)v + (size_t)i;
        if (c == 1) {
            const float x = logits[at], phi = dist[at];
            const float p = 1.f / (1.f + expf(-x));
            acc += (double)p * (double)phi;
            if (dlogits) dlogits[at] = ((p * (1.f - p) * phi) * inv_m) * grad_scale;
            continue;
        }
        float mx = logits[at];
        for (int k = 1; k < c; ++k) mx = fmaxf(mx, logits[at + (size_t)k * (size_t)v]);
        float den = 0.f;
        for (int k = 0; k < c; ++k) den += expf(logits[at + (size_t)k * (size_t)v] - mx);
        const float rden = 1.f / den;
        double sel = 0.0;
        for (int k = first_class; k < c; ++k) {
            const size_t e = at + (size_t)k * (size_t)v;
            sel += (double)(expf(logits[e] - mx) * rden) * (double)dist[e];
        }
        acc += sel;
        if (dlogits) {
            const float self = (float)sel;
            for (int k = 0; k < c; ++k) {
                const size_t e = at + (size_t)k * (size_t)v;
                const float p = expf(logits[e] - mx) * rden;
                const float br = (k >= first_class ? dist[e] : 0.f) - self;
                dlogits[e] = ((p * br) * inv_m) * grad_scale;
            }
        }
    }
    acc = bl_block_sum(acc, sh);
    if (threadIdx.x == 0) part[blockIdx.x] = acc;
}

// one wave: lane l folds its run of the partials in index order, then the fixed butterfly
__global__ __launch_bounds__(64) void bl_final_kernel(const double* part, int nblk, double m, float* out1) {
    const int lane = lane_id();
    const int per = (nblk + 63) / 64;
    double v = 0.0;
    for (int j = lane * per; j < (lane + 1) * per && j < nblk; ++j) v += part[j];
#pragma unroll
    for (int msk = 32; msk >= 1; msk >>= 1) v += __shfl_xor(v, msk);
    if (lane == 0) out1[0] = (float)(v / m);
}

}  // namespace

size_t edt_ws_bytes(int n, int d, int h, int w) {
    const EdtGeom g = edt_geom(n, d, h, w);
    return edt_align((size_t)n * 4) + edt_align((size_t)n * g.wps * 8) + 3 * edt_align((size_t)n * g.V * 4);
}

void launch_edt(const unsigned char* labels, int n, int d, int h, int w, int cls, float sz, float sy, float sx, int mode, void* ws, float* out,
                long long out_stride_n, hipStream_t s) {
    const EdtGeom g = edt_geom(n, d, h, w);
    const EdtWs c = edt_carve(ws, g);
    (void)hipMemsetAsync(c.flags, 0, (size_t)n * 4, s);
    const dim3 wgrid((g.wps + (EDT_BLOCK / 64) * EDT_WORDS - 1) / ((EDT_BLOCK / 64) * EDT_WORDS), n);
    hipLaunchKernelGGL(edt_pack_kernel, wgrid, dim3(EDT_BLOCK), 0, s, labels, g, cls, c.bits, c.flags);
    const bool unit = sz == 1.f && sy == 1.f && sx == 1.f;
    const int runs = mode >= SEG_EDT_SIGNED ? 2 : 1;
    for (int inv = 0; inv < runs; ++inv) {
        if (unit) edt_run<int>(g, c, inv, sz, sy, sx, mode, out, out_stride_n, s);
        else edt_run<float>(g, c, inv, sz, sy, sx, mode, out, out_stride_n, s);
    }
}

size_t boundary_loss_ws_bytes() { return edt_align((size_t)BL_GRID * sizeof(double)); }

void launch_boundary_loss(const float* logits, const float* dist, int n, int c, long long v, int first_class, float grad_scale, void* ws, float* out1,
                          float* dlogits, hipStream_t s) {
    const long long total = (long long)n * v;
    const double m = (double)n * (double)(c - first_class) * (double)v;
    const long long want = (total + BL_BLOCK - 1) / BL_BLOCK;
    const int nblk = (int)(want < BL_GRID ? want : BL_GRID);
    hipLaunchKernelGGL(bl_kernel, dim3(nblk), dim3(BL_BLOCK), 0, s, logits, dist, c, v, total, first_class, (float)(1.0 / m), grad_scale, (double*)ws, dlogits);
    hipLaunchKernelGGL(bl_final_kernel, dim3(1), dim3(64), 0, s, (const double*)ws, nblk, m, out1);
}

}  // namespace seg
