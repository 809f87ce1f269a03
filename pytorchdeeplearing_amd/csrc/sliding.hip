// Sliding-window inference with blended class probabilities (no counterpart in the reference, whose inference_patch ORs hard masks):
//   * gather_windows  - crop a batch of windows out of a volume, optionally mirrored per axis, padded where a window overhangs
//   * blend_windows   - acc[c] += w * p[b][c], wsum += w over the windows of one batch, w = wz[i] * wy[j] * wx[k] (importance map)
//   * blend_finalize  - threshold (C == 1) or first arg-max (C > 1) of the blended field, optionally acc / wsum as probabilities
// A window entry is four int32 {z, y, x, flipbits} in device memory; bit 0 mirrors z, bit 1 y, bit 2 x.  (i, j, k) is a position
// inside the window in VOLUME orientation (voxel - origin); the network saw, and answered, at (i', j', k') with a primed index
// = p - 1 - index on a mirrored axis.  All three kernels are streaming passes: bytes in, bytes out, a handful of flops per byte.
#include "kernels.h"

namespace seg {
namespace {

inline int sw_blocks(long long threads) {
    long long b = (threads + 255) / 256;
    return (int)(b < 1 ? 1 : (b > 16384 ? 16384 : b));
}
inline bool al16(const void* p) { return ((uintptr_t)p & 15) == 0; }

// a thread produces VEC consecutive x of one output row (one 16-byte store when VEC == 4; the launcher picks VEC so that pw % VEC == 0)
template <int VEC>
__global__ __launch_bounds__(256) void gather_windows_kernel(const float* __restrict__ vol, int D, int H, int W, const int* __restrict__ entries,
                                                             int nb, int pd, int ph, int pw, float pad_value, float* __restrict__ out) {
    const int wv = pw / VEC;
    const long long rows = (long long)nb * pd * ph, total = rows * wv;
    for (long long t = (long long)blockIdx.x * 256 + threadIdx.x; t < total; t += (long long)gridDim.x * 256) {
        const int kq = (int)(t % wv);
        const long long row = t / wv;
        const int j = (int)(row % ph), i = (int)((row / ph) % pd), b = (int)(row / ((long long)ph * pd));
        const int* e = entries + 4 * (long long)b;
        const int oz = e[0], oy = e[1], ox = e[2], fl = e[3];
        const long long z = (long long)oz + ((fl & 1) ? pd - 1 - i : i), y = (long long)oy + ((fl & 2) ? ph - 1 - j : j);
        const bool row_in = z >= 0 && z < D && y >= 0 && y < H;
        const float* src = vol + (row_in ? (z * H + y) * W : 0);
        vec<float, VEC> v;
#pragma unroll
        for (int u = 0; u < VEC; ++u) {
            const int k = kq * VEC + u;
            const long long x = (long long)ox + ((fl & 4) ? pw - 1 - k : k);
            v[u] = (row_in && x >= 0 && x < W) ? src[x] : pad_value;
        }
        *(vec<float, VEC>*)(out + row * pw + (long long)kq * VEC) = v;
    }
}

typedef int entry_t __attribute__((ext_vector_type(4), aligned(4)));      // {z, y, x, flipbits}; the list need not be 16-byte aligned
struct BlendDims {
    int nb, C, pd, ph, pw, D, H, W;
    int lo[3], hi[3];        // the launch covers voxels lo <= (z, y, x) < hi
};

// Output-stationary: a thread owns VEC consecutive x of one (z, y) row, reads acc / wsum there once, walks the nb entries in index
// order (the entry words are wave-uniform and nothing the kernel stores can alias them: one scalar load per entry, not one per
// lane; the next entry is fetched while the current one is applied), adds every window that contains a voxel and writes back.  No
// atomics, and the order of the additions into a voxel is the entry order whatever the launch shape: two runs agree bit for bit.
// VEC == 4 needs W % 4 == 0 and 16-byte aligned acc / wsum; the x range is widened to whole quads, and a voxel of a quad that no
// window contains is written back as it was read.  CB classes are kept in registers per sweep over the entry list; the class
// indices of a last, partial sweep are clamped to C - 1 (the loads stay unconditional, the duplicates are not stored).
// probs [nb][C][pd][ph][pw], entries [nb][4], acc [C][D][H][W], wsum [D][H][W].
template <int VEC, int CB>
__global__ __launch_bounds__(256) void blend_windows_kernel(const float* __restrict__ probs, const int* __restrict__ entries,
                                                            const float* __restrict__ wz, const float* __restrict__ wy,
                                                            const float* __restrict__ wx, float* __restrict__ acc, float* __restrict__ wsum,
                                                            BlendDims a) {
    typedef vec<float, VEC> fv;
    const int xq0 = a.lo[2] / VEC, nxq = (a.hi[2] + VEC - 1) / VEC - xq0;
    const int ny = a.hi[1] - a.lo[1], nz = a.hi[0] - a.lo[0];
    const long long total = (long long)nz * ny * nxq;
    const long long plane = (long long)a.D * a.H * a.W, pvol = (long long)a.pd * a.ph * a.pw;
    const bool wide = VEC == 4 && (((uintptr_t)probs | (uintptr_t)wx) & 15) == 0 && a.pw % 4 == 0;
    const entry_t* ent = (const entry_t*)entries;
    for (long long t = (long long)blockIdx.x * 256 + threadIdx.x; t < total; t += (long long)gridDim.x * 256) {
        const int x0 = (xq0 + (int)(t % nxq)) * VEC;
        const int y = a.lo[1] + (int)((t / nxq) % ny), z = a.lo[0] + (int)(t / ((long long)nxq * ny));
        const long long voff = ((long long)z * a.H + y) * a.W + x0;
        for (int c0 = 0; c0 < a.C; c0 += CB) {
            long long coff[CB];          // class offsets inside one window's probabilities / the accumulator, clamped
            fv av[CB], ws;
#pragma unroll
            for (int u = 0; u < CB; ++u) {
                const int c = c0 + u < a.C ? c0 + u : a.C - 1;
                coff[u] = c * pvol;
                av[u] = *(const fv*)(acc + c * plane + voff);
            }
#pragma unroll
            for (int v = 0; v < VEC; ++v) ws[v] = 0.f;
            if (c0 == 0) ws = *(const fv*)(wsum + voff);
            bool touched = false;
            entry_t nxt = ent[0];
            for (int b = 0; b < a.nb; ++b) {
                const entry_t e = nxt;
                if (b + 1 < a.nb) nxt = ent[b + 1];
                // modulo 2^32 on purpose: a difference outside [0, p) stays outside whatever the origin
                const unsigned i = (unsigned)z - (unsigned)e[0], j = (unsigned)y - (unsigned)e[1];
                const unsigned k3 = (unsigned)x0 - (unsigned)e[2] + (unsigned)(VEC - 1);          // k of the quad's last voxel
                if (i >= (unsigned)a.pd || j >= (unsigned)a.ph || k3 >= (unsigned)(a.pw + VEC - 1)) continue;
                touched = true;
                const int k0 = (int)k3 - (VEC - 1), fl = e[3];
                const int ip = (fl & 1) ? a.pd - 1 - (int)i : (int)i, jp = (fl & 2) ? a.ph - 1 - (int)j : (int)j;
                const float* prow = probs + (long long)b * a.C * pvol + ((long long)ip * a.ph + jp) * a.pw;
                const float wzy = wz[i] * wy[j];
                if (wide && (unsigned)k0 <= (unsigned)(a.pw - 4) && (k0 & 3) == 0) {
                    // the whole quad lies in the window on a 16-byte boundary of its rows: one wide load per class (reversed under an x mirror)
                    const int kp = (fl & 4) ? a.pw - 4 - k0 : k0;
                    vec<float, 4> w4 = *(const vec<float, 4>*)(wx + k0), p4[CB];
#pragma unroll
                    for (int u = 0; u < CB; ++u) p4[u] = *(const vec<float, 4>*)(prow + coff[u] + kp);
#pragma unroll
                    for (int v = 0; v < VEC; ++v) {
                        w4[v] *= wzy;
                        ws[v] += w4[v];
                    }
#pragma unroll
                    for (int u = 0; u < CB; ++u) {
#pragma unroll
                        for (int v = 0; v < VEC; ++v) av[u][v] += w4[v] * ((fl & 4) ? p4[u][3 - v] : p4[u][v]);
                    }
                } else {
#pragma unroll
                    for (int v = 0; v < VEC; ++v) {
                        const int k = k0 + v;
                        if ((unsigned)k >= (unsigned)a.pw) continue;
                        const float w = wzy * wx[k];
                        const int kp = (fl & 4) ? a.pw - 1 - k : k;
                        ws[v] += w;
#pragma unroll
                        for (int u = 0; u < CB; ++u) av[u][v] += w * prow[coff[u] + kp];
                    }
                }
            }
            if (!touched) break;          // containment does not depend on the class: nothing to write for the later sweeps either
#pragma unroll
            for (int u = 0; u < CB; ++u)
                if (c0 + u < a.C) *(fv*)(acc + (c0 + u) * plane + voff) = av[u];
            if (c0 == 0) *(fv*)(wsum + voff) = ws;
        }
    }
}

// mask = (acc / wsum > threshold) * scale (C == 1) or the first arg-max over acc[c] (C > 1: the common divisor does not move it);
// probs_out[c] = acc[c] / wsum when asked for; a voxel no window reached (wsum == 0) gives mask 0 and probability 0
template <int VEC>
__global__ __launch_bounds__(256) void blend_finalize_kernel(const float* __restrict__ acc, const float* __restrict__ wsum, int C, long long V,
                                                             float threshold, int scale, unsigned char* __restrict__ mask,
                                                             float* __restrict__ probs_out) {
    const long long total = V / VEC;
    for (long long t = (long long)blockIdx.x * 256 + threadIdx.x; t < total; t += (long long)gridDim.x * 256) {
        const long long o = t * VEC;
        const vec<float, VEC> ws = *(const vec<float, VEC>*)(wsum + o);
        vec<float, VEC> best = *(const vec<float, VEC>*)(acc + o);
        vec<unsigned char, VEC> m;
#pragma unroll
        for (int v = 0; v < VEC; ++v) m[v] = 0;
        if (C == 1) {
            vec<float, VEC> p;
#pragma unroll
            for (int v = 0; v < VEC; ++v) {
                p[v] = ws[v] > 0.f ? best[v] / ws[v] : 0.f;
                m[v] = (unsigned char)(p[v] > threshold ? scale : 0);
            }
            if (probs_out) *(vec<float, VEC>*)(probs_out + o) = p;
        } else {
            for (int c = 0; c < C; ++c) {
                const vec<float, VEC> x = c ? *(const vec<float, VEC>*)(acc + c * V + o) : best;
                vec<float, VEC> p;
#pragma unroll
                for (int v = 0; v < VEC; ++v) {
                    if (x[v] > best[v]) { best[v] = x[v]; m[v] = (unsigned char)c; }
                    p[v] = ws[v] > 0.f ? x[v] / ws[v] : 0.f;
                }
                if (probs_out) *(vec<float, VEC>*)(probs_out + c * V + o) = p;
            }
#pragma unroll
            for (int v = 0; v < VEC; ++v)
                if (!(ws[v] > 0.f)) m[v] = 0;
        }
        *(vec<unsigned char, VEC>*)(mask + o) = m;
    }
}

}  // namespace

void launch_gather_windows(const float* vol, int D, int H, int W, const int* entries, int nb, int pd, int ph, int pw, float pad_value, float* out,
                           hipStream_t s) {
    const long long n = (long long)nb * pd * ph * pw;
    if (pw % 4 == 0 && al16(out))
        hipLaunchKernelGGL(HIP_KERNEL_NAME(gather_windows_kernel<4>), dim3(sw_blocks(n / 4)), dim3(256), 0, s, vol, D, H, W, entries, nb, pd, ph, pw,
                           pad_value, out);
    else
        hipLaunchKernelGGL(HIP_KERNEL_NAME(gather_windows_kernel<1>), dim3(sw_blocks(n)), dim3(256), 0, s, vol, D, H, W, entries, nb, pd, ph, pw,
                           pad_value, out);
}

void launch_blend_windows(const float* probs, const int* entries, int nb, int C, int pd, int ph, int pw, const float* wz, const float* wy,
                          const float* wx, const int* box_lo, const int* box_hi, float* acc, float* wsum, int D, int H, int W, hipStream_t s) {
    BlendDims a;
    a.nb = nb; a.C = C; a.pd = pd; a.ph = ph; a.pw = pw; a.D = D; a.H = H; a.W = W;
    for (int d = 0; d < 3; ++d) { a.lo[d] = box_lo[d]; a.hi[d] = box_hi[d]; }
    const long long rows = (long long)(a.hi[0] - a.lo[0]) * (a.hi[1] - a.lo[1]);
    // classes per sweep: 1 or 2 for binary / two-class heads, 4 otherwise
    const int cb = C >= 3 ? 4 : C;
    auto go = [&](auto kernel, long long threads) {
        hipLaunchKernelGGL(kernel, dim3(sw_blocks(threads)), dim3(256), 0, s, probs, entries, wz, wy, wx, acc, wsum, a);
    };
    if (W % 4 == 0 && al16(acc) && al16(wsum)) {
        const long long n = rows * ((a.hi[2] + 3) / 4 - a.lo[2] / 4);
        if (cb == 1) go(blend_windows_kernel<4, 1>, n);
        else if (cb == 2) go(blend_windows_kernel<4, 2>, n);
        else go(blend_windows_kernel<4, 4>, n);
    } else {
        const long long n = rows * (a.hi[2] - a.lo[2]);
        if (cb == 1) go(blend_windows_kernel<1, 1>, n);
        else if (cb == 2) go(blend_windows_kernel<1, 2>, n);
        else go(blend_windows_kernel<1, 4>, n);
    }
}

void launch_blend_finalize(const float* acc, const float* wsum, int C, long long V, float threshold, int scale, unsigned char* mask, float* probs_out,
                           hipStream_t s) {
    if (V % 4 == 0 && al16(acc) && al16(wsum) && ((uintptr_t)mask & 3) == 0 && (!probs_out || al16(probs_out)))
        hipLaunchKernelGGL(HIP_KERNEL_NAME(blend_finalize_kernel<4>), dim3(sw_blocks(V / 4)), dim3(256), 0, s, acc, wsum, C, V, threshold, scale, mask,
                           probs_out);
    else
        hipLaunchKernelGGL(HIP_KERNEL_NAME(blend_finalize_kernel<1>), dim3(sw_blocks(V)), dim3(256), 0, s, acc, wsum, C, V, threshold, scale, mask,
                           probs_out);
}

}  // namespace seg
