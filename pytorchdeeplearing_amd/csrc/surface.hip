// Seg_Metirc3d of the reference (model/metric.py:11-142) on the device: surface extraction (binary_erosion with the 18-neighbourhood, border_value 0),
// the four overlap counts, and the symmetric nearest-surface-point distances by an exact all-pairs search.
//
//   pass A  surf_flag_kernel     one streaming pass over both label volumes: surface flags as wave ballots (2 bits / voxel) + integer counts per workgroup
//           surf_scan_kernel     one workgroup: exclusive scan over the workgroup counts, the totals, out16[0..5]
//           surf_compact_kernel  raster-order compaction: rank = workgroup offset + words in front + popcount of the ballot below the lane
//   pass B  surf_nn_kernel       all pairs, both directions in one launch; a fixed grid walks (query tile, target slice) items it derives from the
//                                device-side counts; slices of one query tile are combined with atomicMin on the f32 bit pattern (non-negative
//                                floats order like their bits as unsigned, min is order-independent: deterministic)
//   pass C  surf_reduce_kernel   nn = sqrtf(min d^2); per-workgroup sum / sum of squares / max in double, fixed order
//           surf_final_kernel    one wave folds the partials in index order -> out16[6..15]
//
// Nothing is read back by the host and no grid depends on a count: an empty surface walks zero items.  No floating-point atomics.
#include "kernels.h"

namespace seg {

namespace {

constexpr int SF_BLOCK = 256;
constexpr int SF_CHUNK = 4096;                   // voxels per workgroup of pass A: 16 rounds of 256, 64 ballot words
constexpr int SF_WORDS = SF_CHUNK / 64;
constexpr int SF_BLK_STRIDE = 8;                 // per-workgroup record: {surf R, surf P, |R|, |P|, |R n P|, |R u P|, offset R, offset P}
constexpr int NN_Q = 4;                          // query points a thread keeps in registers
constexpr int NN_QTILE = SF_BLOCK * NN_Q;        // queries per work item
constexpr int NN_TILE = 512;                     // targets staged in LDS at a time (8 KB; every lane reads the same address: a broadcast)
constexpr int NN_GRID = 1024;                    // four workgroups per CU
constexpr int NN_WANT_ITEMS = 2048;              // work items a direction is split into when its query tiles alone would not fill the grid
constexpr int RD_GRID = 256;
constexpr unsigned F32_INF_BITS = 0x7f800000u;

// counts the later passes read on the device
enum { HDR_NR = 0, HDR_NP = 1, HDR_WORDS = 64 };

struct SurfWs {
    unsigned* hdr;              // [64]
    double* part;               // [RD_GRID][6]
    unsigned* blk;              // [nblk][8]
    unsigned long long* bits;   // [2][nwords]   surface ballots of R, of P
    unsigned* idx[2];           // [V] packed linear indices of the surface voxels, raster order
    unsigned* best[2];          // [V] min d^2 as f32 bits
};

__device__ __forceinline__ unsigned umin(unsigned a, unsigned b) { return a < b ? a : b; }
__device__ __forceinline__ unsigned umax(unsigned a, unsigned b) { return a > b ? a : b; }

__host__ __device__ inline size_t sf_align(size_t v) { return (v + 255) / 256 * 256; }

inline SurfWs carve(void* ws, long long V) {
    const size_t nblk = (size_t)((V + SF_CHUNK - 1) / SF_CHUNK), nwords = nblk * SF_WORDS;
    char* p = (char*)ws;
    SurfWs w;
    for (int s = 0; s < 2; ++s) { w.idx[s] = (unsigned*)p; p += sf_align((size_t)V * sizeof(unsigned)); }      // (documented in segengine.h: callers decode them)
    for (int s = 0; s < 2; ++s) { w.best[s] = (unsigned*)p; p += sf_align((size_t)V * sizeof(unsigned)); }
    w.hdr = (unsigned*)p; p += sf_align(HDR_WORDS * sizeof(unsigned));
    w.part = (double*)p; p += sf_align((size_t)RD_GRID * 6 * sizeof(double));
    w.blk = (unsigned*)p; p += sf_align(nblk * SF_BLK_STRIDE * sizeof(unsigned));
    w.bits = (unsigned long long*)p;
    return w;
}

__device__ __forceinline__ bool in_mask(const unsigned char* vol, int i, int cls) {
    const int v = vol[i];
    return cls < 0 ? v != 0 : v == cls;
}

// mask voxel with an 18-neighbour outside the mask or outside the volume
__device__ __forceinline__ bool is_surface(const unsigned char* vol, int i, int z, int y, int x, int D, int H, int W, int cls) {
    if (z == 0 || y == 0 || x == 0 || z == D - 1 || y == H - 1 || x == W - 1) return true;
    const int HW = H * W;
    bool all = true;
#pragma unroll
    for (int dz = -1; dz <= 1; ++dz)
#pragma unroll
        for (int dy = -1; dy <= 1; ++dy)
#pragma unroll
            for (int dx = -1; dx <= 1; ++dx)
                if ((dz != 0) + (dy != 0) + (dx != 0) <= 2 && (dz | dy | dx) != 0) all = all && in_mask(vol, i + dz * HW + dy * W + dx, cls);
    return !all;
}

__global__ __launch_bounds__(SF_BLOCK) void surf_flag_kernel(const unsigned char* real, const unsigned char* pred, int D, int H, int W, int cls,
                                                             unsigned long long* bits, long long nwords, unsigned* blk) {
    __shared__ unsigned cnt[SF_BLOCK / 64][6];
    const unsigned V = (unsigned)D * H * W, HW = (unsigned)H * W;      // V < 2^31: a voxel index inside the volume fits an int
    const int lane = lane_id(), wave = wave_id();
    unsigned c[6] = {0, 0, 0, 0, 0, 0};
    for (int r = 0; r < SF_CHUNK / SF_BLOCK; ++r) {
        const unsigned word = blockIdx.x * SF_WORDS + r * (SF_BLOCK / 64) + wave;
        const unsigned i = word * 64 + lane;
        bool mr = false, mp = false, sr = false, sp = false;
        if (i < V) {
            mr = in_mask(real, i, cls);
            mp = in_mask(pred, i, cls);
            if (mr || mp) {
                const unsigned z = i / HW, rem = i - z * HW, y = rem / W, x = rem - y * W;
                sr = mr && is_surface(real, (int)i, (int)z, (int)y, (int)x, D, H, W, cls);
                sp = mp && is_surface(pred, (int)i, (int)z, (int)y, (int)x, D, H, W, cls);
            }
        }
        const unsigned long long br = __ballot(mr), bp = __ballot(mp), bsr = __ballot(sr), bsp = __ballot(sp);
        c[0] += __builtin_popcountll(bsr); c[1] += __builtin_popcountll(bsp);
        c[2] += __builtin_popcountll(br); c[3] += __builtin_popcountll(bp);
        c[4] += __builtin_popcountll(br & bp); c[5] += __builtin_popcountll(br | bp);
        if (lane == 0) { bits[word] = bsr; bits[nwords + word] = bsp; }
    }
    if (lane == 0)
#pragma unroll
        for (int k = 0; k < 6; ++k) cnt[wave][k] = c[k];
    __syncthreads();
    if (threadIdx.x < 6) {
        unsigned s = 0;
#pragma unroll
        for (int w = 0; w < SF_BLOCK / 64; ++w) s += cnt[w][threadIdx.x];
        blk[blockIdx.x * SF_BLK_STRIDE + threadIdx.x] = s;
    }
}

// one workgroup: thread t owns a contiguous run of workgroup records; exclusive scan of the two surface counts, totals of all six
__global__ __launch_bounds__(SF_BLOCK) void surf_scan_kernel(unsigned* blk, int nblk, unsigned* hdr, double* out16) {
    __shared__ unsigned long long tot[SF_BLOCK][6];
    const int t = threadIdx.x;
    const int per = (nblk + SF_BLOCK - 1) / SF_BLOCK, b0 = (int)umin(nblk, t * per), b1 = (int)umin(nblk, b0 + per);
    unsigned long long s[6] = {0, 0, 0, 0, 0, 0};
    for (int b = b0; b < b1; ++b)
#pragma unroll
        for (int k = 0; k < 6; ++k) s[k] += blk[b * SF_BLK_STRIDE + k];
#pragma unroll
    for (int k = 0; k < 6; ++k) tot[t][k] = s[k];
    __syncthreads();
    unsigned long long off[2] = {0, 0};
    for (int u = 0; u < t; ++u) { off[0] += tot[u][0]; off[1] += tot[u][1]; }
    for (int b = b0; b < b1; ++b) {
        blk[b * SF_BLK_STRIDE + 6] = (unsigned)off[0];
        blk[b * SF_BLK_STRIDE + 7] = (unsigned)off[1];
        off[0] += blk[b * SF_BLK_STRIDE + 0];
        off[1] += blk[b * SF_BLK_STRIDE + 1];
    }
    if (t < 6) {
        unsigned long long a = 0;
        for (int u = 0; u < SF_BLOCK; ++u) a += tot[u][t];
        // out16: {|R|, |P|, |R n P|, |R u P|, n_surf_R, n_surf_P, ...}
        out16[t < 2 ? 4 + t : t - 2] = (double)a;
        if (t < 2) hdr[HDR_NR + t] = (unsigned)a;
    }
}

__global__ __launch_bounds__(SF_BLOCK) void surf_compact_kernel(const unsigned long long* bits, long long nwords, const unsigned* blk, unsigned* idxR,
                                                                unsigned* idxP, unsigned* bestR, unsigned* bestP) {
    __shared__ unsigned base[2][SF_WORDS];
    const int lane = lane_id(), wave = wave_id();
    if (wave < 2) {           // wave s: exclusive scan over the 64 ballot words of side s (one word per lane)
        const unsigned n = __builtin_popcountll(bits[wave * nwords + (long long)blockIdx.x * SF_WORDS + lane]);
        unsigned inc = n;
#pragma unroll
        for (int d = 1; d < 64; d <<= 1) {
            const unsigned o = __shfl(inc, lane >= d ? lane - d : 0);
            if (lane >= d) inc += o;
        }
        base[wave][lane] = blk[blockIdx.x * SF_BLK_STRIDE + 6 + wave] + inc - n;
    }
    __syncthreads();
    const unsigned long long below = (1ull << lane) - 1ull;
    for (int w = wave; w < SF_WORDS; w += SF_BLOCK / 64) {
        const long long word = (long long)blockIdx.x * SF_WORDS + w;
        const unsigned v = (unsigned)(word * 64 + lane);
        const unsigned long long mr = bits[word], mp = bits[nwords + word];
        if ((mr >> lane) & 1ull) {
            const unsigned r = base[0][w] + __builtin_popcountll(mr & below);
            idxR[r] = v; bestR[r] = F32_INF_BITS;
        }
        if ((mp >> lane) & 1ull) {
            const unsigned r = base[1][w] + __builtin_popcountll(mp & below);
            idxP[r] = v; bestP[r] = F32_INF_BITS;
        }
    }
}

__device__ __forceinline__ void decode(unsigned v, unsigned HW, unsigned W, float& z, float& y, float& x) {
    const unsigned zi = v / HW, rem = v - zi * HW, yi = rem / W;
    z = (float)zi; y = (float)yi; x = (float)(rem - yi * W);
}

// how one direction (nq query points against nt target points) is cut into work items
struct NnPlan { unsigned slices, tiles_per_slice, items; };
__device__ __forceinline__ NnPlan nn_plan(unsigned nq, unsigned nt) {
    NnPlan p = {0, 0, 0};
    if (nq == 0 || nt == 0) return p;
    const unsigned nqt = (nq + NN_QTILE - 1) / NN_QTILE, ntiles = (nt + NN_TILE - 1) / NN_TILE;
    const unsigned want = umin(ntiles, umax(1u, (NN_WANT_ITEMS + nqt - 1) / nqt));
    p.tiles_per_slice = (ntiles + want - 1) / want;
    p.slices = (ntiles + p.tiles_per_slice - 1) / p.tiles_per_slice;
    p.items = nqt * p.slices;
    return p;
}

// Coordinates are exact integers in f32 (extents <= 2048), so the differences are exact; with unit spacing every d^2 is an integer below 2^24 and
// the minimum is exact.
__global__ __launch_bounds__(SF_BLOCK) void surf_nn_kernel(const unsigned* hdr, const unsigned* idxR, const unsigned* idxP, unsigned* bestR, unsigned* bestP,
                                                           int H, int W, float sz, float sy, float sx) {
    __shared__ f32x4 tile[NN_TILE];
    const unsigned nR = hdr[HDR_NR], nP = hdr[HDR_NP];
    const unsigned HW = (unsigned)H * (unsigned)W;
    const NnPlan p0 = nn_plan(nR, nP), p1 = nn_plan(nP, nR);
    const unsigned total = p0.items + p1.items;
    for (unsigned item = blockIdx.x; item < total; item += gridDim.x) {
        const bool rev = item >= p0.items;                      // false: real -> pred, true: pred -> real
        const NnPlan p = rev ? p1 : p0;
        const unsigned local = rev ? item - p0.items : item;
        const unsigned qt = local / p.slices, sl = local - qt * p.slices;
        const unsigned nq = rev ? nP : nR, nt = rev ? nR : nP;
        const unsigned* qidx = rev ? idxP : idxR;
        const unsigned* tidx = rev ? idxR : idxP;
        unsigned* best = rev ? bestP : bestR;
        float qz[NN_Q], qy[NN_Q], qx[NN_Q], m[NN_Q];
#pragma unroll
        for (int q = 0; q < NN_Q; ++q) {
            const unsigned qi = qt * NN_QTILE + q * SF_BLOCK + threadIdx.x;
            decode(qi < nq ? qidx[qi] : 0u, HW, (unsigned)W, qz[q], qy[q], qx[q]);
            m[q] = __builtin_bit_cast(float, F32_INF_BITS);
        }
        const unsigned t0 = sl * p.tiles_per_slice * NN_TILE, t1 = umin(nt, t0 + p.tiles_per_slice * NN_TILE);
        for (unsigned tb = t0; tb < t1; tb += NN_TILE) {
            const int cnt = (int)umin((unsigned)NN_TILE, t1 - tb);
            __syncthreads();                                    // the previous tile has been consumed
            for (int j = threadIdx.x; j < cnt; j += SF_BLOCK) {
                float tz, ty, tx;
                decode(tidx[tb + j], HW, (unsigned)W, tz, ty, tx);
                const f32x4 t = {tz, ty, tx, 0.f};
                tile[j] = t;
            }
            __syncthreads();
#pragma unroll 8
            for (int j = 0; j < cnt; ++j) {
                const f32x4 t = tile[j];
#pragma unroll
                for (int q = 0; q < NN_Q; ++q) {
                    const float dz = (qz[q] - t[0]) * sz, dy = (qy[q] - t[1]) * sy, dx = (qx[q] - t[2]) * sx;
                    m[q] = fminf(m[q], dz * dz + dy * dy + dx * dx);
                }
            }
        }
#pragma unroll
        for (int q = 0; q < NN_Q; ++q) {
            const unsigned qi = qt * NN_QTILE + q * SF_BLOCK + threadIdx.x;
            if (qi < nq) atomicMin(&best[qi], __builtin_bit_cast(unsigned, m[q]));
        }
    }
}

// workgroup-wide fold in a fixed order: xor butterfly inside the wave, then the waves in index order
__device__ __forceinline__ double block_fold(double v, bool is_max, double* sh) {
#pragma unroll
    for (int msk = 32; msk >= 1; msk >>= 1) {
        const double o = __shfl_xor(v, msk);
        v = is_max ? fmax(v, o) : v + o;
    }
    __syncthreads();
    if (lane_id() == 0) sh[wave_id()] = v;
    __syncthreads();
    double r = sh[0];
    for (int w = 1; w < SF_BLOCK / 64; ++w) r = is_max ? fmax(r, sh[w]) : r + sh[w];
    return r;
}

__global__ __launch_bounds__(SF_BLOCK) void surf_reduce_kernel(const unsigned* hdr, const unsigned* bestR, const unsigned* bestP, float* nnR, float* nnP,
                                                               double* part) {
    __shared__ double sh[SF_BLOCK / 64];
    for (int side = 0; side < 2; ++side) {
        const unsigned n = hdr[HDR_NR + side];
        const unsigned* best = side ? bestP : bestR;
        float* nn = side ? nnP : nnR;
        double s = 0.0, s2 = 0.0, mx = 0.0;
        for (unsigned i = blockIdx.x * SF_BLOCK + threadIdx.x; i < n; i += gridDim.x * SF_BLOCK) {
            const float d = sqrtf(__builtin_bit_cast(float, best[i]));
            if (nn) nn[i] = d;
            s += (double)d; s2 += (double)d * (double)d; mx = fmax(mx, (double)d);
        }
        s = block_fold(s, false, sh); s2 = block_fold(s2, false, sh); mx = block_fold(mx, true, sh);
        if (threadIdx.x == 0) {
            part[blockIdx.x * 6 + side] = s;
            part[blockIdx.x * 6 + 2 + side] = s2;
            part[blockIdx.x * 6 + 4 + side] = mx;
        }
    }
}

// one wave: lane l folds partials 4l .. 4l+3 in index order, then the fixed butterfly; out16[6..11] = {sum r2p, sum p2r, sum r2p^2, sum p2r^2, max r2p, max p2r}
__global__ __launch_bounds__(64) void surf_final_kernel(const unsigned* hdr, const double* part, double* out16) {
    const int lane = lane_id();
    const bool empty = hdr[HDR_NR] == 0 || hdr[HDR_NP] == 0;
    for (int k = 0; k < 6; ++k) {
        const bool is_max = k >= 4;
        double v = part[(lane * (RD_GRID / 64)) * 6 + k];
        for (int j = 1; j < RD_GRID / 64; ++j) {
            const double o = part[(lane * (RD_GRID / 64) + j) * 6 + k];
            v = is_max ? fmax(v, o) : v + o;
        }
#pragma unroll
        for (int msk = 32; msk >= 1; msk >>= 1) {
            const double o = __shfl_xor(v, msk);
            v = is_max ? fmax(v, o) : v + o;
        }
        if (lane == 0) out16[6 + k] = empty ? __builtin_nan("") : v;
    }
    if (lane < 4) out16[12 + lane] = 0.0;
}

}  // namespace

size_t surface_ws_bytes(int D, int H, int W) {
    const long long V = (long long)D * H * W;
    const size_t nblk = (size_t)((V + SF_CHUNK - 1) / SF_CHUNK);
    return sf_align(HDR_WORDS * sizeof(unsigned)) + sf_align((size_t)RD_GRID * 6 * sizeof(double)) + sf_align(nblk * SF_BLK_STRIDE * sizeof(unsigned)) +
           sf_align(2 * nblk * SF_WORDS * sizeof(unsigned long long)) + 4 * sf_align((size_t)V * sizeof(unsigned));
}

void launch_surface_metrics(const unsigned char* real, const unsigned char* pred, int D, int H, int W, int cls, double sz, double sy, double sx, void* ws,
                            double* out16, float* real2pred_nn, float* pred2real_nn, hipStream_t s) {
    const long long V = (long long)D * H * W;
    const int nblk = (int)((V + SF_CHUNK - 1) / SF_CHUNK);
    const long long nwords = (long long)nblk * SF_WORDS;
    const SurfWs w = carve(ws, V);
    hipLaunchKernelGGL(surf_flag_kernel, dim3(nblk), dim3(SF_BLOCK), 0, s, real, pred, D, H, W, cls, w.bits, nwords, w.blk);
    hipLaunchKernelGGL(surf_scan_kernel, dim3(1), dim3(SF_BLOCK), 0, s, w.blk, nblk, w.hdr, out16);
    hipLaunchKernelGGL(surf_compact_kernel, dim3(nblk), dim3(SF_BLOCK), 0, s, (const unsigned long long*)w.bits, nwords, (const unsigned*)w.blk, w.idx[0],
                       w.idx[1], w.best[0], w.best[1]);
    hipLaunchKernelGGL(surf_nn_kernel, dim3(NN_GRID), dim3(SF_BLOCK), 0, s, (const unsigned*)w.hdr, (const unsigned*)w.idx[0], (const unsigned*)w.idx[1],
                       w.best[0], w.best[1], H, W, (float)sz, (float)sy, (float)sx);
    hipLaunchKernelGGL(surf_reduce_kernel, dim3(RD_GRID), dim3(SF_BLOCK), 0, s, (const unsigned*)w.hdr, (const unsigned*)w.best[0], (const unsigned*)w.best[1],
                       real2pred_nn, pred2real_nn, w.part);
    hipLaunchKernelGGL(surf_final_kernel, dim3(1), dim3(64), 0, s, (const unsigned*)w.hdr, (const double*)w.part, out16);
}

}  // namespace seg
