// Mask post-processing on the device (dataprocess/utils.py:7-96 of the reference): connected components (labels, sizes, largest component, bounding
// boxes, size filters) and binary morphology (dilate / erode / open / close with a ball, box or cross) of n independent uint8 volumes [n][d][h][w].
//
// Both halves work on the bit-packed mask: one 64-bit word per 64 voxels of a row (rows padded to whole words, x = bit index), written by one ballot
// per word (pp_pack_kernel, shared).  A "run" below is a maximal set of consecutive set bits INSIDE one word; its first voxel is the element that
// stands for it in the union-find, so nothing is ever united along x inside a word.
//
//   components   pp_pack_kernel     ballot words; L[start] = start and cnt[start] = 0 at every run start
//                pp_union_kernel    one thread per word: runs are united with the run across the word boundary of their row and with the runs they touch
//                                   in the rows at y-1 and z-1 (faces), plus the three other rows of the backward half-neighbourhood with the x range
//                                   widened by one (fully connected).  One union per contact, found with bit operations, not per voxel.  The union
//                                   is the lock-free one of Playne & Hawick / Komura: chase both roots, atomicMin the larger root's entry to the smaller
//                                   root, go on from the returned value when the entry was no root any more.  EVERY access to L in this launch is a
//                                   relaxed agent-scope atomic (load or atomicMin): the L2s of the XCDs are not coherent for plain accesses within a
//                                   launch.  Entries only decrease and always point into their own set, so a stale value is a valid ancestor and every
//                                   chase ends; no workgroup waits for another, nothing polls.
//                pp_resolve_kernel  (a launch of its own: the kernel boundary publishes the unions)  R[start] = root = smallest linear index of the
//                                   component; component sizes are added per RUN, lanes of a wave that share a root first add up among themselves
//                                   (one atomicAdd per distinct root per wave in the common case); foreground count and box per sample likewise
//                pp_roots_kernel    root flags per word, 64-bit atomicMax per sample on size << 32 | (0xFFFFFFFF - root) (largest component, ties to
//                                   the first in raster order), number of components, exclusive scan of the root counts inside the workgroup
//                pp_scan_kernel     one workgroup: exclusive scan over the workgroups' root counts (numbering 1..K in raster order of the first voxel)
//                pp_number_kernel   L[root] = number; box of the largest component
//                pp_labels_kernel / pp_filter_kernel / pp_stats_kernel   the outputs
//   morphology   pp_morph_kernel    one thread per OUTPUT word: for every row offset (dz, dy) of the structuring element the x extent is one run
//                                   [-hw, hw] (all shapes here are convex and symmetric); the neighbouring row's left / centre / right words are
//                                   widened by hw with shift doubling (log2 steps, carries across the words) and or-ed.  Erosion is the complement of
//                                   the dilation of the complement.  Rows outside the volume and the padding bits of a row's last word are replaced
//                                   by the border value WHEN READ, so whatever a pass leaves in the padding never enters the volume.  No float, no
//                                   atomic, no loop over taps.
//
// All arithmetic is integer and every combination (min, max, add) is order-independent: two calls agree bit for bit.  Nothing is read back, no grid depends
// on the data.
#include "kernels.h"

namespace seg {

namespace {

typedef unsigned long long u64;

constexpr int PP_BLOCK = 256;
constexpr int PP_PACK_WORDS = 8;                 // words a wave of the pack / unpack / label / filter kernels walks
constexpr int PP_STATS = SEG_CC_STATS_INTS;      // int32 per sample
enum { ST_K = 0, ST_FG = 1, ST_SIZE = 2, ST_LABEL = 3, ST_INDEX = 4, ST_BOX = 5, ST_FGBOX = 11 };

struct PpGeom {
    int n, d, h, w, rw;      // rw: words per row
    unsigned V;              // voxels per sample
    unsigned nwords;         // n * d * h * rw  (< 2^31: at most one word per voxel)
};

struct CcWs {
    u64* bits;               // [nwords]
    u64* rootbits;           // [nwords]
    int* L;                  // [n * V] union-find parents at run starts; component numbers at roots after pp_number_kernel
    int* R;                  // [n * V] roots at run starts
    unsigned* cnt;           // [n * V] component sizes at roots
    unsigned* wordoff;       // [nwords] roots in front of the word inside its workgroup
    unsigned* blk;           // [nblk] roots per workgroup, then roots in front of the workgroup
    u64* best;               // [n]
    int* stats;              // [n][PP_STATS] when the caller passes none
};

// relaxed agent-scope load of a union-find entry (the host checker runs one thread at a time: a plain load)
#ifdef SEG_EMU
#define PP_ATOMIC_LOAD(p) (*(p))
#else
#define PP_ATOMIC_LOAD(p) __hip_atomic_load((p), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)
#endif

__host__ __device__ inline size_t pp_align(size_t v) { return (v + 255) / 256 * 256; }

inline PpGeom pp_geom(int n, int d, int h, int w) {
    PpGeom g;
    g.n = n; g.d = d; g.h = h; g.w = w; g.rw = (w + 63) / 64;
    g.V = (unsigned)d * (unsigned)h * (unsigned)w;
    g.nwords = (unsigned)n * (unsigned)d * (unsigned)h * (unsigned)g.rw;
    return g;
}
inline unsigned pp_nblk(const PpGeom& g) { return (g.nwords + PP_BLOCK - 1) / PP_BLOCK; }

inline CcWs pp_carve(void* ws, const PpGeom& g) {
    const size_t NV = (size_t)g.n * g.V;
    char* p = (char*)ws;
    CcWs c;
    c.bits = (u64*)p; p += pp_align((size_t)g.nwords * 8);
    c.rootbits = (u64*)p; p += pp_align((size_t)g.nwords * 8);
    c.L = (int*)p; p += pp_align(NV * 4);
    c.R = (int*)p; p += pp_align(NV * 4);
    c.cnt = (unsigned*)p; p += pp_align(NV * 4);
    c.wordoff = (unsigned*)p; p += pp_align((size_t)g.nwords * 4);
    c.blk = (unsigned*)p; p += pp_align((size_t)pp_nblk(g) * 4);
    c.best = (u64*)p; p += pp_align((size_t)g.n * 8);
    c.stats = (int*)p;
    return c;
}

__device__ __forceinline__ int imin(int a, int b) { return a < b ? a : b; }
__device__ __forceinline__ int imax(int a, int b) { return a > b ? a : b; }

// first bit of the run of `wd` that bit x belongs to
__device__ __forceinline__ int pp_run_start(u64 wd, int x) {
    const u64 z = ~wd & ((1ull << x) - 1ull);
    return z ? 64 - __builtin_clzll(z) : 0;
}

// word t -> row (over the whole batch), word in the row, sample, z, y
struct PpPos { unsigned row; int k, s, z, y; };
__device__ __forceinline__ PpPos pp_pos(unsigned t, const PpGeom& g) {
    PpPos p;
    p.row = t / (unsigned)g.rw;
    p.k = (int)(t - p.row * (unsigned)g.rw);
    const unsigned dh = (unsigned)g.d * (unsigned)g.h;
    p.s = (int)(p.row / dh);
    const unsigned r = p.row - (unsigned)p.s * dh;
    p.z = (int)(r / (unsigned)g.h);
    p.y = (int)(r - (unsigned)p.z * (unsigned)g.h);
    return p;
}

// ---- pack / unpack -----------------------------------------------------------------------------------------------------------------------------------

__global__ __launch_bounds__(PP_BLOCK) void pp_pack_kernel(const unsigned char* mask, PpGeom g, int cls, u64* bits, int* L, unsigned* cnt) {
    const int lane = lane_id();
    const unsigned first = (blockIdx.x * (PP_BLOCK / 64) + wave_id()) * PP_PACK_WORDS;
    for (int i = 0; i < PP_PACK_WORDS; ++i) {
        const unsigned t = first + i;
        if (t >= g.nwords) break;                              // wave-uniform
        const unsigned row = t / (unsigned)g.rw;
        const int x = (int)(t - row * (unsigned)g.rw) * 64 + lane;
        const unsigned idx = row * (unsigned)g.w + (unsigned)x;
        bool fg = false;
        if (x < g.w) {
            const int v = mask[idx];
            fg = cls < 0 ? v != 0 : v == cls;
        }
        const u64 b = __ballot(fg);
        if (lane == 0) bits[t] = b;
        if (L && fg && !(lane > 0 && ((b >> (lane - 1)) & 1ull))) { L[idx] = (int)idx; cnt[idx] = 0u; }
    }
}

__global__ __launch_bounds__(PP_BLOCK) void pp_unpack_kernel(const u64* bits, PpGeom g, int fg_value, unsigned char* out) {
    const int lane = lane_id();
    const unsigned first = (blockIdx.x * (PP_BLOCK / 64) + wave_id()) * PP_PACK_WORDS;
    for (int i = 0; i < PP_PACK_WORDS; ++i) {
        const unsigned t = first + i;
        if (t >= g.nwords) break;
        const unsigned row = t / (unsigned)g.rw;
        const int x = (int)(t - row * (unsigned)g.rw) * 64 + lane;
        if (x < g.w) out[row * (unsigned)g.w + (unsigned)x] = (unsigned char)(((bits[t] >> lane) & 1ull) ? fg_value : 0);
    }
}

// ---- connected components ----------------------------------------------------------------------------------------------------------------------------

__device__ __forceinline__ int pp_find(int* L, int x) {
    for (;;) {
        const int p = PP_ATOMIC_LOAD(&L[x]);
        if (p == x) return x;
        const int g = PP_ATOMIC_LOAD(&L[p]);                   // g <= p < x: entries only decrease
        if (g == p) return p;
        atomicMin(&L[x], g);                                   // path halving: g is an ancestor of x and stays one, so chains stay short under concurrency
        x = g;
    }
}

__device__ __forceinline__ void pp_unite(int* L, int a, int b) {
    for (;;) {
        a = pp_find(L, a);
        b = pp_find(L, b);
        if (a == b) return;
        if (a < b) { const int t = a; a = b; b = t; }
        const int old = atomicMin(&L[a], b);
        if (old == a) return;                                  // a was a root and now hangs under b
        a = old;                                               // somebody linked a first: its former parent and b still have to meet
    }
}

__global__ __launch_bounds__(PP_BLOCK) void pp_init_kernel(PpGeom g, u64* best, int* stats) {
    const int s = blockIdx.x * PP_BLOCK + threadIdx.x;
    if (s >= g.n) return;
    best[s] = 0ull;
    int* st = stats + (size_t)s * PP_STATS;
    for (int i = 0; i < PP_STATS; ++i) st[i] = 0;
    st[ST_INDEX] = -1;
    for (int b = ST_BOX; b <= ST_FGBOX; b += ST_FGBOX - ST_BOX) {
        st[b] = g.d; st[b + 1] = g.h; st[b + 2] = g.w;
        st[b + 3] = -1; st[b + 4] = -1; st[b + 5] = -1;
    }
}

__global__ __launch_bounds__(PP_BLOCK) void pp_union_kernel(const u64* bits, PpGeom g, int conn, int* L) {
    const unsigned t = blockIdx.x * PP_BLOCK + threadIdx.x;
    if (t >= g.nwords) return;
    const u64 A = bits[t];
    if (!A) return;
    const PpPos p = pp_pos(t, g);
    const int baseA = (int)(p.row * (unsigned)g.w) + p.k * 64;
    if (p.k > 0 && (A & 1ull)) {                               // the run that goes on from the word before
        const u64 Al = bits[t - 1];
        if (Al >> 63) pp_unite(L, baseA, baseA - 64 + pp_run_start(Al, 63));
    }
    const int ndz[4] = {0, -1, -1, -1}, ndy[4] = {-1, 0, -1, 1};
    const int nnb = conn == 1 ? 2 : 4;
    for (int j = 0; j < nnb; ++j) {
        const int zz = p.z + ndz[j], yy = p.y + ndy[j];
        if (zz < 0 || yy < 0 || yy >= g.h) continue;
        const unsigned rowB = (unsigned)((int)p.row + ndz[j] * g.h + ndy[j]);
        const unsigned tB = rowB * (unsigned)g.rw + (unsigned)p.k;
        const int baseB = (int)(rowB * (unsigned)g.w) + p.k * 64;
        const u64 Bc = bits[tB];
        const u64 O = A & Bc;
        u64 S = O & ~(O << 1);                                 // a stretch of the overlap lies in one run of either row: one union at its first bit
        while (S) {
            const int x = __builtin_ctzll(S);
            S &= S - 1ull;
            pp_unite(L, baseA + pp_run_start(A, x), baseB + pp_run_start(Bc, x));
        }
        if (conn != 1) {
            // contacts along a diagonal only: a run of A that starts at x right after a run of B ended at x - 1, or that ends at x right before one
            // starts at x + 1 (every other diagonal contact of two runs comes with a direct overlap of the same two runs)
            const u64 Bl = p.k > 0 ? bits[tB - 1] : 0ull, Br = p.k + 1 < g.rw ? bits[tB + 1] : 0ull;
            u64 Dl = A & ((Bc << 1) | (Bl >> 63)) & ~(A << 1) & ~Bc;
            while (Dl) {
                const int x = __builtin_ctzll(Dl);
                Dl &= Dl - 1ull;
                pp_unite(L, baseA + x, x > 0 ? baseB + pp_run_start(Bc, x - 1) : baseB - 64 + pp_run_start(Bl, 63));
            }
            u64 Dr = A & ((Bc >> 1) | (Br << 63)) & ~(A >> 1) & ~Bc;
            while (Dr) {
                const int x = __builtin_ctzll(Dr);
                Dr &= Dr - 1ull;
                pp_unite(L, baseA + pp_run_start(A, x), baseB + x + 1);      // B is clear at x: x + 1 starts a run (bit 0 of the next word for x = 63)
            }
        }
    }
}

// arr[key] += val for the active lanes; lanes that share the first active lane's key add up in the wave first (two rounds, then every lane for itself)
__device__ __forceinline__ void pp_wave_add(unsigned* arr, bool active, unsigned key, unsigned val) {
    const int lane = lane_id();
    for (int round = 0; round < 2; ++round) {
        const u64 act = __ballot(active);
        if (!act) return;                                      // wave-uniform
        const int leader = __builtin_ctzll(act);
        const unsigned k0 = __shfl(key, leader);
        const bool m = active && key == k0;
        unsigned v = m ? val : 0u;
#pragma unroll
        for (int msk = 32; msk >= 1; msk >>= 1) v += __shfl_xor(v, msk);
        if (lane == leader) atomicAdd(&arr[k0], v);
        active = active && !m;
    }
    if (active) atomicAdd(&arr[key], val);
}

// box[0..5] of sample s (stats + s * PP_STATS + off) takes in the lane's box; same aggregation
__device__ __forceinline__ void pp_wave_box(int* stats, int off, bool active, int s, int z, int y, int x0, int x1) {
    const int lane = lane_id();
    for (int round = 0; round < 2; ++round) {
        const u64 act = __ballot(active);
        if (!act) return;
        const int leader = __builtin_ctzll(act);
        const int s0 = __shfl(s, leader);
        const bool m = active && s == s0;
        int lz = m ? z : 0x7fffffff, ly = m ? y : 0x7fffffff, lx = m ? x0 : 0x7fffffff, hz = m ? z : -1, hy = m ? y : -1, hx = m ? x1 : -1;
#pragma unroll
        for (int msk = 32; msk >= 1; msk >>= 1) {
            lz = imin(lz, __shfl_xor(lz, msk)); ly = imin(ly, __shfl_xor(ly, msk)); lx = imin(lx, __shfl_xor(lx, msk));
            hz = imax(hz, __shfl_xor(hz, msk)); hy = imax(hy, __shfl_xor(hy, msk)); hx = imax(hx, __shfl_xor(hx, msk));
        }
        if (lane == leader) {
            int* b = stats + (size_t)s0 * PP_STATS + off;
            atomicMin(&b[0], lz); atomicMin(&b[1], ly); atomicMin(&b[2], lx);
            atomicMax(&b[3], hz); atomicMax(&b[4], hy); atomicMax(&b[5], hx);
        }
        active = active && !m;
    }
    if (active) {
        int* b = stats + (size_t)s * PP_STATS + off;
        atomicMin(&b[0], z); atomicMin(&b[1], y); atomicMin(&b[2], x0);
        atomicMax(&b[3], z); atomicMax(&b[4], y); atomicMax(&b[5], x1);
    }
}

__global__ __launch_bounds__(PP_BLOCK) void pp_resolve_kernel(const u64* bits, PpGeom g, const int* L, int* R, unsigned* cnt, int* stats) {
    const unsigned t = blockIdx.x * PP_BLOCK + threadIdx.x;
    const bool valid = t < g.nwords;
    const u64 A = valid ? bits[t] : 0ull;
    const PpPos p = pp_pos(valid ? t : 0u, g);
    const int baseA = (int)(p.row * (unsigned)g.w) + p.k * 64;
    u64 RS = A & ~(A << 1);
    while (__ballot(RS != 0ull)) {                             // the wave walks its lanes' runs together
        const bool have = RS != 0ull;
        int root = 0;
        unsigned len = 0;
        if (have) {
            const int x = __builtin_ctzll(RS);
            RS &= RS - 1ull;
            const u64 rest = ~(A >> x);
            len = rest ? (unsigned)__builtin_ctzll(rest) : 64u;
            root = baseA + x;
            for (int q = L[root]; q != root; q = L[root]) root = q;      // plain loads: nothing writes L in this launch
            R[baseA + x] = root;
        }
        pp_wave_add(cnt, have, (unsigned)root, len);
    }
    const bool fg = A != 0ull;
    pp_wave_add((unsigned*)stats, fg, (unsigned)p.s * PP_STATS + ST_FG, (unsigned)__builtin_popcountll(A));
    pp_wave_box(stats, ST_FGBOX, fg, p.s, p.z, p.y, fg ? p.k * 64 + __builtin_ctzll(A) : 0, fg ? p.k * 64 + 63 - __builtin_clzll(A) : 0);
}

__global__ __launch_bounds__(PP_BLOCK) void pp_roots_kernel(const u64* bits, PpGeom g, const int* R, const unsigned* cnt, u64* rootbits, unsigned* wordoff,
                                                            unsigned* blk, u64* best, int* stats) {
    __shared__ unsigned wsum[PP_BLOCK / 64];
    const unsigned t = blockIdx.x * PP_BLOCK + threadIdx.x;
    const int lane = lane_id(), wave = wave_id();
    const bool valid = t < g.nwords;
    const u64 A = valid ? bits[t] : 0ull;
    const PpPos p = pp_pos(valid ? t : 0u, g);
    const int baseA = (int)(p.row * (unsigned)g.w) + p.k * 64;
    u64 roots = 0ull, key = 0ull;
    for (u64 RS = A & ~(A << 1); RS; RS &= RS - 1ull) {
        const int x = __builtin_ctzll(RS), idx = baseA + x;
        if (R[idx] == idx) {
            roots |= 1ull << x;
            const u64 k = ((u64)cnt[idx] << 32) | (u64)(0xFFFFFFFFu - (unsigned)idx);
            key = k > key ? k : key;
        }
    }
    const unsigned nroots = (unsigned)__builtin_popcountll(roots);
    if (valid) rootbits[t] = roots;
    pp_wave_add((unsigned*)stats, nroots != 0u, (unsigned)p.s * PP_STATS + ST_K, nroots);
    bool active = nroots != 0u;                                // largest component: the wave's maximum per sample, then one 64-bit atomicMax
    for (int round = 0; round < 2; ++round) {
        const u64 act = __ballot(active);
        if (!act) break;
        const int leader = __builtin_ctzll(act);
        const int s0 = __shfl(p.s, leader);
        const bool m = active && p.s == s0;
        u64 v = m ? key : 0ull;
#pragma unroll
        for (int msk = 32; msk >= 1; msk >>= 1) { const u64 o = __shfl_xor(v, msk); v = o > v ? o : v; }
        if (lane == leader) atomicMax(&best[s0], v);
        active = active && !m;
    }
    if (active) atomicMax(&best[p.s], key);
    // exclusive scan of the root counts over the workgroup's 256 words
    unsigned inc = nroots;
#pragma unroll
    for (int dd = 1; dd < 64; dd <<= 1) {
        const unsigned o = __shfl(inc, lane >= dd ? lane - dd : 0);
        if (lane >= dd) inc += o;
    }
    if (lane == 63) wsum[wave] = inc;
    __syncthreads();
    unsigned before = 0;
    for (int w = 0; w < wave; ++w) before += wsum[w];
    if (valid) wordoff[t] = before + inc - nroots;
    if (threadIdx.x == PP_BLOCK - 1) blk[blockIdx.x] = before + inc;
}

// one workgroup: blk[b] = roots in front of workgroup b
__global__ __launch_bounds__(PP_BLOCK) void pp_scan_kernel(unsigned* blk, unsigned nblk) {
    __shared__ unsigned tot[PP_BLOCK];
    const unsigned t = threadIdx.x;
    const unsigned per = (nblk + PP_BLOCK - 1) / PP_BLOCK;
    const unsigned b0 = t * per < nblk ? t * per : nblk, b1 = b0 + per < nblk ? b0 + per : nblk;
    unsigned s = 0;
    for (unsigned b = b0; b < b1; ++b) s += blk[b];
    tot[t] = s;
    __syncthreads();
    unsigned off = 0;
    for (unsigned u = 0; u < t; ++u) off += tot[u];
    for (unsigned b = b0; b < b1; ++b) { const unsigned c = blk[b]; blk[b] = off; off += c; }
}

// roots in front of word t over the whole batch
__device__ __forceinline__ unsigned pp_rank_word(const unsigned* wordoff, const unsigned* blk, unsigned t) { return blk[t / PP_BLOCK] + wordoff[t]; }

// number 1..K of the root at voxel idx (linear over the batch) inside its sample
__device__ __forceinline__ int pp_number(const u64* rootbits, const unsigned* wordoff, const unsigned* blk, const PpGeom& g, unsigned idx) {
    const unsigned row = idx / (unsigned)g.w, x = idx - row * (unsigned)g.w;
    const unsigned t = row * (unsigned)g.rw + x / 64u;
    const unsigned s = idx / g.V;
    const unsigned t0 = s * (unsigned)g.d * (unsigned)g.h * (unsigned)g.rw;
    return (int)(pp_rank_word(wordoff, blk, t) + (unsigned)__builtin_popcountll(rootbits[t] & ((1ull << (x & 63u)) - 1ull)) - pp_rank_word(wordoff, blk, t0)) + 1;
}

__device__ __forceinline__ bool pp_best(const u64* best, int s, int& root, unsigned& size) {
    const u64 b = best[s];
    size = (unsigned)(b >> 32);
    root = (int)(0xFFFFFFFFu - (unsigned)b);
    return size != 0u;
}

__global__ __launch_bounds__(PP_BLOCK) void pp_number_kernel(const u64* bits, const u64* rootbits, PpGeom g, const int* R, const unsigned* wordoff,
                                                             const unsigned* blk, const u64* best, int* L, int* stats) {
    const unsigned t = blockIdx.x * PP_BLOCK + threadIdx.x;
    const bool valid = t < g.nwords;
    const u64 A = valid ? bits[t] : 0ull;
    const PpPos p = pp_pos(valid ? t : 0u, g);
    const int baseA = (int)(p.row * (unsigned)g.w) + p.k * 64;
    if (valid) {
        const unsigned t0 = (unsigned)p.s * (unsigned)g.d * (unsigned)g.h * (unsigned)g.rw;
        int num = (int)(pp_rank_word(wordoff, blk, t) - pp_rank_word(wordoff, blk, t0));
        for (u64 rb = rootbits[t]; rb; rb &= rb - 1ull) L[baseA + __builtin_ctzll(rb)] = ++num;
    }
    int broot;
    unsigned bsize;
    const bool any = pp_best(best, p.s, broot, bsize);
    int x0 = 64, x1 = -1;
    for (u64 RS = A & ~(A << 1); RS && any; RS &= RS - 1ull) {
        const int x = __builtin_ctzll(RS);
        if (R[baseA + x] != broot) continue;
        const u64 rest = ~(A >> x);
        const int len = rest ? __builtin_ctzll(rest) : 64;
        x0 = imin(x0, x); x1 = imax(x1, x + len - 1);
    }
    pp_wave_box(stats, ST_BOX, x1 >= 0, p.s, p.z, p.y, p.k * 64 + x0, p.k * 64 + x1);
}

__global__ __launch_bounds__(PP_BLOCK) void pp_stats_kernel(PpGeom g, const u64* rootbits, const unsigned* wordoff, const unsigned* blk, const u64* best,
                                                            int* stats) {
    const int s = blockIdx.x * PP_BLOCK + threadIdx.x;
    if (s >= g.n) return;
    int root;
    unsigned size;
    if (!pp_best(best, s, root, size)) return;                 // empty foreground: what pp_init_kernel wrote
    int* st = stats + (size_t)s * PP_STATS;
    st[ST_SIZE] = (int)size;
    st[ST_LABEL] = pp_number(rootbits, wordoff, blk, g, (unsigned)root);
    st[ST_INDEX] = root - (int)((unsigned)s * g.V);
}

__global__ __launch_bounds__(PP_BLOCK) void pp_labels_kernel(const u64* bits, PpGeom g, const int* L, const int* R, int* labels) {
    const int lane = lane_id();
    const unsigned first = (blockIdx.x * (PP_BLOCK / 64) + wave_id()) * PP_PACK_WORDS;
    for (int i = 0; i < PP_PACK_WORDS; ++i) {
        const unsigned t = first + i;
        if (t >= g.nwords) break;
        const unsigned row = t / (unsigned)g.rw;
        const int k = (int)(t - row * (unsigned)g.rw), x = k * 64 + lane;
        if (x >= g.w) continue;
        const u64 A = bits[t];
        const int base = (int)(row * (unsigned)g.w) + k * 64;
        labels[base + lane] = ((A >> lane) & 1ull) ? L[R[base + pp_run_start(A, lane)]] : 0;
    }
}

__global__ __launch_bounds__(PP_BLOCK) void pp_filter_kernel(const u64* bits, PpGeom g, const int* R, const unsigned* cnt, const u64* best, int mode,
                                                             unsigned min_voxels, const unsigned char* mask, unsigned char* out) {
    const int lane = lane_id();
    const unsigned first = (blockIdx.x * (PP_BLOCK / 64) + wave_id()) * PP_PACK_WORDS;
    for (int i = 0; i < PP_PACK_WORDS; ++i) {
        const unsigned t = first + i;
        if (t >= g.nwords) break;
        const unsigned row = t / (unsigned)g.rw;
        const int k = (int)(t - row * (unsigned)g.rw), x = k * 64 + lane;
        if (x >= g.w) continue;
        const u64 A = bits[t];
        const int base = (int)(row * (unsigned)g.w) + k * 64;
        bool keep = false;
        if ((A >> lane) & 1ull) {
            const int root = R[base + pp_run_start(A, lane)];
            if (mode == SEG_CC_KEEP_LARGEST) {
                int broot;
                unsigned bsize;
                keep = pp_best(best, (int)(row / ((unsigned)g.d * (unsigned)g.h)), broot, bsize) && root == broot;
            } else {
                keep = cnt[root] >= min_voxels;
            }
        }
        const unsigned char v = mask[base + lane];             // read before the store: out may be mask
        out[base + lane] = keep ? v : (unsigned char)0;
    }
}

// ---- morphology --------------------------------------------------------------------------------------------------------------------------------------

// largest |dx| the structuring element holds in the row at offset (az, ay) >= 0, or -1 when the row is no part of it.  Ball: sum (d_a / (r_a + 0.5))^2 <= 1,
// multiplied out with R_a = 2 r_a + 1 to 4 (dz^2 Ry^2 Rx^2 + dy^2 Rz^2 Rx^2 + dx^2 Rz^2 Ry^2) <= Rz^2 Ry^2 Rx^2: exact integers below 2^40, and never
// an equality (even against odd).  An axis with radius 0 has d_a = 0 only, which is what leaving it out of the sum means.
__device__ __forceinline__ int pp_half_width(int shape, int az, int ay, int rz, int ry, int rx) {
    if (shape == SEG_SE_BOX) return rx;
    if (shape == SEG_SE_CROSS) return az == 0 && ay == 0 ? rx : (az == 0 || ay == 0 ? 0 : -1);
    const long long Rz = (2 * rz + 1) * (2 * rz + 1), Ry = (2 * ry + 1) * (2 * ry + 1), Rx = (2 * rx + 1) * (2 * rx + 1);
    const long long rhs = Rz * Ry * Rx, zy = 4 * ((long long)az * az * Ry * Rx + (long long)ay * ay * Rz * Rx);
    int hw = -1;
    for (int dx = 0; dx <= rx; ++dx)
        if (zy + 4 * (long long)dx * dx * Rz * Ry <= rhs) hw = dx;
    return hw;
}

// centre word of the row (l, c, r) after a dilation by the run [-hw, hw] along x, 0 <= hw <= 31: the set of shifts 0..span doubles per step
__device__ __forceinline__ u64 pp_dilate_row(u64 l, u64 c, u64 r, int hw) {
    u64 lo = l, hi = c;                                        // towards larger x: bits leave l's top for c's bottom
    for (int span = 0; span < hw;) {
        const int s = imin(span + 1, hw - span);
        hi |= (hi << s) | (lo >> (64 - s));
        lo |= lo << s;
        span += s;
    }
    u64 lo2 = c, hi2 = r;                                      // towards smaller x
    for (int span = 0; span < hw;) {
        const int s = imin(span + 1, hw - span);
        lo2 |= (lo2 >> s) | (hi2 << (64 - s));
        hi2 |= hi2 >> s;
        span += s;
    }
    return hi | lo2;
}

__global__ __launch_bounds__(PP_BLOCK) void pp_morph_kernel(const u64* src, u64* dst, PpGeom g, int shape, int rz, int ry, int rx, int border, int inv) {
    __shared__ signed char hwtab[32 * 32];
    for (int e = threadIdx.x; e < (rz + 1) * (ry + 1); e += PP_BLOCK) hwtab[e] = (signed char)pp_half_width(shape, e / (ry + 1), e % (ry + 1), rz, ry, rx);
    __syncthreads();
    const unsigned t = blockIdx.x * PP_BLOCK + threadIdx.x;
    if (t >= g.nwords) return;
    const PpPos p = pp_pos(t, g);
    const int tail = g.w & 63;
    const u64 pad = tail ? ~0ull << tail : 0ull;               // padding bits of a row's last word
    const u64 outside = (border != 0) != (inv != 0) ? ~0ull : 0ull;      // what the pass sees outside the volume (complemented for an erosion)
    u64 acc = 0ull;
    for (int dz = -rz; dz <= rz; ++dz) {
        const int zz = p.z + dz;
        for (int dy = -ry; dy <= ry; ++dy) {
            const int hw = hwtab[(dz < 0 ? -dz : dz) * (ry + 1) + (dy < 0 ? -dy : dy)];
            if (hw < 0) continue;
            const int yy = p.y + dy;
            if (zz < 0 || zz >= g.d || yy < 0 || yy >= g.h) { acc |= outside; continue; }
            const u64* rowp = src + (size_t)((int)p.row + dz * g.h + dy) * (size_t)g.rw;
            u64 w3[3];
#pragma unroll
            for (int j = 0; j < 3; ++j) {
                const int kk = p.k + j - 1;
                if (kk < 0 || kk >= g.rw || (j != 1 && hw == 0)) { w3[j] = outside; continue; }
                u64 v = rowp[kk];
                if (kk == g.rw - 1) v = border ? v | pad : v & ~pad;
                w3[j] = inv ? ~v : v;
            }
            acc |= pp_dilate_row(w3[0], w3[1], w3[2], hw);
        }
    }
    dst[t] = inv ? ~acc : acc;
}

inline dim3 pp_word_grid(const PpGeom& g) { return dim3(pp_nblk(g)); }
inline dim3 pp_wave_grid(const PpGeom& g) {
    const unsigned per = (PP_BLOCK / 64) * PP_PACK_WORDS;
    return dim3((g.nwords + per - 1) / per);
}

// the passes every component call shares; leaves R, cnt, best, rootbits, the scan and the numbers (in L) in ws and the statistics in `stats`
void cc_run(const unsigned char* mask, const PpGeom& g, int cls, int conn, const CcWs& c, int* stats, hipStream_t s) {
    hipLaunchKernelGGL(pp_init_kernel, dim3((g.n + PP_BLOCK - 1) / PP_BLOCK), dim3(PP_BLOCK), 0, s, g, c.best, stats);
    hipLaunchKernelGGL(pp_pack_kernel, pp_wave_grid(g), dim3(PP_BLOCK), 0, s, mask, g, cls, c.bits, c.L, c.cnt);
    hipLaunchKernelGGL(pp_union_kernel, pp_word_grid(g), dim3(PP_BLOCK), 0, s, (const u64*)c.bits, g, conn, c.L);
    hipLaunchKernelGGL(pp_resolve_kernel, pp_word_grid(g), dim3(PP_BLOCK), 0, s, (const u64*)c.bits, g, (const int*)c.L, c.R, c.cnt, stats);
    hipLaunchKernelGGL(pp_roots_kernel, pp_word_grid(g), dim3(PP_BLOCK), 0, s, (const u64*)c.bits, g, (const int*)c.R, (const unsigned*)c.cnt, c.rootbits,
                       c.wordoff, c.blk, c.best, stats);
    hipLaunchKernelGGL(pp_scan_kernel, dim3(1), dim3(PP_BLOCK), 0, s, c.blk, pp_nblk(g));
    hipLaunchKernelGGL(pp_number_kernel, pp_word_grid(g), dim3(PP_BLOCK), 0, s, (const u64*)c.bits, (const u64*)c.rootbits, g, (const int*)c.R,
                       (const unsigned*)c.wordoff, (const unsigned*)c.blk, (const u64*)c.best, c.L, stats);
    hipLaunchKernelGGL(pp_stats_kernel, dim3((g.n + PP_BLOCK - 1) / PP_BLOCK), dim3(PP_BLOCK), 0, s, g, (const u64*)c.rootbits, (const unsigned*)c.wordoff,
                       (const unsigned*)c.blk, (const u64*)c.best, stats);
}

}  // namespace

size_t cc_ws_bytes(int n, int d, int h, int w) {
    const PpGeom g = pp_geom(n, d, h, w);
    const size_t NV = (size_t)g.n * g.V;
    return 2 * pp_align((size_t)g.nwords * 8) + 3 * pp_align(NV * 4) + pp_align((size_t)g.nwords * 4) + pp_align((size_t)pp_nblk(g) * 4) +
           pp_align((size_t)n * 8) + pp_align((size_t)n * PP_STATS * 4);
}

void launch_cc_label(const unsigned char* mask, int n, int d, int h, int w, int cls, int connectivity, void* ws, int* labels, int* stats, hipStream_t s) {
    const PpGeom g = pp_geom(n, d, h, w);
    const CcWs c = pp_carve(ws, g);
    cc_run(mask, g, cls, connectivity, c, stats, s);
    if (labels)
        hipLaunchKernelGGL(pp_labels_kernel, pp_wave_grid(g), dim3(PP_BLOCK), 0, s, (const u64*)c.bits, g, (const int*)c.L, (const int*)c.R, labels);
}

void launch_cc_filter(const unsigned char* mask, unsigned char* out, int n, int d, int h, int w, int cls, int connectivity, int mode, long long min_voxels,
                      void* ws, int* stats, hipStream_t s) {
    const PpGeom g = pp_geom(n, d, h, w);
    const CcWs c = pp_carve(ws, g);
    cc_run(mask, g, cls, connectivity, c, stats ? stats : c.stats, s);
    const unsigned minv = min_voxels > 0x7fffffffLL ? 0x80000000u : (unsigned)min_voxels;
    hipLaunchKernelGGL(pp_filter_kernel, pp_wave_grid(g), dim3(PP_BLOCK), 0, s, (const u64*)c.bits, g, (const int*)c.R, (const unsigned*)c.cnt,
                       (const u64*)c.best, mode, minv, mask, out);
}

size_t morph3d_ws_bytes(int n, int d, int h, int w) {
    const PpGeom g = pp_geom(n, d, h, w);
    return 2 * pp_align((size_t)g.nwords * 8);
}

void launch_morph3d(const unsigned char* mask, unsigned char* out, int n, int d, int h, int w, int cls, int op, int shape, int rz, int ry, int rx, int border,
                    int fg_value, void* ws, hipStream_t s) {
    const PpGeom g = pp_geom(n, d, h, w);
    u64* plane[2] = {(u64*)ws, (u64*)((char*)ws + pp_align((size_t)g.nwords * 8))};
    hipLaunchKernelGGL(pp_pack_kernel, pp_wave_grid(g), dim3(PP_BLOCK), 0, s, mask, g, cls, plane[0], (int*)nullptr, (unsigned*)nullptr);
    // {erode?, border} of the one or two passes; open = dilate(erode(x, 1), 0), close = erode(dilate(x, 0), 1)
    const int first_erode = op == SEG_MORPH_ERODE || op == SEG_MORPH_OPEN;
    const int two = op == SEG_MORPH_OPEN || op == SEG_MORPH_CLOSE;
    const int b0 = two ? first_erode : (border < 0 ? first_erode : border);
    hipLaunchKernelGGL(pp_morph_kernel, pp_word_grid(g), dim3(PP_BLOCK), 0, s, (const u64*)plane[0], plane[1], g, shape, rz, ry, rx, b0, first_erode);
    if (two)
        hipLaunchKernelGGL(pp_morph_kernel, pp_word_grid(g), dim3(PP_BLOCK), 0, s, (const u64*)plane[1], plane[0], g, shape, rz, ry, rx, !first_erode,
                           !first_erode);
    hipLaunchKernelGGL(pp_unpack_kernel, pp_wave_grid(g), dim3(PP_BLOCK), 0, s, (const u64*)plane[two ? 0 : 1], g, fg_value, out);
}

}  // namespace seg
