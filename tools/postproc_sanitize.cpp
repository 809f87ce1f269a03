// Stand-alone host program: csrc/postproc.hip compiled through the host checker's headers (tests/emu) under AddressSanitizer and UBSan, run on the
// shapes of the tiny (5x7x9) and slab (3x130x67) test cases and a two-sample batch, with exactly-sized heap buffers so that any access outside a
// buffer or the workspace is reported.  Results are checked against a flood fill and a tap-by-tap morphology written here.  Host only: it never
// touches a GPU and is no part of the library or of the test suite.
//
//   clang++ -x c++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=undefined -I tests/emu -I pytorchdeeplearing_amd/csrc \
//       -Wno-unused-value -Wno-vla-cxx-extension tools/postproc_sanitize.cpp -o /tmp/postproc_sanitize
//   ASAN_OPTIONS=detect_stack_use_after_return=0:detect_leaks=0 /tmp/postproc_sanitize
// (the checker's fibers switch stacks by hand, and it keeps their 256 stacks for the life of the process: the only thing the leak check reports)
#include "../pytorchdeeplearing_amd/csrc/postproc.hip"

#include <cstdio>
#include <vector>

using namespace seg;

static unsigned lcg_state = 12345u;
static double lcg() { lcg_state = lcg_state * 1664525u + 1013904223u; return (lcg_state >> 8) / 16777216.0; }

static int fails = 0;
#define CHECK(c) do { if (!(c)) { printf("FAILED line %d: %s\n", __LINE__, #c); ++fails; } } while (0)

struct Vol { int n, d, h, w; std::vector<unsigned char> v; size_t V() const { return (size_t)d * h * w; } };

static Vol make(int n, int d, int h, int w, double p) {
    Vol m{n, d, h, w, std::vector<unsigned char>((size_t)n * d * h * w)};
    for (auto& x : m.v) x = lcg() < p ? 1 : 0;
    return m;
}

// flood fill in raster order: labels 1..K per sample in raster order of the first voxel
static std::vector<int> flood(const Vol& m, int conn, std::vector<int>& K) {
    std::vector<int> lab(m.v.size(), 0);
    K.assign(m.n, 0);
    for (int s = 0; s < m.n; ++s) {
        const size_t base = s * m.V();
        for (size_t i = 0; i < m.V(); ++i) {
            if (!m.v[base + i] || lab[base + i]) continue;
            const int id = ++K[s];
            std::vector<size_t> stack{i};
            lab[base + i] = id;
            while (!stack.empty()) {
                const size_t c = stack.back();
                stack.pop_back();
                const int z = (int)(c / ((size_t)m.h * m.w)), y = (int)(c / m.w % m.h), x = (int)(c % m.w);
                for (int dz = -1; dz <= 1; ++dz)
                    for (int dy = -1; dy <= 1; ++dy)
                        for (int dx = -1; dx <= 1; ++dx) {
                            const int nz = (dz != 0) + (dy != 0) + (dx != 0);
                            if (nz == 0 || (conn == 1 && nz > 1)) continue;
                            const int zz = z + dz, yy = y + dy, xx = x + dx;
                            if (zz < 0 || yy < 0 || xx < 0 || zz >= m.d || yy >= m.h || xx >= m.w) continue;
                            const size_t q = ((size_t)zz * m.h + yy) * m.w + xx;
                            if (m.v[base + q] && !lab[base + q]) { lab[base + q] = id; stack.push_back(q); }
                        }
            }
        }
    }
    return lab;
}

static bool in_se(int shape, int dz, int dy, int dx, int rz, int ry, int rx) {
    if (shape == SEG_SE_BOX) return true;
    if (shape == SEG_SE_CROSS) return (dz != 0) + (dy != 0) + (dx != 0) <= 1;
    double s = 0;
    if (rz) s += (dz / (rz + .5)) * (dz / (rz + .5));
    if (ry) s += (dy / (ry + .5)) * (dy / (ry + .5));
    if (rx) s += (dx / (rx + .5)) * (dx / (rx + .5));
    return s <= 1.0;
}

static std::vector<unsigned char> morph1(const Vol& m, const std::vector<unsigned char>& in, bool erode, int shape, int rz, int ry, int rx, int border) {
    std::vector<unsigned char> out(in.size());
    for (int s = 0; s < m.n; ++s)
        for (int z = 0; z < m.d; ++z)
            for (int y = 0; y < m.h; ++y)
                for (int x = 0; x < m.w; ++x) {
                    bool r = erode;
                    for (int dz = -rz; dz <= rz; ++dz)
                        for (int dy = -ry; dy <= ry; ++dy)
                            for (int dx = -rx; dx <= rx; ++dx) {
                                if (!in_se(shape, dz, dy, dx, rz, ry, rx)) continue;
                                const int zz = z + dz, yy = y + dy, xx = x + dx;
                                const bool v = zz < 0 || yy < 0 || xx < 0 || zz >= m.d || yy >= m.h || xx >= m.w
                                                   ? border != 0 : in[s * m.V() + ((size_t)zz * m.h + yy) * m.w + xx] != 0;
                                r = erode ? (r && v) : (r || v);
                            }
                    out[s * m.V() + ((size_t)z * m.h + y) * m.w + x] = r;
                }
    return out;
}

static void run(const Vol& m) {
    const size_t total = m.v.size();
    for (int conn = 1; conn <= 3; conn += 2) {
        std::vector<char> ws(cc_ws_bytes(m.n, m.d, m.h, m.w));
        std::vector<int> labels(total), stats((size_t)m.n * 32), K;
        launch_cc_label(m.v.data(), m.n, m.d, m.h, m.w, -1, conn, ws.data(), labels.data(), stats.data(), nullptr);
        const std::vector<int> want = flood(m, conn, K);
        CHECK(labels == want);
        for (int s = 0; s < m.n; ++s) CHECK(stats[s * 32] == K[s]);
        std::vector<unsigned char> out(total);
        launch_cc_filter(m.v.data(), out.data(), m.n, m.d, m.h, m.w, -1, conn, SEG_CC_KEEP_LARGEST, 0, ws.data(), nullptr, nullptr);
        for (size_t i = 0; i < total; ++i) CHECK(out[i] == (want[i] != 0 && want[i] == stats[i / m.V() * 32 + 3]));
        launch_cc_filter(m.v.data(), out.data(), m.n, m.d, m.h, m.w, -1, conn, SEG_CC_MIN_SIZE, 3, ws.data(), stats.data(), nullptr);
    }
    std::vector<char> ws(morph3d_ws_bytes(m.n, m.d, m.h, m.w));
    const int ses[5][4] = {{SEG_SE_BALL, 1, 1, 1}, {SEG_SE_BALL, 2, 2, 2}, {SEG_SE_BOX, 1, 1, 1}, {SEG_SE_CROSS, 1, 1, 1}, {SEG_SE_BALL, 1, 2, 31}};
    for (const auto& se : ses)
        for (int op = SEG_MORPH_DILATE; op <= SEG_MORPH_CLOSE; ++op)
            for (int border = -1; border <= (op >= SEG_MORPH_OPEN ? -1 : 1); ++border) {
                std::vector<unsigned char> out(total);
                launch_morph3d(m.v.data(), out.data(), m.n, m.d, m.h, m.w, -1, op, se[0], se[1], se[2], se[3], border, 1, ws.data(), nullptr);
                const bool first_erode = op == SEG_MORPH_ERODE || op == SEG_MORPH_OPEN;
                std::vector<unsigned char> want = morph1(m, m.v, first_erode, se[0], se[1], se[2], se[3],
                                                         op >= SEG_MORPH_OPEN || border < 0 ? first_erode : border);
                if (op >= SEG_MORPH_OPEN) want = morph1(m, want, !first_erode, se[0], se[1], se[2], se[3], !first_erode);
                CHECK(out == want);
            }
}

int main() {
    run(make(1, 5, 7, 9, .45));
    run(make(1, 3, 130, 67, .5));
    run(make(2, 6, 11, 70, .3));
    run(make(1, 1, 40, 200, .55));
    run(make(1, 2, 3, 128, .9));
    printf(fails ? "postproc_sanitize: %d check(s) FAILED\n" : "postproc_sanitize: all checks passed, no sanitizer report\n", fails);
    return fails != 0;
}
