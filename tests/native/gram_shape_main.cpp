// Stand-alone check of how the MFMA block builds cut their grids (adelie_amd/csrc/gram_shape.hpp, what the launchers of
// kernels_gram.hip / kernels_strip.hip and the kernel-level test entry call), built with -fsanitize=address,undefined by
// tests/test_block_build_cases.py.  Sweeps row counts and block shapes; exits non-zero when a split is empty, a K chunk breaks
// the kernels' alignment, a tile grid does not cover its block or a work buffer is smaller than what the launch's grid writes.
#include "../../adelie_amd/csrc/gram_shape.hpp"
#include <cstdio>
#include <vector>

using namespace ahip;

static long fails = 0;
#define CHECK(c)                                                                                                       \
    do {                                                                                                               \
        if (!(c)) {                                                                                                    \
            if (fails < 20) std::printf("FAILED line %d: %s (n=%lld M=%lld N=%lld count=%d)\n", __LINE__, #c, (long long)g_n, \
                                        (long long)g_M, (long long)g_N, g_count);                                      \
            ++fails;                                                                                                   \
        }                                                                                                              \
    } while (0)

static int64_t g_n = 0, g_M = 0, g_N = 0;
static int g_count = 0;
constexpr int64_t kMaxPartial = int64_t(1) << 28;

static void check_split(int64_t n, int nsplit, int64_t kchunk, int64_t mult) {
    CHECK(nsplit >= 1);
    CHECK(kchunk >= 1 && kchunk % mult == 0);
    CHECK(int64_t(nsplit - 1) * kchunk < n); // the last split is not empty
    CHECK(n <= int64_t(nsplit) * kchunk);    // the splits cover every row
}

// ---- what one launch's grid writes, restated from the kernels' index arithmetic ----------------------------------------------
// syrk_kernel: workgroup sp stores an SB x SB tile at part + sp * SB * SB
static int64_t syrk_grid_elems(int nsplit, int SB) { return int64_t(nsplit) * SB * SB; }
// syrk_batch_kernel: workgroup (sp, y) stores at part + (y * nsplit + sp) * SB * SB
static int64_t syrk_batch_grid_elems(int nsplit, int count, int SB) { return (int64_t(count - 1) * nsplit + nsplit) * SB * SB; }
// gram_kernel: split sp stores entry (row < Mt * 128, col < Npad) at part + sp * Mpad * Npad + col * Mpad + row
static int64_t gram_grid_elems(const GramShape& g) { return int64_t(g.nsplit) * g.Mt * kGramBM * g.Npad; }
// gram_batch_kernel: block y, split sp: a 128 x 128 tile at part + (y * nsplit + sp) * 128 * 128
static int64_t gram_batch_grid_elems(int nsplit, int count) { return int64_t(count) * nsplit * kGramBM * 128; }
// strip kernels: strip y, split sp: 16 MT rows of 256 at part + (y * nsplit + sp) * 16 MT * 256
static int64_t strip_grid_elems(int nsplit, int count, int MT) { return int64_t(count) * nsplit * 16 * MT * kStripW; }

static void check_n(int64_t n, bool all_shapes) {
    g_n = n;
    g_M = g_N = 0;
    g_count = 0;
    int ns;
    int64_t kc;
    // single diagonal block
    syrk_shape(n, ns, kc);
    check_split(n, ns, kc, 256);
    for (int64_t M = 1; M <= 128; ++M) {
        g_M = M;
        const int SB = syrk_tile_class(M);
        CHECK(SB >= M && (SB == 32 || SB == 64 || SB == 128));
        CHECK(syrk_work_elems(n, M) >= syrk_grid_elems(ns, SB));
        CHECK(syrk_work_elems(n, M) <= kMaxPartial);
    }
    g_M = 0;
    // batches of diagonal blocks / of cross blocks (the same K-splits)
    for (int count = 1; count <= 16; ++count) {
        g_count = count;
        syrk_batch_shape(n, count, ns, kc);
        check_split(n, ns, kc, 256);
        CHECK(kc % kGramKT == 0);
        CHECK(syrk_batch_work_elems(n, count) >= syrk_batch_grid_elems(ns, count, 128));
        CHECK(syrk_batch_work_elems(n, count) <= kMaxPartial);
        CHECK(gram_batch_work_elems(n, count) >= gram_batch_grid_elems(ns, count));
        CHECK(gram_batch_work_elems(n, count) <= kMaxPartial);
    }
    // strips: every spread a host thread may set, the work buffer sized without knowing it
    for (int count = 1; count <= 8; ++count) {
        g_count = count;
        for (int wgs : {1, 7, 64, kStripWgsDefault, 512, kStripWgsMax}) {
            strip_shape(n, count, wgs, ns, kc);
            check_split(n, ns, kc, 32);
            for (int m = 1; m <= 64; ++m) {
                g_M = m;
                const int MT = strip_row_tiles(m);
                CHECK(MT >= 1 && MT <= 4 && 16 * MT >= m && 16 * (MT - 1) < m);
                CHECK(strip_work_elems(n, count, m) >= strip_grid_elems(ns, count, MT));
                CHECK(strip_work_elems(n, count, m) <= kMaxPartial);
            }
            g_M = 0;
        }
    }
    CHECK(strip_row_tiles(65) == 0);
    g_count = 0;
    // general Gram
    static const int64_t edge[] = {1, 2, 63, 64, 65, 127, 128, 129, 191, 192, 193, 200, 255, 256, 257, 300, 384, 385, 400};
    auto one = [&](int64_t M, int64_t N) {
        g_M = M;
        g_N = N;
        const GramShape g = gram_shape(n, M, N);
        check_split(n, g.nsplit, g.kchunk, kGramKT);
        CHECK(g.Npad >= N && g.Npad == g.n128 * 128 + g.n64 * 64 && g.Npad - N < 128);
        CHECK(g.n64 == 0 || g.n64 == 1);
        CHECK(g.Mt * kGramBM >= M && (g.Mt - 1) * kGramBM < M);
        CHECK(gram_grid_elems(g) <= kMaxPartial);
        CHECK(gram_work_elems(n, M, N) >= gram_grid_elems(g));
    };
    if (all_shapes) {
        for (int64_t M = 1; M <= 400; ++M)
            for (int64_t N = 1; N <= 400; ++N) one(M, N);
    } else {
        for (int64_t M : edge)
            for (int64_t N : edge) one(M, N);
    }
    CHECK(gram_work_elems(n, 0, 5) == 0 && gram_work_elems(n, 5, 0) == 0);
}

int main() {
    // every shape at the row counts where the split arithmetic changes; every row count at the shapes where the tiling does
    static const int64_t full[] = {1, 2, 31, 32, 33, 255, 256, 257, 511, 512, 513, 1000, 1024, 4096, 5000, 8320, 65536, 100000,
                                   131071, 131072, 131073, 500000, 999999, 1000000};
    for (int64_t n : full) check_n(n, true);
    for (int64_t n = 1; n <= 5000; ++n) check_n(n, false);
    for (int64_t n : {10007LL, 123457LL, 262144LL, 750001LL}) check_n(n, false);
    if (fails) {
        std::printf("gram_shape: %ld checks failed\n", fails);
        return 1;
    }
    std::printf("gram_shape: ok\n");
    return 0;
}
