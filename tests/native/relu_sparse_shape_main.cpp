// Stand-alone check of the host-side grid of a convex-relu design kept sparse (adelie_amd/csrc/relu_sparse_shape.hpp), built
// with -fsanitize=address,undefined by tests/test_relu_sparse_host.py.  Over a grid of (n, d, m) it replays what the launchers
// and the kernels do with a shape -- which rows a tile owns, which gates a word, where a wavefront leaves its partial sums --
// and checks that the tiles cover [0, n) exactly once, the words the m gates exactly once, and that every partial sum lies
// inside relu_sparse_sweep_work_elems and is written once; exits non-zero on the first disagreement.  With `--table` it also
// prints one line "n m tile_rows tiles words" per (n, m).
#include "../../adelie_amd/csrc/relu_sparse_shape.hpp"
#include <algorithm>
#include <cstdio>
#include <cstring>
#include <vector>

using namespace ahip;

static int fails = 0;
#define CHECK(c) do { if (!(c)) { std::printf("FAILED line %d: %s (n=%lld d=%lld m=%lld)\n", __LINE__, #c, (long long)n, (long long)d, (long long)m); ++fails; } } while (0)

static void check_case(int64_t n, int64_t d, int64_t m, bool table) {
    const ReluSparseShape sh = relu_sparse_shape(n, m);
    const int64_t work = relu_sparse_sweep_work_elems(n, d, m);
    if (table)
        std::printf("%lld %lld %lld %lld %lld\n", (long long)n, (long long)m, (long long)sh.tile_rows, (long long)sh.tiles,
                    (long long)sh.words);
    CHECK(sh.tile_rows >= kReluSpTileUnit && sh.tile_rows % kReluSpTileUnit == 0);
    CHECK(sh.tiles >= 1 && sh.tiles <= kReluSpMaxTiles);
    CHECK(sh.tiles * sh.tile_rows >= n && (sh.tiles - 1) * sh.tile_rows < std::max<int64_t>(n, 1)); // no empty tile
    CHECK(sh.words * kReluSpWordBits >= m && (sh.words - 1) * kReluSpWordBits < std::max<int64_t>(m, 1));
    // the rows: tile t owns [t * tile_rows, min(n, (t + 1) * tile_rows))
    if (n <= (int64_t(1) << 21)) {
        std::vector<unsigned char> seen(size_t(n), 0);
        for (int64_t t = 0; t < sh.tiles; ++t)
            for (int64_t i = t * sh.tile_rows; i < std::min<int64_t>(n, (t + 1) * sh.tile_rows); ++i) ++seen[size_t(i)];
        for (int64_t i = 0; i < n; ++i) CHECK(seen[size_t(i)] == 1);
    }
    // the partial sums: tile t, gate jm = word * 32 + lane, column j of Z at t * (m d) + jm * d + j, every one written once
    if (sh.tiles * d * m <= (int64_t(1) << 20)) {
        std::vector<unsigned char> hit(size_t(work), 0);
        for (int64_t t = 0; t < sh.tiles; ++t)
            for (int64_t w = 0; w < sh.words; ++w)
                for (int64_t j = 0; j < d; ++j)
                    for (int lane = 0; lane < kReluSpWordBits; ++lane) {
                        const int64_t jm = w * kReluSpWordBits + lane;
                        if (jm >= m) continue;
                        const int64_t at = t * (m * d) + jm * d + j;
                        CHECK(at >= 0 && at < work);
                        if (at >= 0 && at < work) ++hit[size_t(at)];
                    }
        for (int64_t at = 0; at < sh.tiles * m * d; ++at) CHECK(hit[size_t(at)] == 1);
    }
    CHECK(work >= sh.tiles * m * d);
}

int main(int argc, char** argv) {
    const bool table = argc > 1 && std::strcmp(argv[1], "--table") == 0;
    const int64_t ns[] = {0, 1, 5, 257, 1031, 4095, 4096, 4097, 8192, 8229, 32805, 65536, 65537, 131072, 131073, 200000, 1000003,
                          (int64_t(1) << 31) - 1};
    const int64_t ms[] = {1, 8, 9, 19, 31, 32, 33, 37, 64, 65, 70};
    for (int64_t n : ns)
        for (int64_t m : ms) {
            check_case(n, 3, m, table);
            check_case(n, 17, m, false);
        }
    if (fails) return 1;
    std::printf("relu_sparse_shape: ok\n");
    return 0;
}
