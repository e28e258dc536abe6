// Stand-alone check of the host-side grid of the structured sweep of a convex-relu design (adelie_amd/csrc/relu_shape.hpp),
// built with -fsanitize=address,undefined by tests/test_relu_host.py.  Over a grid of (n, d, m) it replays what the launcher
// and the kernel do with a shape -- which rows a slice owns, where a wave leaves its partial sums -- and checks that the
// slices cover [0, n) exactly once and that every partial sum lies inside relu_sweep_work_elems; exits non-zero on the
// first disagreement.  With `--table` it also prints one line "n d m d_tiles m_groups nslice rows_per_slice" per case.
#include "../../adelie_amd/csrc/relu_shape.hpp"
#include <algorithm>
#include <cstdio>
#include <cstring>
#include <vector>

using namespace ahip;

static int fails = 0;
#define CHECK(c) do { if (!(c)) { std::printf("FAILED line %d: %s (n=%lld d=%lld m=%lld)\n", __LINE__, #c, (long long)n, (long long)d, (long long)m); ++fails; } } while (0)

static void check_case(int64_t n, int64_t d, int64_t m, bool table) {
    const ReluShape sh = relu_shape(n, d, m);
    const int64_t work = relu_sweep_work_elems(n, d, m);
    if (table)
        std::printf("%lld %lld %lld %lld %lld %lld %lld\n", (long long)n, (long long)d, (long long)m, (long long)sh.d_tiles,
                    (long long)sh.m_groups, (long long)sh.nslice, (long long)sh.rows_per_slice);
    CHECK(sh.d_tiles * kReluTile >= d && (sh.d_tiles - 1) * kReluTile < std::max<int64_t>(d, 1));
    CHECK(sh.m_groups * kReluTile * kReluMT >= m && (sh.m_groups - 1) * kReluTile * kReluMT < std::max<int64_t>(m, 1));
    CHECK(sh.nslice >= 1 && sh.nslice <= 1024);
    CHECK(sh.rows_per_slice >= kReluStep && sh.rows_per_slice % kReluStep == 0);
    CHECK(sh.nslice == 1 || sh.rows_per_slice > 4 * kReluStep); // a slice is worth its partial sums: more than four steps
    // the rows: slice s owns [s * rps, min(n, (s + 1) * rps)), a wave walks them in steps of kReluStep, a lane in runs of kReluRun
    std::vector<unsigned char> seen(size_t(n), 0);
    for (int64_t s = 0; s < sh.nslice; ++s) {
        const int64_t r0 = s * sh.rows_per_slice, r1 = std::min<int64_t>(n, r0 + sh.rows_per_slice);
        CHECK(n == 0 || r0 < r1); // no empty slice
        for (int64_t k = r0; k < r1; k += kReluStep)
            for (int q = 0; q < 4; ++q)
                for (int e = 0; e < kReluRun; ++e) {
                    const int64_t i = k + q * kReluRun + e;
                    if (i < n) {
                        CHECK(i < r1); // (a step never reaches into the next slice: rows_per_slice is a multiple of the step)
                        ++seen[size_t(i)];
                    }
                }
    }
    for (int64_t i = 0; i < n; ++i) CHECK(seen[size_t(i)] == 1);
    // the partial sums: slice s, mask column jm, column jz of Z at s * (m d) + jm * d + jz, every one written exactly once
    if (sh.nslice * d * m <= (int64_t(1) << 20)) {
        std::vector<unsigned char> hit(size_t(work), 0);
        for (int64_t s = 0; s < sh.nslice; ++s)
            for (int64_t mg = 0; mg < sh.m_groups; ++mg)
                for (int64_t dt = 0; dt < sh.d_tiles; ++dt)
                    for (int t = 0; t < kReluMT; ++t)
                        for (int j = 0; j < kReluTile; ++j)
                            for (int i = 0; i < kReluTile; ++i) {
                                const int64_t jm = (mg * kReluMT + t) * kReluTile + j, jz = dt * kReluTile + i;
                                if (jm >= m || jz >= d) continue;
                                const int64_t at = s * (m * d) + jm * d + jz;
                                CHECK(at >= 0 && at < work);
                                if (at >= 0 && at < work) ++hit[size_t(at)];
                            }
        for (int64_t at = 0; at < sh.nslice * m * d; ++at) CHECK(hit[size_t(at)] == 1);
    }
    CHECK(work >= sh.nslice * m * d);
    CHECK(sh.d_tiles * sh.m_groups < (int64_t(1) << 31) && (sh.nslice + kReluWaves - 1) / kReluWaves <= 65535); // grid limits
}

int main(int argc, char** argv) {
    const bool table = argc > 1 && std::strcmp(argv[1], "--table") == 0;
    const int64_t ns[] = {0, 1, 2, 31, 32, 33, 255, 256, 257, 511, 512, 513, 769, 1031, 4097, 70001, 100000, 1000003};
    const int64_t dm[] = {1, 3, 16, 17, 19, 64, 65, 100};
    for (int64_t n : ns)
        for (int64_t d : dm)
            for (int64_t m : dm) check_case(n, d, m, table);
    // wide designs: one slice once the tiles alone fill the chip, and the partial sums stay d * m values per slice
    {
        const int64_t n = 100000, d = 4096, m = 4096;
        const ReluShape sh = relu_shape(n, d, m);
        CHECK(sh.nslice == 1 && relu_sweep_work_elems(n, d, m) == d * m + 16);
        check_case(n, 1, int64_t(1) << 30, false);
        check_case(n, int64_t(1) << 30, 1, false);
    }
    if (fails) return 1;
    std::printf("relu_shape: ok\n");
    return 0;
}
