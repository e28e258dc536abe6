// adelie_amd/csrc/multi_shape.hpp as a stand-alone host program (tests/test_multi_shape_host.py builds it under the address and
// undefined-behaviour sanitizers).  Without arguments: sweeps the sweep's plan over nb, nfeat, K, the vector width and the two
// alignment conditions and checks what the kernels rely on.  With `--plan nb nfeat K vec base_vec v_vec ...` (groups of six):
// prints the plan of each group, for the Python restatement in tests/multi_checks.py.
#include "../../adelie_amd/csrc/multi_shape.hpp"

#include <cstdio>
#include <cstdlib>
#include <cstring>

using namespace ahip;

static int fails = 0;
#define CHECK(c)                                                                                                       \
    do {                                                                                                               \
        if (!(c)) {                                                                                                    \
            if (++fails < 20)                                                                                          \
                std::printf("FAILED %s at nb=%lld nfeat=%lld K=%d vec=%d base_vec=%d v_vec=%d\n", #c, (long long)nb,   \
                            (long long)nfeat, K, vec, int(bv), int(vv));                                              \
        }                                                                                                              \
    } while (0)

int main(int argc, char** argv) {
    if (argc > 1 && !std::strcmp(argv[1], "--plan")) {
        if ((argc - 2) % 6 != 0) return 2;
        for (int q = 2; q + 6 <= argc; q += 6) {
            const MSweepPlan p = msweep_plan(std::atoll(argv[q]), std::atoll(argv[q + 1]), std::atoi(argv[q + 2]), std::atoi(argv[q + 3]),
                                             std::atoi(argv[q + 4]) != 0, std::atoi(argv[q + 5]) != 0);
            std::printf("%d %d %d %d %lld %d %lld %d\n", p.variant, p.vec, p.kt, p.feats, (long long)p.blocks_c, p.nsplit,
                        (long long)p.rows_per_split, p.kchunks);
        }
        return 0;
    }
    const int64_t feats[] = {1, 7, 8, 9, 31, 32, 33, 1000, 20000};
    const int vecs[] = {1, 2, 4};
    long long plans = 0, staged = 0, fourwave = 0, plain = 0, multi_split = 0;
    for (int vec : vecs)
        for (int64_t nfeat : feats)
            for (int K = 1; K <= 17; ++K)
                for (int64_t nb = 1; nb <= 10000; ++nb)
                    for (int al = 0; al < 4; ++al) {
                        const bool bv = al & 1, vv = al & 2;
                        const int64_t off = nb % 64;
                        if ((al == 1 || al == 2) && off > 2 && off < 62) continue; // the mixed cases around the multiples of 64 only
                        const MSweepPlan p = msweep_plan(nb, nfeat, K, vec, bv, vv);
                        ++plans;
                        const int64_t unit = int64_t(256) * vec;
                        CHECK(p.nsplit >= 1 && p.nsplit <= 65535);
                        CHECK(p.rows_per_split * p.nsplit >= nb);
                        CHECK(p.rows_per_split % unit == 0 && p.rows_per_split > 0);
                        CHECK(int64_t(p.nsplit - 1) * p.rows_per_split < nb); // no empty split
                        CHECK(p.kt == kt_of(K) && (p.kt == 2 || p.kt == 4 || p.kt == 8) && p.kt >= (K > 8 ? 8 : K));
                        CHECK(p.kchunks * p.kt >= K && (p.kchunks - 1) * p.kt < K);
                        CHECK(p.vec == (bv ? vec : 1));
                        CHECK(p.feats == (p.variant == kMSweepPlain ? 8 : 32));
                        CHECK(p.blocks_c * p.feats >= nfeat && (p.blocks_c - 1) * p.feats < nfeat);
                        CHECK(msweep_work_elems(nb, nfeat, K, vec) >= int64_t(p.nsplit) * nfeat * K);
                        CHECK((p.variant == kMSweepStaged) == (K > 4 && bv && vv));
                        CHECK((p.variant == kMSweepFourWave) == (K > 4 && !(bv && vv)));
                        CHECK((p.variant == kMSweepPlain) == (K <= 4));
                        // a bare 2-bit design: the plain kernel whatever K, and the same work size covers it
                        const MSweepPlan q = msweep_plan(nb, nfeat, K, vec, true, false, false);
                        CHECK(q.variant == kMSweepPlain && q.feats == 8 && q.vec == vec);
                        CHECK(q.rows_per_split % unit == 0 && q.rows_per_split * q.nsplit >= nb && int64_t(q.nsplit - 1) * q.rows_per_split < nb);
                        CHECK(msweep_work_elems(nb, nfeat, K, vec) >= int64_t(q.nsplit) * nfeat * K);
                        staged += p.variant == kMSweepStaged;
                        fourwave += p.variant == kMSweepFourWave;
                        plain += p.variant == kMSweepPlain;
                        multi_split += p.nsplit > 1;
                        // the steps: slices cover the rows, the fused step's leading dimension is whole workgroups
                        const int64_t sl = mstep_slices(nb, p.vec), ld = mfused_part_ld(nb, p.vec);
                        CHECK(sl * 64 * p.vec >= nb && (sl - 1) * 64 * p.vec < nb);
                        CHECK(ld >= sl && ld % kMultiFusedWaves == 0 && ld - sl < kMultiFusedWaves);
                    }
    // the shapes tests/multi_checks.py names: f64 2600 rows -> two splits of 1536 (12 and 8 tiles of 128, 40-row tail); f32 4200
    // rows -> two splits of 3072 (12 and 4 tiles of 256, 104-row tail)
    {
        const int64_t nb = 0, nfeat = 0; const int K = 0, vec = 0; const bool bv = false, vv = false;
        const MSweepPlan a = msweep_plan(2600, 41, 8, 2, true, true), b = msweep_plan(4200, 41, 8, 4, true, true);
        CHECK(a.nsplit == 2 && a.rows_per_split == 1536 && a.variant == kMSweepStaged);
        CHECK(b.nsplit == 2 && b.rows_per_split == 3072 && b.variant == kMSweepStaged);
        CHECK(msweep_plan(400, 9, 8, 2, true, true).nsplit == 1);
    }
    std::printf("plans %lld staged %lld four-wave %lld plain %lld with several splits %lld\n", plans, staged, fourwave, plain, multi_split);
    if (fails || !staged || !fourwave || !plain || !multi_split) {
        std::printf("multi_shape: %d checks failed\n", fails);
        return 1;
    }
    std::printf("multi_shape: ok\n");
    return 0;
}
