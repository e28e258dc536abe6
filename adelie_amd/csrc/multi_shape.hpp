// multi_shape.hpp — the host-side decisions of the multi-response kernels (kernels_multi.hip): how the K-wide sweep cuts its
// grid and which of its kernels runs, how many row slices a panel step has.  Free of device code: the launchers and a
// stand-alone host program of the tests (tests/native/multi_shape_main.cpp) include it.
#pragma once
#include <algorithm>
#include <cstdint>

namespace ahip {

constexpr int kMultiSweepThreads = 256; // threads of a sweep workgroup (four wavefronts)
constexpr int kMultiBlock = 128;        // entries of a panel block (== cd_block_size())
constexpr int kMultiFusedWaves = 16;    // waves (row slices) per workgroup of the fused step

// Features per sweep block.  The K vectors are re-read (from L2) once per block: with 4 features a K = 8 sweep pulls twice as
// many bytes of v through L2 as it streams of X from HBM and ends up bound by L2 (1.73 ms = 4.6 TB/s at 100k x 10k f64); with
// 8 the two are equal.
inline int msweep_mcb() {
    return 8; // features per block (4 was the round-1 shape: the K vectors re-read from L2 twice as often)
}
// 0: one feature group per block; 1: four waves x 8 features; 2: four waves x 4 features (half the accumulators, twice the
// waves per SIMD: 2.2 ms, the vectors' L2 traffic doubles); 3: four waves x 8 features with the vectors staged through LDS
inline int msweep_wpc() {
    return 3; // (the unstaged forms 1 / 2 measured 1.36 / 2.23 ms against 1.335 ms at K = 8)
}
inline void msweep_shape(int64_t nb, int64_t nfeat, int vec, int64_t& blocks_c, int& nsplit, int64_t& rows_per_split,
                         int wpc = 0) {
    constexpr int MT = kMultiSweepThreads;
    const int MCB = wpc == 2 ? 4 * (MT / 64) : wpc ? 8 * (MT / 64) : msweep_mcb();
    blocks_c = (nfeat + MCB - 1) / MCB;
    const int64_t unit = int64_t(MT) * vec;
    const int64_t max_split = std::max<int64_t>(1, (nb + unit * 4 - 1) / (unit * 4));
    int64_t ns = std::max<int64_t>(1, (1024 + blocks_c - 1) / blocks_c);
    ns = std::min<int64_t>(std::min<int64_t>(ns, max_split), 65535);
    rows_per_split = (nb + ns - 1) / ns;
    rows_per_split = ((rows_per_split + unit - 1) / unit) * unit;
    ns = std::max<int64_t>(1, (nb + rows_per_split - 1) / rows_per_split);
    nsplit = int(ns);
}

// responses per chunk (grid z of the sweep, grid y of the steps)
inline int kt_of(int K) { return K > 4 ? 8 : (K > 2 ? 4 : 2); }

// elements of the sweep's partial sums: covers nsplit * nfeat * K of whichever kernel the plan picks
inline int64_t msweep_work_elems(int64_t nb, int64_t nfeat, int K, int vec) {
    int64_t bc, rps;
    int ns, ns2;
    msweep_shape(nb, nfeat, vec, bc, ns, rps);
    msweep_shape(nb, nfeat, vec, bc, ns2, rps, 1);
    ns = std::max(ns, ns2);
    msweep_shape(nb, nfeat, vec, bc, ns2, rps, 2);
    return int64_t(std::max(ns, ns2)) * nfeat * K + 16;
}

enum MSweepVariant {
    kMSweepPlain = 0,    // multi_sweep_kernel, one group of 8 features per workgroup
    kMSweepFourWave = 1, // multi_sweep_kernel<WPC>, four waves x 8 features, the vectors read from global memory
    kMSweepStaged = 2    // multi_sweep_lds_kernel, four waves x 8 features, the vectors staged through LDS
};
struct MSweepPlan {
    int variant;   // MSweepVariant
    int vec;       // rows per load of the design: the type's vector width, or 1 (scalar loads)
    int kt;        // responses per chunk
    int feats;     // features per workgroup
    int64_t blocks_c;
    int nsplit;
    int64_t rows_per_split;
    int kchunks;
};
// The sweep's plan.  vec: the vector width of the value type (2 doubles, 4 floats: the row splits are cut for it whatever the
// loads); base_vec: the base takes vector loads (leading dimension a multiple of vec, 16-byte aligned columns; always for a
// 2-bit base); v_vec: nb % vec == 0 and v 16-byte aligned, i.e. each of the K vectors starts aligned; wide: the four-wave
// kernels may be used (not by the sweep over a bare 2-bit design, launch_multi_sweep_snp).
inline MSweepPlan msweep_plan(int64_t nb, int64_t nfeat, int K, int vec, bool base_vec, bool v_vec, bool wide = true) {
    MSweepPlan p{};
    p.kt = kt_of(K);
    const int wpc = (wide && p.kt == 8 && msweep_mcb() == 8) ? msweep_wpc() : 0;
    msweep_shape(nb, nfeat, vec, p.blocks_c, p.nsplit, p.rows_per_split, wpc);
    p.variant = (wpc == 3 && base_vec && v_vec) ? kMSweepStaged : wpc ? kMSweepFourWave : kMSweepPlain;
    p.vec = base_vec ? vec : 1;
    p.feats = wpc ? 8 * (kMultiSweepThreads / 64) : msweep_mcb();
    p.kchunks = (K + p.kt - 1) / p.kt;
    return p;
}

// row slices of a panel step (one wave each) and the leading dimension of the fused step's partials
inline int64_t mstep_slices(int64_t nb, int vec) { return (nb + 64 * int64_t(vec) - 1) / (64 * int64_t(vec)); }
inline int64_t mfused_part_ld(int64_t nb, int vec) {
    return ((mstep_slices(nb, vec) + kMultiFusedWaves - 1) / kMultiFusedWaves) * kMultiFusedWaves;
}

} // namespace ahip
