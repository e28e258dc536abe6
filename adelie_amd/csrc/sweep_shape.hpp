// sweep_shape.hpp — how a sweep over a dense design cuts its grid: panels of columns times row splits.  Free of device code:
// the kernels' launchers (kernels_sweep.hip, kernels_filter.hip) and a stand-alone host program of the tests include it.
#pragma once
#include <cstdint>

namespace ahip {

constexpr int kSweepThreads = 256; // threads of a sweep workgroup
// columns per panel of sweep_kernel (8 halves the re-reads of v through L2 and measured 6.66 against 6.85 TB/s)
constexpr int kSweepCB = 4;
// the float32 shadow sweep (shadow_sweep_kernel<ShadowF32>, kernels_filter.hip): columns per panel, floats per load.  8 columns of 16-byte float loads read
// 16 B of v per 64 B of design, as sweep_kernel does with 4 columns of doubles (measured: profiles/filter_sweep_fused.txt)
constexpr int kShadowCB = 8, kShadowVec = 4;
// the 16-bit shadow sweep (shadow_sweep_kernel<ShadowQ15>): 16-byte loads of 8 rows.  At 8 columns a lane reads 64 B of v per 128 B of
// design, at 16 columns 64 B per 256 B (the float32 kind's ratio).  Both widths were measured: 8 columns 421 us per launch on the
// headline, 16 columns 477 us plus a reduce launch (one wave less per SIMD, two row splits: profiles/filter_sweep_q15.txt)
// (with the plain body loop; the rotation of two half panels the kernel runs now needs CB even: 374 us, profiles/shadow_q15_rate.txt)
constexpr int kShadowCB16 = 8, kShadowVec16 = 8;
static_assert(kShadowCB16 % 2 == 0, "the q15 body loop rotates two half panels");
// leading dimension of the 16-bit copy: a multiple of this many elements (128 B), pad rows hold 0
constexpr int kShadowPad16 = 64;

// vec: rows per thread and iteration; cb: columns per panel of the kernel the shape is for
inline void sweep_shape(int64_t n, int64_t ncols, int vec, int64_t& blocks_c, int& nsplit, int64_t& rows_per_split,
                        int cb = kSweepCB) {
    blocks_c = (ncols + cb - 1) / cb;
    const int64_t unit = int64_t(kSweepThreads) * vec;         // rows per block iteration
    const int64_t max_split = (n + unit * 4 - 1) / (unit * 4); // >= 4 iterations per split
    int64_t want = (1024 + blocks_c - 1) / blocks_c;
    int64_t ns = want < 1 ? 1 : want;
    if (ns > max_split) ns = max_split;
    if (ns < 1) ns = 1;
    if (ns > 65535) ns = 65535;
    rows_per_split = (n + ns - 1) / ns;
    rows_per_split = ((rows_per_split + unit - 1) / unit) * unit;
    ns = (n + rows_per_split - 1) / rows_per_split;
    if (ns < 1) ns = 1;
    nsplit = int(ns);
}

} // namespace ahip
