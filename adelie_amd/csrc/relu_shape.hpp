// relu_shape.hpp — how the structured sweep of a convex-relu design (kernels_relu.hip) cuts its grid: 16-column tiles of Z
// times groups of 16-column tiles of the mask times row slices, one wave per (tile, group, slice).  Free of device code: the
// launcher and a stand-alone host program of the tests include it.
#pragma once
#include <cstdint>

namespace ahip {

constexpr int kReluTile = 16;   // columns of Z / of the mask per matrix-core tile
constexpr int kReluMT = 4;      // mask tiles a wave keeps in accumulators against one tile of Z
constexpr int kReluRun = 8;     // consecutive rows of its column a lane loads per step
constexpr int kReluStep = 4 * kReluRun; // rows a wave consumes per step (the instruction's k = 4 lanes groups of one run each)
constexpr int kReluWaves = 4;   // waves (= row slices) per workgroup

struct ReluShape {
    int64_t d_tiles = 0, m_groups = 0; // grid x = d_tiles * m_groups
    int64_t nslice = 0;                // row slices (partial sums per column), grid y = ceil(nslice / kReluWaves)
    int64_t rows_per_slice = 0;        // a multiple of kReluStep; slice s owns rows [s * rows_per_slice, min(n, (s + 1) * ...))
};

// Row slices: about 2048 waves in all (two per SIMD of 256 compute units) so that a small d * m still covers the chip, about
// eight steps per slice or more (never as few as four), at most 1024 slices.  The partial sums are nslice * d * m values: at most 1024 d m, and once
// d * m fills the chip without slicing (more than 2048 tile groups) exactly d m.
inline ReluShape relu_shape(int64_t n, int64_t d, int64_t m) {
    ReluShape sh;
    sh.d_tiles = (d + kReluTile - 1) / kReluTile;
    sh.m_groups = (m + kReluTile * kReluMT - 1) / (kReluTile * kReluMT);
    const int64_t groups = sh.d_tiles * sh.m_groups < 1 ? 1 : sh.d_tiles * sh.m_groups;
    const int64_t unit = kReluStep;
    const int64_t max_slice = (n + unit * 8 - 1) / (unit * 8);
    int64_t ns = (2048 + groups - 1) / groups;
    if (ns > max_slice) ns = max_slice;
    if (ns > 1024) ns = 1024;
    if (ns < 1) ns = 1;
    int64_t rps = (n + ns - 1) / ns;
    rps = ((rps + unit - 1) / unit) * unit;
    if (rps < unit) rps = unit;
    ns = (n + rps - 1) / rps;
    if (ns < 1) ns = 1;
    sh.nslice = ns;
    sh.rows_per_slice = rps;
    return sh;
}

// elements of the caller's work buffer: the slices' partial sums of the m * d columns of the unsigned half
inline int64_t relu_sweep_work_elems(int64_t n, int64_t d, int64_t m) {
    return relu_shape(n, d, m).nslice * d * m + 16;
}

} // namespace ahip
