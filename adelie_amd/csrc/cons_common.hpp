// cons_common.hpp — what the one-wavefront constraint kernels share (kernels_cons.hip: box / one-sided objects;
// kernels_cons_linear.hip: linear objects): the return codes of a visit and the unconstrained group update.  The workgroup kernel
// of kernels_cons_linear_wide.hip takes the return codes from here and restates the update on two components a lane.
#pragma once
#include "kernels.hpp"
#include "wavered.hpp"

namespace ahip {
namespace {

enum ConsRc { CRC_OK = 0, CRC_PN = 1, CRC_QP = 2, CRC_UNEXPECTED = 3, CRC_BVLS = 4 };

// bcd/unconstrained/newton.hpp:35-142 + optimization/newton.hpp:28-65 (the unconstrained group update, started at h = 0 as the
// reference's): x, and the buffers b1 = L + l2, b2 = 1 / (b1 h + l1) the dual Hessian reads.  Ctx gives `lane` and the group's
// size `d`; lane i carries component i.
template <class Ctx>
__device__ __forceinline__ void group_prox(const Ctx& c, double L, double v, double l1, double l2, double& x, double& b1, double& b2) {
    const bool in = c.lane < c.d;
    const double vn = sqrt(wave_sum64(in ? v * v : 0.0));
    if (vn <= l1) { x = 0; return; }
    if (l1 <= 0.0) { x = in ? v / (L + l2) : 0.0; return; }
    b1 = L + l2;
    double h = 0, fh, dfh;
    auto step_f = [&](double hh) {
        b2 = in ? 1.0 / (b1 * hh + l1) : 0.0;
        const double z = v * b2, zz = in ? z * z : 0.0;
        const double t = wave_sum64(zz);
        fh = t - 1.0;
        const double s = wave_sum64(zz * b1 * b2);
        dfh = -s * (1.0 + sqrt(t)) / t;
    };
    step_f(h);
    for (int it = 0; fabs(fh) > 1e-12 && it < 100000; ++it) {
        h -= fh / dfh;
        h = fmax(h, 0.0);
        step_f(h);
    }
    x = in ? h * v * b2 : 0.0;
}

} // namespace
} // namespace ahip
