// shadow_kind_host.hpp — which encoding the shadow copy of a dense f64 design gets (design.hip, kernels_filter.hip), free of any
// device call so that it also builds into a stand-alone program (tests/native/shadow_kind_main.cpp, run under the address and
// undefined-behaviour sanitizers by tests/test_shadow_kind_host.py).
#pragma once
#include <cmath>
#include <cstdint>
#include <cstring>

namespace ahip {

// float32 column-major / int16 column-major with one f64 scale per column (s_j = max_i |x_ij| / 32767)
constexpr int kShadowF32 = 0, kShadowQ15 = 1, kShadowAuto = -1;
constexpr int64_t kShadowMinBytesDefault = int64_t(1) << 30; // `auto` looks at q15 when the float32 copy would be this large
constexpr double kShadowQ15MaxRatio = 1.0 / 2048.0;          // 2^-11: what a half-precision copy would guarantee per column

// ADELIE_HIP_SHADOW_KIND: "f32", "q15", anything else (unset, "auto") is auto
inline int shadow_kind_parse(const char* e) {
    if (!e) return kShadowAuto;
    if (!std::strcmp(e, "f32")) return kShadowF32;
    if (!std::strcmp(e, "q15")) return kShadowQ15;
    return kShadowAuto;
}

// Whether the q15 copy is built at all: forced, or `auto` on a design whose float32 copy would reach min_bytes (n p 4 >= min_bytes,
// in a form that cannot overflow).
inline bool shadow_q15_wanted(int forced, int64_t n, int64_t p, int64_t min_bytes) {
    if (forced == kShadowQ15) return true;
    if (forced == kShadowF32 || n < 1 || p < 1) return false;
    if (min_bytes <= 0) return true;
    const int64_t need = min_bytes / 4 + (min_bytes % 4 != 0); // elements
    return n >= need / p + (need % p != 0);                    // n * p >= need
}

// After the q15 copy was built and measured (err[j] = ||x_j - s_j q_j||, nrm[j] = ||s_j q_j||: the column's own norm up to err[j]):
// forced q15 keeps it; `auto` keeps it when at least 7/8 of the columns have err <= 2^-11 nrm.  A zero column (nrm = 0, err = 0)
// counts as good, a column with nrm = 0 < err (all entries denormal) or a value that is not finite as bad.
inline int shadow_kind_pick(int forced, const double* err, const double* nrm, int64_t p) {
    if (forced == kShadowQ15) return kShadowQ15;
    if (forced == kShadowF32) return kShadowF32;
    int64_t good = 0;
    for (int64_t j = 0; j < p; ++j)
        if (err[j] <= kShadowQ15MaxRatio * nrm[j]) ++good; // (false for NaN)
    return good * 8 >= p * 7 ? kShadowQ15 : kShadowF32;
}

} // namespace ahip
