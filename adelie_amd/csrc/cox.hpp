// cox.hpp — the Cox family on the device (kernels_cox.hip): the handle behind adelie_hip_glm_cox and its evaluation.
#pragma once
#include <hip/hip_runtime.h>
#include <cstdint>

#include "../../include/adelie_hip.h"

namespace ahip {

// Everything that depends only on (start, stop, status, strata, weights, tie method), uploaded once.  "Stop order" / "start
// order": rows sorted by (stratum, stop) / (stratum, start), stable; a stratum occupies the same segment in both.  A tie group
// is a run of equal stop times inside a stratum (stop order).
struct CoxPack {
    int64_t n = 0;
    // stop order (q = stop position)
    const int64_t* to = nullptr;     // row at stop position q
    const int64_t* so = nullptr;     // row at start position q
    const int64_t* gstart = nullptr; // first stop position of q's tie group
    const int64_t* bpos = nullptr;   // first start position of q's stratum with start >= stop(q), -1 if none
    const double* scale = nullptr;   // tie-breaking scale sigma (Efron k / size; 0 for Breslow)
    const double* dw = nullptr;      // status * wbar (averaged weight of the event tie), 0 for censored / zero-weight rows
    const uint8_t* flags = nullptr;  // COX_* bits below
    // row order
    const int64_t* row_a = nullptr;  // last stop position of the row's tie group
    const int64_t* row_b = nullptr;  // last stop position of the row's stratum with stop <= start(row), -1 if none
    const double* w = nullptr;       // weights
    const double* wd = nullptr;      // weights * status
    const double* ind = nullptr;     // status * (weights != 0)
};
enum : uint8_t {
    COX_STRATUM_FIRST = 1, // stop / start position q opens a stratum
    COX_TIE_FIRST = 2,     // stop position q opens a tie group (every stratum start does)
    COX_STRATUM_LAST = 4,
    COX_TIE_LAST = 8,
    COX_IND = 16           // stop position q is an event with non-zero weight
};

// doubles of caller-owned scratch one evaluation over n rows needs
size_t cox_scratch_doubles(int64_t n);
// One evaluation at eta (device pointers, row order; grad / hess may be null).  Enqueued on `st`; the loss lands in
// scratch[cox_loss_slot(n)] (a double) when want_loss.
template <class T>
void cox_eval(const CoxPack& pk, const T* eta, T* grad, T* hess, bool want_loss, double* scratch, hipStream_t st);
size_t cox_loss_slot(int64_t n);

// The losses of `lc` etas under two packs over the same n rows (cv_grpnet: the full-data family and a fold's training family),
// eta_l[i] = T(base[l * n + i] + b0[l] + off[i]), in five launches whatever `lc`: out[2 l] is the double cox_eval(pa, eta_l,
// null, null, true) leaves in its loss slot, out[2 l + 1] the same under pb, bit for bit (same tiles, same combination trees).
// Device pointers, enqueued on `st`; `scratch` holds cox_loss_batch_scratch_doubles(n, lc) doubles.
template <class T>
void cox_loss_batch(const CoxPack& pa, const CoxPack& pb, const T* base, const T* b0, const T* off, int64_t lc,
                    double* scratch, double* out, hipStream_t st);
size_t cox_loss_batch_scratch_doubles(int64_t n, int64_t lc);

} // namespace ahip

struct adelie_hip_glm_cox;
namespace ahip {
// the C entry points' bodies (throw core_error)
adelie_hip_glm_cox* cox_create(int device, int dtype, int64_t n, const void* start, const void* stop, const void* status,
                               const int64_t* strata, const void* weights, int tie_method);
void cox_destroy(adelie_hip_glm_cox* h);
void cox_eval_host(const adelie_hip_glm_cox* h, const void* eta, void* grad, void* hess, double* loss);
} // namespace ahip

struct adelie_hip_glm_cox {
    int device = 0;
    int dtype = ADELIE_HIP_F64;
    void* block = nullptr; // one device allocation holding every array of `pack`
    ahip::CoxPack pack;
};
