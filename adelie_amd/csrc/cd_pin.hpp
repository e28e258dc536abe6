// cd_pin.hpp — what the one-launch pin path (kernels_cd_pin.hip) and its host driver (solver_pin.hpp) exchange.
//
// A pin solve (solver_gaussian_pin_naive.hpp:217-401, solver_gaussian_pin_cov.hpp:530-705) runs the coordinate descent of
// kernels_cd.hip / kernels_cd_lasso.hip at every lambda of a given path on a screen set that never changes.  Nothing has to
// be looked at between two lambdas, so one workgroup runs the whole path: the per-lambda body is the text the single-lambda
// kernels instantiate (cd_path_body.hpp), the loop over the path and the exit rules are around it on the device.
#pragma once
#include "kernels.hpp"

namespace ahip {

// row l of the snapshot block: the state after lambda l (counters cumulative over the path)
template <class T>
struct CdPinRow {
    T rsq, resid_sum;
    int64_t iters, n_visits_screen, n_visits_active, n_updates, n_passes_screen, n_passes_active;
    int64_t clock; // wall_clock64() when the row was written (the one-launch route; 0 otherwise)
    int32_t active_size, _pad;
};

struct CdPinOut {
    int32_t n_solved; // rows written (the row at which an exit rule fires is kept)
    int32_t status;   // CdStatus of the lambda that failed, CD_OK otherwise
    int32_t fail_idx; // its index in the path
    int32_t _pad;
    int64_t clock0;   // wall_clock64() before the first lambda
};

template <class T>
struct CdPinPath {
    const T* lmdas;  // [L]
    int32_t L;
    int32_t cov;     // 0: naive exit rules (adev / ddev), 1: covariance method (rdev)
    T adev_thr;      // adev_tol * y_var
    T ddev_thr;      // ddev_tol * y_var
    T rdev_tol;
    T* snap_beta;    // [L, nv] the screen coefficients after each lambda
    T* snap_g;       // [L, nv] the screen gradient after each lambda, or nullptr
    CdPinRow<T>* rows; // [L]
    CdPinOut* out;
};

// the exit rules of a pin path after row l, in T (pin_naive:398-399, pin_cov:703); shared by the device loop and the host route
template <class T>
__host__ __device__ inline bool pin_path_exit(int cov, int l, T rsq, T rsq_prev, T adev_thr, T ddev_thr, T rdev_tol) {
    const T inc = rsq - rsq_prev;
    if (cov) {
        const T thr = rdev_tol * rsq;
        return l >= 1 && inc <= thr;
    }
    if (rsq >= adev_thr) return true;
    return l >= 1 && inc <= ddev_thr;
}

// One launch for the whole path; same territory as launch_cd (throws where launch_cd would).  p.lmda is not read.
template <class T> void launch_cd_pin(const CdParams<T>& p, const CdPinPath<T>& pp, hipStream_t s);

} // namespace ahip
