// kernels_cd_pin.hip — a whole pin path in one launch (gfx950): the PATH = true forms of the two single-workgroup descents.
//
// The per-lambda work is the text of cd_path_body.hpp / cd_lasso_path_body.hpp, the same text the single-lambda kernels
// instantiate, so a lambda solved here does the operations of a lambda solved by launch_cd in the same order.  Around it,
// on the device: g (and the lasso form's active flags) are staged in LDS once, the loop runs over the lambdas of CdPinPath,
// `iters` runs on from lambda to lambda against the one max_iters (pin_naive:356, pin_cov:676), and after every lambda row l
// of the snapshot block is written (coefficients, the gradient when asked for, rsq, resid_sum, active size, the counters)
// and the exit rules are taken (pin_path_exit, cd_pin.hpp).  Every loop is bounded by max_iters or newton_max_iters; a lambda
// that fails ends the launch with its status and index in CdPinOut.  One workgroup, no atomics: reruns give the same bits.
//
// The kernel selection (lasso form with K register-resident chunks of g, else the grouped form with g in LDS or in global
// memory) is launch_cd's, so the two routes always run the same form on the same problem.
#include "cd_lasso_path_body.hpp"
#include <stdexcept>
#include <string>

namespace ahip {

namespace {

template <class T, int NT, bool GLDS>
__global__ __launch_bounds__(NT) void cd_pin_kernel(CdParams<T> p, CdPinPath<T> pp) {
    extern __shared__ __attribute__((aligned(16))) char smem_raw[];
    cd_path_body<T, NT, GLDS, true>(p, pp, smem_raw);
}

template <class T, int NT, int K, bool TAIL>
__global__ __launch_bounds__(NT) void cd_pin_lasso_kernel(CdParams<T> p, CdPinPath<T> pp) {
    extern __shared__ __attribute__((aligned(16))) char smem_raw[];
    cd_lasso_path_body<T, NT, K, TAIL, true>(p, pp, smem_raw);
}

void check_launch(const char* what) {
    if (const hipError_t e = hipGetLastError(); e != hipSuccess) // a refused launch must not pass for a solve
        throw std::runtime_error(std::string("adelie_hip: HIP error '") + hipGetErrorString(e) + "' launching " + what);
}

template <class T, int NT, int K>
void launch_pin_k(const CdParams<T>& p, const CdPinPath<T>& pp, size_t bytes, bool tail, hipStream_t s) {
    auto k = tail ? cd_pin_lasso_kernel<T, NT, K, true> : cd_pin_lasso_kernel<T, NT, K, false>;
    static const bool raised = [] { // once per instantiation, to the cap (see launch_k in kernels_cd_lasso.hip)
        (void)hipFuncSetAttribute(reinterpret_cast<const void*>(cd_pin_lasso_kernel<T, NT, K, true>),
                                  hipFuncAttributeMaxDynamicSharedMemorySize, 150 * 1024);
        (void)hipFuncSetAttribute(reinterpret_cast<const void*>(cd_pin_lasso_kernel<T, NT, K, false>),
                                  hipFuncAttributeMaxDynamicSharedMemorySize, 150 * 1024);
        return true;
    }();
    (void)raised;
    (void)hipGetLastError();
    hipLaunchKernelGGL(k, dim3(1), dim3(NT), bytes, s, p, pp);
    check_launch("cd_pin_lasso_kernel");
}

// the lasso form, under the conditions of launch_cd_lasso
template <class T>
bool launch_cd_pin_lasso(const CdParams<T>& p, const CdPinPath<T>& pp, hipStream_t s) {
    if (!(p.all_scalar && p.nv == p.ns)) return false;
    constexpr int NT = 512, KMAX = 8, VEC = 16 / sizeof(T);
    const size_t lds_cap = 150 * 1024;
    const size_t nvp = size_t((p.nv + NT * VEC - 1) / (NT * VEC)) * (NT * VEC);
    const size_t bytes = nvp * sizeof(T) + size_t(p.ns) + 16;
    if (bytes > lds_cap || int64_t(nvp) > p.ldc) return false;
    const int kmax = int(nvp / (NT * VEC));
    switch (kmax < KMAX ? kmax : KMAX) {
        case 1: launch_pin_k<T, NT, 1>(p, pp, bytes, false, s); break;
        case 2: launch_pin_k<T, NT, 2>(p, pp, bytes, false, s); break;
        case 3: launch_pin_k<T, NT, 3>(p, pp, bytes, false, s); break;
        case 4: launch_pin_k<T, NT, 4>(p, pp, bytes, false, s); break;
        case 5: launch_pin_k<T, NT, 5>(p, pp, bytes, false, s); break;
        case 6: launch_pin_k<T, NT, 6>(p, pp, bytes, false, s); break;
        case 7: launch_pin_k<T, NT, 7>(p, pp, bytes, false, s); break;
        default: launch_pin_k<T, NT, 8>(p, pp, bytes, kmax > KMAX, s); break;
    }
    return true;
}

} // namespace

template <class T>
void launch_cd_pin(const CdParams<T>& p, const CdPinPath<T>& pp, hipStream_t s) {
    if (pp.L <= 0) throw std::runtime_error("adelie_core: launch_cd_pin needs a non-empty lambda path.");
    if (launch_cd_pin_lasso<T>(p, pp, s)) return;
    constexpr int NT = 256;
    const size_t base = size_t(8 * p.max_group_size + 8) * sizeof(T);
    const size_t with_g = base + size_t(p.nv) * sizeof(T);
    const size_t lds_cap = 150 * 1024; // of the 160 KiB per CU; the static cnt[] array takes ~1 KiB
    static const bool raised = [] {
        (void)hipFuncSetAttribute(reinterpret_cast<const void*>(cd_pin_kernel<T, NT, true>), hipFuncAttributeMaxDynamicSharedMemorySize,
                                  150 * 1024);
        (void)hipFuncSetAttribute(reinterpret_cast<const void*>(cd_pin_kernel<T, NT, false>), hipFuncAttributeMaxDynamicSharedMemorySize,
                                  150 * 1024);
        return true;
    }();
    (void)raised;
    (void)hipGetLastError();
    if (with_g <= lds_cap) {
        hipLaunchKernelGGL((cd_pin_kernel<T, NT, true>), dim3(1), dim3(NT), with_g, s, p, pp);
    } else {
        if (base > lds_cap) throw std::runtime_error("adelie_core: a group is too large for the single-workgroup coordinate descent.");
        hipLaunchKernelGGL((cd_pin_kernel<T, NT, false>), dim3(1), dim3(NT), base, s, p, pp);
    }
    check_launch("cd_pin_kernel");
}

template void launch_cd_pin<double>(const CdParams<double>&, const CdPinPath<double>&, hipStream_t);
template void launch_cd_pin<float>(const CdParams<float>&, const CdPinPath<float>&, hipStream_t);

} // namespace ahip
