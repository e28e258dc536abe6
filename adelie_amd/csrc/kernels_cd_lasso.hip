// kernels_cd_lasso.hip — coordinate-descent pin solver for one lambda, lasso specialisation: the kernel around the body of
// cd_lasso_path_body.hpp (which documents it) and its launch.
#include "cd_lasso_path_body.hpp"
#include <stdexcept>
#include <string>

namespace ahip {

namespace {

template <class T, int NT, int K, bool TAIL>
__global__ __launch_bounds__(NT) void cd_lasso_kernel(CdParams<T> p) {
    extern __shared__ __attribute__((aligned(16))) char smem_raw[];
    cd_lasso_path_body<T, NT, K, TAIL, false>(p, CdPinPath<T>{}, smem_raw);
}

} // namespace

// Returns false when the problem does not fit this specialisation (the caller then uses the generic kernel).
// The kernel is instantiated per number of 512-lane x 16-byte chunks of g (K = 1..8, exactly the chunks in use: every
// load instruction moves 8 KB through the CU's vector cache whether it hits or not, so none is issued in vain);
// longer screen sets use K = 8 plus an on-demand tail.
template <class T, int NT, int K>
static void launch_k(const CdParams<T>& p, size_t bytes, bool tail, hipStream_t s) {
    auto k = tail ? cd_lasso_kernel<T, NT, K, true> : cd_lasso_kernel<T, NT, K, false>;
    // The limit is raised ONCE per instantiation, to the most any launch asks for (thread-safe static initialisation).  It used
    // to be set to this launch's size on every call: with several solves in flight (the folds of cv_grpnet run on threads) one
    // thread could lower it between another thread's call and its launch, and a launch above the limit does not run.
    static const bool raised = [] {
        (void)hipFuncSetAttribute(reinterpret_cast<const void*>(cd_lasso_kernel<T, NT, K, true>),
                                  hipFuncAttributeMaxDynamicSharedMemorySize, 150 * 1024);
        (void)hipFuncSetAttribute(reinterpret_cast<const void*>(cd_lasso_kernel<T, NT, K, false>),
                                  hipFuncAttributeMaxDynamicSharedMemorySize, 150 * 1024);
        return true;
    }();
    (void)raised;
    (void)hipGetLastError(); // (whatever an earlier call of this thread left behind, e.g. an allocation the pool retried)
    hipLaunchKernelGGL(k, dim3(1), dim3(NT), bytes, s, p);
    if (const hipError_t e = hipGetLastError(); e != hipSuccess) // a refused launch must not pass for a solve
        throw std::runtime_error(std::string("adelie_hip: HIP error '") + hipGetErrorString(e) + "' launching cd_lasso_kernel");
}

template <class T>
bool launch_cd_lasso(const CdParams<T>& p, hipStream_t s) {
    if (!(p.all_scalar && p.nv == p.ns)) return false;
    constexpr int NT = 512, KMAX = 8, VEC = 16 / sizeof(T);
    const size_t lds_cap = 150 * 1024; // of the 160 KiB per CU (static arrays take a few KiB)
    const size_t nvp = size_t((p.nv + NT * VEC - 1) / (NT * VEC)) * (NT * VEC);
    const size_t bytes = nvp * sizeof(T) + size_t(p.ns) + 16;
    if (bytes > lds_cap || int64_t(nvp) > p.ldc) return false;
    const int kmax = int(nvp / (NT * VEC));
    switch (kmax < KMAX ? kmax : KMAX) {
        case 1: launch_k<T, NT, 1>(p, bytes, false, s); break;
        case 2: launch_k<T, NT, 2>(p, bytes, false, s); break;
        case 3: launch_k<T, NT, 3>(p, bytes, false, s); break;
        case 4: launch_k<T, NT, 4>(p, bytes, false, s); break;
        case 5: launch_k<T, NT, 5>(p, bytes, false, s); break;
        case 6: launch_k<T, NT, 6>(p, bytes, false, s); break;
        case 7: launch_k<T, NT, 7>(p, bytes, false, s); break;
        default: launch_k<T, NT, 8>(p, bytes, kmax > KMAX, s); break;
    }
    return true;
}

template bool launch_cd_lasso<double>(const CdParams<double>&, hipStream_t);
template bool launch_cd_lasso<float>(const CdParams<float>&, hipStream_t);

} // namespace ahip
