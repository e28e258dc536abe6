// kernels_cd.hip — the block-coordinate-descent pin solver for one lambda, resident on one CU (gfx950): the kernel around the
// body of cd_path_body.hpp (which documents the algorithm and cites the reference lines) and its launch.
#include "cd_path_body.hpp"
#include <stdexcept>
#include <string>

namespace ahip {

namespace {

template <class T, int NT, bool GLDS>
__global__ __launch_bounds__(NT) void cd_kernel(CdParams<T> p) {
    extern __shared__ __attribute__((aligned(16))) char smem_raw[];
    cd_path_body<T, NT, GLDS, false>(p, CdPinPath<T>{}, smem_raw);
}

} // namespace

template <class T> bool launch_cd_lasso(const CdParams<T>& p, hipStream_t s); // kernels_cd_lasso.hip

template <class T>
void launch_cd(const CdParams<T>& p, hipStream_t s) {
    if (launch_cd_lasso<T>(p, s)) return;
    constexpr int NT = 256;
    const size_t base = size_t(8 * p.max_group_size + 8) * sizeof(T);
    const size_t with_g = base + size_t(p.nv) * sizeof(T);
    const size_t lds_cap = 150 * 1024; // of the 160 KiB per CU; the static cnt[] array takes ~1 KiB
    // the dynamic-LDS limit of both instantiations is raised once, to the cap (see launch_k in kernels_cd_lasso.hip: a
    // per-call value races between the threads of concurrent solves)
    static const bool raised = [] {
        (void)hipFuncSetAttribute(reinterpret_cast<const void*>(cd_kernel<T, NT, true>), hipFuncAttributeMaxDynamicSharedMemorySize,
                                  150 * 1024);
        (void)hipFuncSetAttribute(reinterpret_cast<const void*>(cd_kernel<T, NT, false>), hipFuncAttributeMaxDynamicSharedMemorySize,
                                  150 * 1024);
        return true;
    }();
    (void)raised;
    (void)hipGetLastError(); // (whatever an earlier call of this thread left behind, e.g. an allocation the pool retried)
    if (with_g <= lds_cap) {
        hipLaunchKernelGGL((cd_kernel<T, NT, true>), dim3(1), dim3(NT), with_g, s, p);
    } else {
        if (base > lds_cap) throw std::runtime_error("adelie_core: a group is too large for the single-workgroup coordinate descent.");
        hipLaunchKernelGGL((cd_kernel<T, NT, false>), dim3(1), dim3(NT), base, s, p);
    }
    if (const hipError_t e = hipGetLastError(); e != hipSuccess) // a refused launch must not pass for a solve
        throw std::runtime_error(std::string("adelie_hip: HIP error '") + hipGetErrorString(e) + "' launching cd_kernel");
}

template void launch_cd<double>(const CdParams<double>&, hipStream_t);
template void launch_cd<float>(const CdParams<float>&, hipStream_t);

} // namespace ahip
