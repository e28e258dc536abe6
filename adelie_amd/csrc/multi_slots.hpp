// multi_slots.hpp — the per-feature slot lists of the multi-response panel steps (kernels_multi.hip, kernels_multi_sparse.hip).
#pragma once
#include <hip/hip_runtime.h>
#include <cstdint>

namespace ahip {

// slots of a list of view columns: returns the number of slots; feat[slot] = extended feature; for every entry m the
// callback gets (m, slot, response)
template <class F>
__device__ __forceinline__ int build_slots(const int32_t* __restrict__ list, int cnt, int K, int* feat, int lane, F f) {
    int nslot = 0;
    for (int base = 0; base < cnt; base += 64) {
        const int m = base + lane;
        const bool valid = m < cnt;
        const int col = valid ? list[m] : 0;
        const int u = col / K, l = col - u * K;
        const int pu = (valid && m > 0) ? list[m - 1] / K : -1;
        const bool head = valid && (m == 0 || u != pu);
        const unsigned long long mask = __ballot(head);
        const int slot = nslot + __popcll(mask & ((2ull << lane) - 1ull)) - 1;
        if (head) feat[slot] = u;
        if (valid) f(m, slot, l);
        nslot += __popcll(mask);
    }
    return nslot;
}

} // namespace ahip
