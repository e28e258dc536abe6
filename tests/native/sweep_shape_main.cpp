// Prints the row-split counts adelie_amd/csrc/sweep_shape.hpp gives a dense n x p design: the f64 sweep with 16-byte loads,
// the f64 sweep with scalar loads and the float32 shadow sweep.  Built and run by tests/test_gpu_filter_fused.py.
#include "../../adelie_amd/csrc/sweep_shape.hpp"

#include <cstdio>
#include <cstdlib>

int main(int argc, char** argv) {
    if (argc != 3) return 2;
    const int64_t n = std::atoll(argv[1]), p = std::atoll(argv[2]);
    int64_t blocks_c, rps;
    int ns_vec, ns_scalar, ns_shadow;
    ahip::sweep_shape(n, p, 2, blocks_c, ns_vec, rps);
    ahip::sweep_shape(n, p, 1, blocks_c, ns_scalar, rps);
    ahip::sweep_shape(n, p, ahip::kShadowVec, blocks_c, ns_shadow, rps, ahip::kShadowCB);
    std::printf("%d %d %d %d\n", ns_vec, ns_scalar, ns_shadow, ahip::kShadowCB);
    return 0;
}
