// Prints, for a dense n x p design, the row-split counts adelie_amd/csrc/sweep_shape.hpp gives the f64 sweep with 16-byte loads,
// the float32 shadow sweep and the 16-bit shadow sweep, then the 16-bit sweep's panel width and the padding of its leading
// dimension.  Built and run by tests/test_gpu_filter_q15.py.
#include "../../adelie_amd/csrc/sweep_shape.hpp"

#include <cstdio>
#include <cstdlib>

int main(int argc, char** argv) {
    if (argc != 3) return 2;
    const int64_t n = std::atoll(argv[1]), p = std::atoll(argv[2]);
    int64_t blocks_c, rps;
    int ns_f64, ns_f32, ns_q15;
    ahip::sweep_shape(n, p, 2, blocks_c, ns_f64, rps);
    ahip::sweep_shape(n, p, ahip::kShadowVec, blocks_c, ns_f32, rps, ahip::kShadowCB);
    ahip::sweep_shape(n, p, ahip::kShadowVec16, blocks_c, ns_q15, rps, ahip::kShadowCB16);
    std::printf("%d %d %d %d %d\n", ns_f64, ns_f32, ns_q15, ahip::kShadowCB16, ahip::kShadowPad16);
    return 0;
}
