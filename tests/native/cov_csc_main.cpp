// Stand-alone check of the host side of the covariance matrix kept sparse (adelie_amd/csrc/cov_csc_host.hpp), built with
// -fsanitize=address,undefined by tests/test_cov_sparse_host.py, which writes the arrays and judges what is printed.
//
//   cov_csc_main validate p indptr indices values
//       prints "ok" or the message of cov_csc_validate
//   cov_csc_main lanes nnz p
//       prints cov_csc_lanes(nnz, p)
//   cov_csc_main cover ncols lanes
//       walks every (block, group) of cov_csc_shape(ncols, lanes) as the kernels do and prints "ok <blocks> <cols_per_block>" when
//       every column in [0, ncols) is met exactly once and nothing else is, "bad <column>" otherwise
//
// Every array is a raw file and sits in a heap block of exactly its length, so that a read past its end is the sanitizer's.
#include "../../adelie_amd/csrc/cov_csc_host.hpp"
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

using namespace ahip;

template <class T>
static std::vector<T> slurp(const char* path) {
    std::vector<uint8_t> raw;
    std::FILE* f = std::fopen(path, "rb");
    if (!f) { std::printf("cannot open %s\n", path); std::exit(2); }
    uint8_t buf[4096];
    for (size_t k; (k = std::fread(buf, 1, sizeof buf, f)) > 0;) raw.insert(raw.end(), buf, buf + k);
    std::fclose(f);
    std::vector<T> out(raw.size() / sizeof(T)); // capacity == size: the redzone starts at the last element
    if (!raw.empty()) std::memcpy(out.data(), raw.data(), out.size() * sizeof(T));
    return out;
}

int main(int argc, char** argv) {
    const std::string mode = argc > 1 ? argv[1] : "";
    if (mode == "validate" && argc == 6) {
        const int64_t p = std::atoll(argv[2]);
        const auto indptr = slurp<int64_t>(argv[3]);
        const auto indices = slurp<int32_t>(argv[4]);
        const auto values = slurp<uint8_t>(argv[5]);
        if (indptr.size() != size_t(p) + 1) { std::printf("bad pointer array\n"); return 2; }
        const char* e = cov_csc_validate(indptr.data(), indices.data(), values.data(), p);
        std::printf("%s\n", e ? e : "ok");
        return 0;
    }
    if (mode == "lanes" && argc == 4) {
        std::printf("%d\n", cov_csc_lanes(std::atoll(argv[2]), std::atoll(argv[3])));
        return 0;
    }
    if (mode == "cover" && argc == 4) {
        const int64_t ncols = std::atoll(argv[2]);
        const CovCscShape sh = cov_csc_shape(ncols, std::atoi(argv[3]));
        std::vector<int32_t> met(static_cast<size_t>(ncols), 0);
        if (sh.lanes * sh.cols_per_block != kCovCscBlock) { std::printf("bad block\n"); return 0; }
        for (int64_t b = 0; b < sh.blocks; ++b)
            for (int t = 0; t < kCovCscBlock; t += sh.lanes) { // lane 0 of every group
                const int64_t j = b * sh.cols_per_block + t / sh.lanes;
                if (j < ncols) ++met[size_t(j)];
            }
        for (int64_t j = 0; j < ncols; ++j)
            if (met[size_t(j)] != 1) { std::printf("bad %lld\n", static_cast<long long>(j)); return 0; }
        std::printf("ok %lld %d\n", static_cast<long long>(sh.blocks), sh.cols_per_block);
        return 0;
    }
    std::printf("usage: %s validate|lanes|cover ...\n", argv[0]);
    return 2;
}
