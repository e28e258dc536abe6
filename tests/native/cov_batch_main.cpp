// Stand-alone check of the host side of the lambda-batched covariance product (adelie_amd/csrc/cov_batch_host.hpp), built with
// -fsanitize=address,undefined by tests/test_cov_diag_host.py, which writes the arrays and judges what is printed.
//
//   cov_batch_main validate L p indptr indices
//       prints "ok" or the message of cov_batch_validate (the values are a block of 8 bytes per index, never read)
//   cov_batch_main chunk p elem
//       prints cov_batch_chunk_rows(p, elem)
//   cov_batch_main plan L p elem indptr indices values
//       validates, then walks the rows in chunks of cov_batch_chunk_rows(p, elem) as the launcher does and prints, per chunk,
//       "chunk <l0> <lc> <batches>" and per batch "batch <n>" followed by n lines "<column> <coef 0> ... <coef Lb-1>" (float64
//       values, printed with %.17g)
//
// Every array is a raw file and sits in a heap block of exactly its length, so that a read past its end is the sanitizer's.
#include "../../adelie_amd/csrc/cov_batch_host.hpp"
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
        const int64_t L = std::atoll(argv[2]), p = std::atoll(argv[3]);
        const auto indptr = slurp<int64_t>(argv[4]);
        const auto indices = slurp<int64_t>(argv[5]);
        if (L > 0 && indptr.size() != size_t(L) + 1) { std::printf("bad pointer array\n"); return 2; }
        const std::vector<double> values(indices.size(), 0.0);
        const char* e = cov_batch_validate(L, L > 0 ? indptr.data() : nullptr, indices.data(), values.data(), p);
        std::printf("%s\n", e ? e : "ok");
        return 0;
    }
    if (mode == "chunk" && argc == 4) {
        std::printf("%lld\n", static_cast<long long>(cov_batch_chunk_rows(std::atoll(argv[2]), size_t(std::atoll(argv[3])))));
        return 0;
    }
    if (mode == "plan" && argc == 8) {
        const int64_t L = std::atoll(argv[2]), p = std::atoll(argv[3]);
        const size_t elem = size_t(std::atoll(argv[4]));
        const auto indptr = slurp<int64_t>(argv[5]);
        const auto indices = slurp<int64_t>(argv[6]);
        const auto values = slurp<double>(argv[7]);
        if (L > 0 && indptr.size() != size_t(L) + 1) { std::printf("bad pointer array\n"); return 2; }
        if (const char* e = cov_batch_validate(L, L > 0 ? indptr.data() : nullptr, indices.data(), values.data(), p)) {
            std::printf("%s\n", e);
            return 0;
        }
        const int64_t chunk = cov_batch_chunk_rows(p, elem);
        CovBatchPlan<double> plan;
        for (int64_t l0 = 0; l0 < L; l0 += chunk) {
            const int64_t lc = std::min(chunk, L - l0);
            cov_batch_plan_unions<double>(l0, lc, indptr.data(), indices.data(), values.data(), plan);
            std::printf("chunk %lld %lld %lld\n", static_cast<long long>(l0), static_cast<long long>(lc),
                        static_cast<long long>(plan.batches()));
            if (plan.coef.size() != plan.ucols.size() * size_t(kCovBatchLb)) { std::printf("bad coef block\n"); return 0; }
            for (int64_t b = 0; b < plan.batches(); ++b) {
                std::printf("batch %lld\n", static_cast<long long>(plan.uptr[size_t(b) + 1] - plan.uptr[size_t(b)]));
                for (int64_t k = plan.uptr[size_t(b)]; k < plan.uptr[size_t(b) + 1]; ++k) {
                    std::printf("%d", plan.ucols[size_t(k)]);
                    for (int r = 0; r < kCovBatchLb; ++r) std::printf(" %.17g", plan.coef[size_t(k) * kCovBatchLb + size_t(r)]);
                    std::printf("\n");
                }
            }
        }
        std::printf("done\n");
        return 0;
    }
    std::printf("usage: %s validate|chunk|plan ...\n", argv[0]);
    return 2;
}
