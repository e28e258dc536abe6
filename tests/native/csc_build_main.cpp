// Stand-alone check of the host side of the designs kept sparse (adelie_amd/csrc/csc_build_host.hpp), built with
// -fsanitize=address,undefined by tests/test_csc_build_host.py, which writes the arrays and judges what is printed.
//
//   csc_build_main validate n p value_bytes indptr indices values row_indptr row_indices row_values
//       prints "ok" or the message of csc_validate_pair
//   csc_build_main offsets n_cols_counted n_cols_out nt n col_cnt row_cnt out
//       prints "ok" or the message of csc_offsets_from_counts and writes cptr, col_pos, rptr and the total (int64 each) to `out`
//
// Every array is a raw file and sits in a heap block of exactly its length, so that a read past its end is the sanitizer's.
// The row counts are summed in place (row_cnt copied to rptr + 1), as the device builds do.
#include "../../adelie_amd/csrc/csc_build_host.hpp"
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <string>

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
    if (mode == "validate" && argc == 11) {
        const int64_t n = std::atoll(argv[2]), p = std::atoll(argv[3]);
        const size_t vb = size_t(std::atoll(argv[4]));
        const auto indptr = slurp<int64_t>(argv[5]), rptr = slurp<int64_t>(argv[8]);
        const auto indices = slurp<int32_t>(argv[6]), rcol = slurp<int32_t>(argv[9]);
        const auto values = slurp<uint8_t>(argv[7]), rval = slurp<uint8_t>(argv[10]);
        if (indptr.size() != size_t(p) + 1 || rptr.size() != size_t(n) + 1) { std::printf("bad pointer arrays\n"); return 2; }
        const char* e = csc_validate_pair(indptr.data(), indices.data(), values.data(), rptr.data(), rcol.data(), rval.data(), n, p, vb);
        std::printf("%s\n", e ? e : "ok");
        return 0;
    }
    if (mode == "offsets" && argc == 9) {
        const int64_t counted = std::atoll(argv[2]), cols = std::atoll(argv[3]), nt = std::atoll(argv[4]), n = std::atoll(argv[5]);
        const auto col_cnt = slurp<int32_t>(argv[6]);
        const auto row_cnt = slurp<int64_t>(argv[7]);
        if (col_cnt.size() != size_t(counted * nt) || row_cnt.size() != size_t(n)) { std::printf("bad counts\n"); return 2; }
        std::vector<int64_t> cptr(size_t(cols) + 1, -1), col_pos(size_t(cols * nt), -1), rptr(size_t(n) + 1, -1);
        std::copy(row_cnt.begin(), row_cnt.end(), rptr.begin() + 1);
        int64_t total = -1;
        const char* e = csc_offsets_from_counts(col_cnt.data(), counted, cols, nt, rptr.data() + 1, n, cptr.data(), col_pos.data(), rptr.data(), &total);
        std::printf("%s\n", e ? e : "ok");
        std::FILE* f = std::fopen(argv[8], "wb");
        if (!f) { std::printf("cannot write %s\n", argv[8]); return 2; }
        std::fwrite(cptr.data(), 8, cptr.size(), f);
        std::fwrite(col_pos.data(), 8, col_pos.size(), f);
        std::fwrite(rptr.data(), 8, rptr.size(), f);
        std::fwrite(&total, 8, 1, f);
        std::fclose(f);
        return 0;
    }
    std::printf("usage: %s validate|offsets ...\n", argv[0]);
    return 2;
}
