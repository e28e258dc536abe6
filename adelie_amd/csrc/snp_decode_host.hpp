// snp_decode_host.hpp — host side of the .snpdat readers: plain C++, no HIP, so that tests/native/snp_decode_main.cpp and
// phased_decode_main.cpp can run it as stand-alone programs under the address and undefined-behaviour sanitizers.
//
// The unphased format (io_snp_unphased.ipp:10-68,117-135,225-274; adelie_amd/io.py writes it):
//   [u8 is_big_endian][u64 n][u64 p][u64 nnz[p]][u64 nnm[p]][f64 impute[p]][u64 outer[p + 1]]        outer[] absolute
//   column j at outer[j]: [u64 cat_off[3]] relative to the column block; category 0 = missing, 1, 2, each a chunk list:
//   [u32 n_chunks], per non-empty 256-row chunk [u32 chunk_idx][u8 nnz-1][u8 row * nnz]  (the phased format ends in the same)
//
// Every function returns nullptr on success and a message otherwise (the caller raises it as a core_error).  Nothing in an
// image is trusted: every offset, chunk header and run of row bytes is checked against the end of its block BEFORE it is read,
// every row against n before it is handed on.
#pragma once
#include <cstdint>
#include <cstring>

namespace ahip {

constexpr uint64_t kSnpChunk = 256; // rows per chunk of the file formats

// unaligned reads (named for their first user, the phased reader)
inline uint64_t phased_read_u64(const uint8_t* p) { uint64_t v; std::memcpy(&v, p, sizeof v); return v; }
inline uint32_t phased_read_u32(const uint8_t* p) { uint32_t v; std::memcpy(&v, p, sizeof v); return v; }

// The chunk list whose [u32 n_chunks] lies at `pos` inside a block that ends at `endc` (the caller has checked that these four
// bytes lie inside it).  per_row(row) is called for every stored row < n and returns nullptr or the message to fail with.
template <class F>
inline const char* snp_walk_chunks(const uint8_t* buf, uint64_t pos, uint64_t endc, uint64_t n, F&& per_row) {
    const uint32_t n_chunks = phased_read_u32(buf + pos);
    pos += 4;
    for (uint32_t c = 0; c < n_chunks; ++c) {
        if (endc - pos < 5) return "corrupt .snpdat chunk (overrun).";
        const uint64_t cidx = phased_read_u32(buf + pos);
        const uint64_t cnt = uint64_t(buf[pos + 4]) + 1;
        pos += 5;
        if (endc - pos < cnt) return "corrupt .snpdat chunk (overrun).";
        for (uint64_t t = 0; t < cnt; ++t) {
            const uint64_t row = cidx * kSnpChunk + buf[pos + t];
            if (row >= n) return "corrupt .snpdat chunk (row out of range).";
            if (const char* e = per_row(row)) return e;
        }
        pos += cnt;
    }
    return nullptr;
}

struct SnpUnphasedDims {
    uint64_t n = 0, p = 0;
    uint64_t impute_at() const { return 17 + 16 * p; }
    uint64_t outer_at() const { return 17 + 24 * p; }
    uint64_t header_bytes() const { return 17 + 24 * p + 8 * (p + 1); }
};

// The header, bounded before anything is sized from it: every column costs 32 header bytes (nnz, nnm, impute, outer) plus its
// 24-byte offset table, which bounds p by the image size; the rows are only bounded by what the format can address, so a
// plausibility cap stands in (2^32 rows; the largest biobanks have < 2^24).  Then the column index, before anything is allocated.
inline const char* snp_unphased_header(const uint8_t* buf, uint64_t n_bytes, SnpUnphasedDims* out) {
    if (n_bytes < 17) return "buffer is too small to be a .snpdat image.";
    const SnpUnphasedDims d{phased_read_u64(buf + 1), phased_read_u64(buf + 9)};
    if (d.p == 0 || d.n == 0) return "corrupt .snpdat header (row / column counts).";
    if (d.p > n_bytes / 32 || d.n > (uint64_t(1) << 32)) return "corrupt .snpdat header (row / column counts).";
    const uint64_t hdr = d.header_bytes();
    if (n_bytes < hdr) return "truncated .snpdat header.";
    const uint8_t* outer = buf + d.outer_at();
    for (uint64_t j = 0; j < d.p; ++j) {
        const uint64_t base = phased_read_u64(outer + 8 * j), endc = phased_read_u64(outer + 8 * (j + 1));
        if (endc > n_bytes || base < hdr || base > endc || endc - base < 24) return "corrupt .snpdat column index.";
    }
    *out = d;
    return nullptr;
}

// The column block [base, endc) of an image that passed snp_unphased_header -> int8 calls (missing = -9; `col` zeroed by the caller).
inline const char* snp_unphased_decode_column(const uint8_t* buf, uint64_t base, uint64_t endc, uint64_t n, int8_t* col) {
    for (int c = 0; c < 3; ++c) {
        const uint64_t off = phased_read_u64(buf + base + 8 * c);
        if (off > endc - base || endc - base - off < 4) return "corrupt .snpdat category offset.";
        const int8_t val = c == 0 ? int8_t(-9) : int8_t(c);
        if (const char* e = snp_walk_chunks(buf, base + off, endc, n, [&](uint64_t row) -> const char* { col[row] = val; return nullptr; })) return e;
    }
    return nullptr;
}

} // namespace ahip
