// phased_decode_host.hpp — host side of matrix.snp_phased_ancestry: plain C++, no HIP, so that tests/native/
// phased_decode_main.cpp can run it as a stand-alone program under the address and undefined-behaviour sanitizers.
//
// Both routes into the design end in the same CODE TABLE: a column-major uint8 (n, 2 s) array whose column 2 j + k is
// haplotype k of SNP j and whose entry is the ancestry where the call is 1 and kPhasedNone (255) where it is 0 -- free as a
// sentinel because the format keeps A < 256.  kernels_phased.hip builds the compressed arrays of the design from it.
//
//   phased_header / phased_decode   a .snpdat image of the phased-ancestry format (io_snp_phased_ancestry.ipp:10-42,143-347):
//       [u8 is_big_endian][u64 n][u64 s][u8 A][u64 nnz0[s A]][u64 nnz1[s A]][u64 outer[s + 1]]      outer[] absolute
//       SNP j at outer[j]:             [u64 anc_off[A]]   relative to the SNP block
//         ancestry a at anc_off[a]:    [u64 hap_off[2]]   relative to the ancestry block
//           haplotype k at hap_off[k]: [u32 n_chunks], per non-empty 256-row chunk [u32 chunk_idx][u8 nnz-1][u8 row * nnz]
//   phased_pack                     a (calldata, ancestries) pair of column-major int8 (n, 2 s) arrays, validated as the
//                                   reference's writer validates them (io_snp_phased_ancestry.ipp:84-100,207-214,234-249).
//
// Every function returns nullptr on success and a message otherwise (the caller raises it as a core_error).  The decoder
// trusts nothing in the image: every offset, chunk header and run of row bytes is checked against the end of its SNP block
// BEFORE it is read, every row against n before it is written (the chunk walk is snp_decode_host.hpp's, shared with the
// unphased format).
#pragma once
#include <cstdint>
#include <cstring>
#include "snp_decode_host.hpp" // phased_read_u64 / _u32, snp_walk_chunks

namespace ahip {

constexpr int64_t kPhasedTileRows = 4096; // rows per (SNP, tile) workgroup of kernels_phased.hip
constexpr uint8_t kPhasedNone = 255;      // "no mutation" in the code table
constexpr uint64_t kPhasedChunk = kSnpChunk; // rows per chunk of the file format

struct PhasedDims {
    uint64_t n = 0, s = 0, A = 0;
    uint64_t header_bytes() const { return 18 + 16 * s * A + 8 * (s + 1); }
};

// The counts of the image, bounded by what the image can hold before anything is sized from them: a SNP costs at least its
// outer entry and, per ancestry, two nnz counts, one ancestry offset, two haplotype offsets and two chunk counts.
inline const char* phased_header(const uint8_t* buf, uint64_t n_bytes, PhasedDims* out) {
    if (!buf || n_bytes < 18) return "buffer is too small to be a phased-ancestry .snpdat image.";
    if (buf[0] != 0) return "Endianness is inconsistent! Regenerate the file on this machine.";
    PhasedDims d;
    d.n = phased_read_u64(buf + 1);
    d.s = phased_read_u64(buf + 9);
    d.A = buf[17];
    if (d.A < 1) return "corrupt .snpdat header (no ancestries).";
    if (d.n == 0 || d.s == 0) return "corrupt .snpdat header (row / SNP counts).";
    if (d.n >= (uint64_t(1) << 31)) return "number of rows must fit in int32.";
    if (d.s > n_bytes / (8 + 48 * d.A)) return "corrupt .snpdat header (row / SNP counts).";
    if (d.s * d.A >= (uint64_t(1) << 31)) return "number of columns must fit in int32.";
    if (n_bytes < d.header_bytes()) return "truncated .snpdat header.";
    *out = d;
    return nullptr;
}

// `table` holds n * 2 s bytes; it is filled here (kPhasedNone, then the stored calls).
inline const char* phased_decode(const uint8_t* buf, uint64_t n_bytes, const PhasedDims& d, uint8_t* table) {
    const uint64_t n = d.n, s = d.s, A = d.A, hdr = d.header_bytes();
    const uint8_t* outer = buf + 18 + 16 * s * A;
    std::memset(table, kPhasedNone, size_t(n) * size_t(2 * s));
    for (uint64_t j = 0; j < s; ++j) {
        const uint64_t base = phased_read_u64(outer + 8 * j), endc = phased_read_u64(outer + 8 * (j + 1));
        if (endc > n_bytes || base < hdr || base > endc || endc - base < 8 * A) return "corrupt .snpdat SNP index.";
        for (uint64_t a = 0; a < A; ++a) {
            const uint64_t aoff = phased_read_u64(buf + base + 8 * a);
            if (aoff > endc - base || endc - base - aoff < 16) return "corrupt .snpdat ancestry offset.";
            const uint64_t ablk = base + aoff;
            for (uint64_t k = 0; k < 2; ++k) {
                const uint64_t hoff = phased_read_u64(buf + ablk + 8 * k);
                if (hoff > endc - ablk || endc - ablk - hoff < 4) return "corrupt .snpdat haplotype offset.";
                uint8_t* col = table + size_t(2 * j + k) * size_t(n);
                const char* e = snp_walk_chunks(buf, ablk + hoff, endc, n, [&](uint64_t row) -> const char* {
                    if (col[row] != kPhasedNone) return "corrupt .snpdat chunk (a haplotype stored twice).";
                    col[row] = uint8_t(a);
                    return nullptr;
                });
                if (e) return e;
            }
        }
    }
    return nullptr;
}

// Dimension checks of the calldata route (before the table is allocated).
inline const char* phased_pack_dims(int64_t n, int64_t s, int64_t A) {
    if (n <= 0 || s <= 0) return "calldata and ancestries must have shape (n, 2*s).";
    if (A >= int64_t(kPhasedChunk)) return "Number of ancestries A must be < 256.";
    if (A < 1) return "Number of ancestries A must be >= 1.";
    if (n >= (int64_t(1) << 31)) return "number of rows must fit in int32.";
    if (s >= (int64_t(1) << 31) / A) return "number of columns must fit in int32.";
    return nullptr;
}

// Column-major int8 (n, 2 s) calldata / ancestries -> the code table.  As in the reference every ancestry must lie in
// [0, A), also where the call is 0 (there its value is not used), and every call must be 0 or 1.
inline const char* phased_pack(const int8_t* calldata, const int8_t* ancestries, int64_t n, int64_t s, int64_t A, uint8_t* table) {
    const size_t cells = size_t(n) * size_t(2 * s);
    for (size_t k = 0; k < cells; ++k) {
        const int8_t an = ancestries[k], ca = calldata[k];
        if (an < 0 || int64_t(an) >= A)
            return "Detected an ancestry not in the range [0, A). Make sure ancestries only contains values in [0, A). ";
        if (ca != 0 && ca != 1) return "Detected a non-binary value. Make sure calldata only contains 0 or 1 values. ";
        table[k] = ca ? uint8_t(an) : kPhasedNone;
    }
    return nullptr;
}

} // namespace ahip
