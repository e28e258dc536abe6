// pieces_host.hpp — host side of a design made of column blocks that stay as they are (adelie_hip_design_create_pieces,
// matrix.concatenate(..., resident="pieces")): plain C++, no HIP, so that tests/native/pieces_main.cpp runs it as a stand-alone
// program under the address and undefined-behaviour sanitizers.  It holds what a caller may hand over (pieces_validate), the
// table of first columns, the map from a column to (piece, local column), the split of a column range into per-piece ranges
// and the rule for the 16-byte load path.
#pragma once
#include <cstdint>
#include <string>

namespace ahip {

// The descriptor of a pieces design travels by value in the kernel arguments (accessors.hpp: PiecesAcc), so the count is capped.
constexpr int kMaxPieces = 8;
// storage of one piece
constexpr int kPieceDense = 0, kPieceSnp = 1;

// What pieces_validate is told about a source handle: kind as adelie_hip_design::kind (0 dense, 1 2-bit, 2 multi-response view,
// 3 compressed columns, 4 pieces) and the marks that make a dense / 2-bit / compressed handle something else.
struct PieceInfo {
    int kind;
    bool std_view, cov, constraint;
    int dtype, device;
    int64_t n, p;
};

inline const char* piece_kind_name(const PieceInfo& s) {
    if (s.constraint) return "constraint matrix";
    if (s.cov) return "covariance matrix";
    if (s.kind == 2) return "multi-response view";
    if (s.kind == 4) return "pieces";
    if (s.std_view) return "standardized view";
    if (s.kind == 3) return "kept sparse";
    if (s.kind == 0) return "dense";
    if (s.kind == 1) return "snp";
    return "unknown";
}

// Empty when the k sources may stand side by side as pieces, else the refusal: it names the piece, its kind and
// resident="pieces", and says what works instead.
inline std::string pieces_validate(const PieceInfo* src, int64_t k) {
    const std::string tail = " (concatenate(..., resident=\"pieces\"); resident=\"auto\" copies the pieces into one design, on which everything works).";
    if (!src || k < 1) return "concatenate(): resident=\"pieces\" needs at least one piece.";
    if (k > kMaxPieces)
        return "concatenate(): " + std::to_string(k) + " pieces given, at most " + std::to_string(kMaxPieces) + " are kept as they are" + tail;
    int64_t p = 0;
    for (int64_t m = 0; m < k; ++m) {
        const PieceInfo& s = src[m];
        const std::string who = "piece " + std::to_string(m) + " (" + piece_kind_name(s) + ")";
        const bool plain = (s.kind == kPieceDense || s.kind == kPieceSnp) && !s.std_view && !s.cov && !s.constraint;
        if (!plain) return "concatenate(): " + who + " is neither a plain dense nor a plain 2-bit design" + tail;
        if (s.n < 1 || s.p < 1) return "concatenate(): " + who + " has no rows or no columns" + tail;
        if (s.dtype != src[0].dtype) return "concatenate(): " + who + " differs in dtype from piece 0" + tail;
        if (s.n != src[0].n) return "concatenate(): " + who + " differs in its number of rows from piece 0" + tail;
        if (s.device != src[0].device) return "concatenate(): " + who + " lives on another device than piece 0" + tail;
        p += s.p;
        if (p >= (int64_t(1) << 31)) return "concatenate(): the columns up to " + who + " do not fit in int32" + tail;
    }
    return std::string();
}

// first[m] = first column of piece m, first[k] = p, first[m > k] = INT32_MAX (no column reaches an unused slot)
inline void pieces_first_cols(const int64_t* p_of, int k, int32_t (&first)[kMaxPieces + 1]) {
    int64_t at = 0;
    for (int m = 0; m <= kMaxPieces; ++m) {
        first[m] = m <= k ? int32_t(at) : INT32_MAX;
        if (m < k) at += p_of[m];
    }
}

// the piece that holds column j (0 <= j < first[k]) and j's column inside it: the scan the device accessor makes
inline void pieces_locate(const int32_t (&first)[kMaxPieces + 1], int64_t j, int& piece, int64_t& local) {
    piece = 0;
    for (int m = 1; m < kMaxPieces; ++m)
        if (j >= int64_t(first[m])) piece = m;
    local = j - int64_t(first[piece]);
}

// Columns [c0, c0 + ncols) cut at the piece boundaries: `count` columns of piece `piece` from its column `local0`, which are
// outputs [out0, out0 + count) of the range.  Returns how many ranges there are (pieces the range does not meet give none).
struct PieceRange {
    int piece;
    int64_t local0, count, out0;
};
inline int pieces_split(const int32_t (&first)[kMaxPieces + 1], int k, int64_t c0, int64_t ncols, PieceRange (&out)[kMaxPieces]) {
    int nr = 0;
    for (int m = 0; m < k; ++m) {
        const int64_t lo = c0 > int64_t(first[m]) ? c0 : int64_t(first[m]);
        const int64_t hi = c0 + ncols < int64_t(first[m + 1]) ? c0 + ncols : int64_t(first[m + 1]);
        if (hi <= lo) continue;
        out[nr++] = PieceRange{m, lo - int64_t(first[m]), hi - lo, lo - c0};
    }
    return nr;
}

// Whether the kernels may read 16 bytes at a time (vec = elements per 16 bytes): every dense piece must pass the test a dense
// design passes on its own (leading dimension in whole vectors, base on a 16-byte boundary); a 2-bit piece always passes.
inline bool pieces_vec_ok(const int* kind, const uintptr_t* base, const int64_t* ld, int k, int vec) {
    for (int m = 0; m < k; ++m)
        if (kind[m] == kPieceDense && (ld[m] % vec != 0 || base[m] % 16 != 0)) return false;
    return true;
}

} // namespace ahip
