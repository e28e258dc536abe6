// Stand-alone check of the host side of a design made of pieces (adelie_amd/csrc/pieces_host.hpp), built with
// -fsanitize=address,undefined by tests/test_pieces_host.py: the refusals and their messages, the table of first columns, the
// column -> (piece, local column) map at every boundary, the split of column ranges and the rule for 16-byte loads.  Exits
// non-zero on the first disagreement.
#include "../../adelie_amd/csrc/pieces_host.hpp"
#include <cstdio>
#include <cstring>
#include <random>
#include <vector>

using namespace ahip;

static int fails = 0;
#define CHECK(c) do { if (!(c)) { std::printf("FAILED line %d: %s\n", __LINE__, #c); ++fails; } } while (0)

static bool has(const std::string& s, const char* what) { return s.find(what) != std::string::npos; }
// a refusal names the piece, its kind and resident="pieces", and says what works instead
static bool refusal(const std::string& s, const char* piece, const char* why) {
    return has(s, piece) && has(s, why) && has(s, "resident=\"pieces\"") && has(s, "resident=\"auto\"");
}
static PieceInfo plain(int kind, int64_t n, int64_t p) { return PieceInfo{kind, false, false, false, 1, 0, n, p}; }

int main() {
    // ---- validation -------------------------------------------------------------------------------------------------------
    {
        std::vector<PieceInfo> v = {plain(0, 50, 3), plain(1, 50, 7), plain(0, 50, 2), plain(1, 50, 5)};
        CHECK(pieces_validate(v.data(), 4).empty());
        CHECK(pieces_validate(v.data(), 1).empty());
        std::vector<PieceInfo> same(kMaxPieces, plain(1, 9, 4)); // the same kind repeated, up to the cap
        CHECK(pieces_validate(same.data(), kMaxPieces).empty());
        same.push_back(plain(1, 9, 4));
        const std::string cap = pieces_validate(same.data(), kMaxPieces + 1);
        CHECK(has(cap, "9 pieces") && has(cap, "at most 8") && has(cap, "resident=\"pieces\"") && has(cap, "resident=\"auto\""));
        CHECK(!pieces_validate(v.data(), 0).empty() && !pieces_validate(nullptr, 2).empty());

        auto bad = [&](int at, PieceInfo s) {
            std::vector<PieceInfo> w = v;
            w[size_t(at)] = s;
            return pieces_validate(w.data(), int64_t(w.size()));
        };
        PieceInfo s = plain(3, 50, 7);
        CHECK(refusal(bad(1, s), "piece 1 (kept sparse)", "neither a plain dense nor a plain 2-bit"));
        s = plain(2, 50, 7);
        CHECK(refusal(bad(2, s), "piece 2 (multi-response view)", "neither a plain dense nor a plain 2-bit"));
        s = plain(4, 50, 7);
        CHECK(refusal(bad(0, s), "piece 0 (pieces)", "neither a plain dense nor a plain 2-bit"));
        s = plain(1, 50, 7), s.std_view = true;
        CHECK(refusal(bad(3, s), "piece 3 (standardized view)", "neither a plain dense nor a plain 2-bit"));
        s = plain(3, 50, 7), s.std_view = true; // the standardized view of a design kept sparse
        CHECK(refusal(bad(3, s), "piece 3 (standardized view)", "neither a plain dense nor a plain 2-bit"));
        s = plain(0, 50, 50), s.cov = true;
        CHECK(refusal(bad(2, s), "piece 2 (covariance matrix)", "neither a plain dense nor a plain 2-bit"));
        s = plain(3, 50, 50), s.cov = true;
        CHECK(refusal(bad(2, s), "piece 2 (covariance matrix)", "neither a plain dense nor a plain 2-bit"));
        s = plain(0, 50, 4), s.constraint = true;
        CHECK(refusal(bad(1, s), "piece 1 (constraint matrix)", "neither a plain dense nor a plain 2-bit"));
        s = plain(1, 50, 7), s.dtype = 0;
        CHECK(refusal(bad(1, s), "piece 1 (snp)", "dtype"));
        s = plain(0, 51, 2);
        CHECK(refusal(bad(2, s), "piece 2 (dense)", "number of rows"));
        s = plain(1, 50, 5), s.device = 3;
        CHECK(refusal(bad(3, s), "piece 3 (snp)", "another device"));
        s = plain(0, 50, 0);
        CHECK(refusal(bad(2, s), "piece 2 (dense)", "no rows or no columns"));
        std::vector<PieceInfo> wide = {plain(1, 4, (int64_t(1) << 30)), plain(1, 4, (int64_t(1) << 30))};
        CHECK(refusal(pieces_validate(wide.data(), 2), "piece 1 (snp)", "int32"));
        wide[1].p = (int64_t(1) << 30) - 1;
        CHECK(pieces_validate(wide.data(), 2).empty());
    }

    // ---- first columns, the column map at every boundary ----------------------------------------------------------------------
    {
        const int64_t p_of[4] = {3, 7, 2, 5};
        int32_t first[kMaxPieces + 1];
        pieces_first_cols(p_of, 4, first);
        CHECK(first[0] == 0 && first[1] == 3 && first[2] == 10 && first[3] == 12 && first[4] == 17);
        for (int m = 5; m <= kMaxPieces; ++m) CHECK(first[m] == INT32_MAX);
        const int64_t at[] = {0, 2, 3, 9, 10, 11, 12, 16};
        const int piece[] = {0, 0, 1, 1, 2, 2, 3, 3};
        const int64_t local[] = {0, 2, 0, 6, 0, 1, 0, 4};
        for (int t = 0; t < 8; ++t) {
            int pc = -1;
            int64_t lc = -1;
            pieces_locate(first, at[t], pc, lc);
            CHECK(pc == piece[t] && lc == local[t]);
        }
        // the cap: eight pieces of one column each
        const int64_t ones[kMaxPieces] = {1, 1, 1, 1, 1, 1, 1, 1};
        int32_t f8[kMaxPieces + 1];
        pieces_first_cols(ones, kMaxPieces, f8);
        for (int m = 0; m <= kMaxPieces; ++m) CHECK(f8[m] == m);
        for (int j = 0; j < kMaxPieces; ++j) {
            int pc = -1;
            int64_t lc = -1;
            pieces_locate(f8, j, pc, lc);
            CHECK(pc == j && lc == 0);
        }

        // ---- range splits -------------------------------------------------------------------------------------------------
        PieceRange rg[kMaxPieces];
        int nr = pieces_split(first, 4, 0, 17, rg); // everything
        CHECK(nr == 4);
        for (int r = 0; r < nr; ++r) CHECK(rg[r].piece == r && rg[r].local0 == 0 && rg[r].count == p_of[r] && rg[r].out0 == first[r]);
        nr = pieces_split(first, 4, 2, 9, rg);      // starts inside piece 0, ends inside piece 2: columns 2 .. 10
        CHECK(nr == 3 && rg[0].piece == 0 && rg[0].local0 == 2 && rg[0].count == 1 && rg[0].out0 == 0);
        CHECK(rg[1].piece == 1 && rg[1].local0 == 0 && rg[1].count == 7 && rg[1].out0 == 1);
        CHECK(rg[2].piece == 2 && rg[2].local0 == 0 && rg[2].count == 1 && rg[2].out0 == 8);
        nr = pieces_split(first, 4, 4, 3, rg);      // inside one piece
        CHECK(nr == 1 && rg[0].piece == 1 && rg[0].local0 == 1 && rg[0].count == 3 && rg[0].out0 == 0);
        nr = pieces_split(first, 4, 10, 2, rg);     // exactly one piece, from boundary to boundary
        CHECK(nr == 1 && rg[0].piece == 2 && rg[0].local0 == 0 && rg[0].count == 2 && rg[0].out0 == 0);
        nr = pieces_split(first, 4, 16, 1, rg);     // the last column
        CHECK(nr == 1 && rg[0].piece == 3 && rg[0].local0 == 4 && rg[0].count == 1);
        CHECK(pieces_split(first, 4, 5, 0, rg) == 0);  // an empty range meets nothing
        CHECK(pieces_split(first, 4, 10, 0, rg) == 0); // ... on a boundary as well
        CHECK(pieces_split(first, 1, 3, 0, rg) == 0);
        // random ranges against the column map
        std::mt19937 gen(7);
        for (int t = 0; t < 2000; ++t) {
            const int64_t c0 = int64_t(gen() % 17), nc = int64_t(gen() % (17 - c0 + 1));
            nr = pieces_split(first, 4, c0, nc, rg);
            int64_t covered = 0;
            for (int r = 0; r < nr; ++r) {
                CHECK(rg[r].count > 0 && rg[r].out0 == covered);
                for (int64_t c = 0; c < rg[r].count; ++c) {
                    int pc;
                    int64_t lc;
                    pieces_locate(first, c0 + covered + c, pc, lc);
                    CHECK(pc == rg[r].piece && lc == rg[r].local0 + c);
                }
                covered += rg[r].count;
            }
            CHECK(covered == nc);
        }
    }

    // ---- 16-byte loads: every dense piece must pass a dense design's own test; a 2-bit piece always passes ------------------------
    {
        const int kind[4] = {kPieceDense, kPieceSnp, kPieceDense, kPieceSnp};
        uintptr_t base[4] = {0x1000, 0x2003, 0x3010, 0x4001}; // (the 2-bit pieces' bases and leading dimensions do not matter)
        int64_t ld[4] = {204, 51, 204, 77};
        CHECK(pieces_vec_ok(kind, base, ld, 4, 2) && pieces_vec_ok(kind, base, ld, 4, 4));
        base[2] = 0x3008;                                     // a dense piece off a 16-byte boundary: a slice from an odd column
        CHECK(!pieces_vec_ok(kind, base, ld, 4, 2) && !pieces_vec_ok(kind, base, ld, 4, 4));
        CHECK(pieces_vec_ok(kind, base, ld, 2, 2));           // (the first two pieces alone are fine)
        base[2] = 0x3010, ld[0] = 203;                        // a leading dimension that is no whole vector
        CHECK(!pieces_vec_ok(kind, base, ld, 4, 2));
        ld[0] = 206;                                          // whole f64 vectors, but not whole f32 vectors
        CHECK(pieces_vec_ok(kind, base, ld, 4, 2) && !pieces_vec_ok(kind, base, ld, 4, 4));
        const int snp_only[2] = {kPieceSnp, kPieceSnp};
        const uintptr_t b2[2] = {1, 3};
        const int64_t l2[2] = {5, 7};
        CHECK(pieces_vec_ok(snp_only, b2, l2, 2, 2) && pieces_vec_ok(snp_only, b2, l2, 2, 4));
    }

    if (fails) return 1;
    std::printf("pieces_host: ok\n");
    return 0;
}
