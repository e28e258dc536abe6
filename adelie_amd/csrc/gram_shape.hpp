// gram_shape.hpp — how the MFMA block builds cut their grids: K-splits, tile classes and the size of the partial buffers.  Free of
// device code: the launchers (kernels_gram.hip, kernels_strip.hip), the kernel-level test entry (solver.hip) and a stand-alone
// host program of the tests (tests/native/gram_shape_main.cpp) include it.
#pragma once
#include <cstdint>

namespace ahip {

constexpr int kGramBM = 128;  // rows of a Gram tile
constexpr int kGramKT = 32;   // rows of the design per stage of the staged kernels
// Workgroups a SMALL build (one diagonal block / one cross block / a batch of diagonal blocks) is spread over.  512 = one
// full round of two resident workgroups per CU, the fastest for the build itself.  (Confining side-stream builds to fewer
// workgroups was measured slower: 56 -> 2.69, 112 -> 2.99 vs 3.17 paths/s unconfined; the chain waits for the slower builds.)
constexpr int kSmallGramWgs = 512;
constexpr int kStripChunk = 16;  // rows of the design per chunk of a strip wavefront
constexpr int kStripW = 256;     // columns of a strip (previous block | own block)
// K-splits of a strip launch (per entry).  Each split writes a partial strip of 16 MT x 256 values that the reduce kernel reads
// back (512 splits: 53 MB written per launch of the headline's screen strips, PMC), and in the path the strips only get the
// ~60 CUs the fused launches leave, so more splits than that buy nothing: 192 instead of 512 is worth 1.5 ms per headline path
// and 4.7 ms on config 3 (the chain starts to wait for the strips below ~112).  set_strip_workgroups changes it for one host
// thread (the strip micro-benchmark does), up to kStripWgsMax, which the work buffer is sized for.
constexpr int kStripWgsDefault = 192;
constexpr int kStripWgsMax = 1024;

// tile class of a diagonal block (or of the widest block of a batch): the SB of syrk_kernel / syrk_batch_kernel
inline int syrk_tile_class(int64_t M) { return M <= 32 ? 32 : (M <= 64 ? 64 : 128); }

inline void syrk_shape(int64_t n, int& nsplit, int64_t& kchunk) {
    int64_t want = 512; // one full round of 2 resident blocks per CU
    const int64_t max_split = (n + kGramKT * 8 - 1) / (kGramKT * 8);
    if (want > max_split) want = max_split;
    if (want < 1) want = 1;
    kchunk = (n + want - 1) / want;
    kchunk = ((kchunk + 255) / 256) * 256; // whole super-stages of the SNP body (a multiple of KT as well)
    const int64_t ns = (n + kchunk - 1) / kchunk;
    nsplit = int(ns < 1 ? 1 : ns);
}

inline void syrk_batch_shape(int64_t n, int count, int& nsplit, int64_t& kchunk) {
    // about one full round of 2 resident workgroups per CU over all the blocks of the batch (count = 1: the single-block shape)
    int64_t want = (int64_t(kSmallGramWgs) + count - 1) / count;
    const int64_t max_split = (n + kGramKT * 8 - 1) / (kGramKT * 8);
    if (want > max_split) want = max_split;
    if (want < 1) want = 1;
    kchunk = (n + want - 1) / want;
    kchunk = ((kchunk + 255) / 256) * 256; // whole super-stages of the SNP body (a multiple of KT as well)
    const int64_t ns = (n + kchunk - 1) / kchunk;
    nsplit = int(ns < 1 ? 1 : ns);
}

// N tiling: full 128-wide tiles, then the remainder as one 64-wide tile when it fits (less padding than a 128 tile)
struct GramShape {
    int64_t Mt, n128, n64, Npad, kchunk;
    int nsplit;
};
inline GramShape gram_shape(int64_t n, int64_t M, int64_t N) {
    GramShape g;
    g.Mt = (M + kGramBM - 1) / kGramBM;
    g.n128 = N / 128;
    const int64_t rem = N - g.n128 * 128;
    g.n64 = 0;
    if (rem > 64) ++g.n128;
    else if (rem > 0) g.n64 = 1;
    g.Npad = g.n128 * 128 + g.n64 * 64;
    const int64_t tiles = g.Mt * (g.n128 + g.n64);
    // Many tiles: ~3072 blocks so that the last partial round over the 256 CUs x 2 resident blocks costs little.  A single
    // diagonal block of the panel engine: one full round (512 blocks) - more K-splits only add partial-tile traffic
    // (128 KB written and re-read per split; measured -18 % at n = 500k).
    const int64_t target = tiles <= 4 ? int64_t(kSmallGramWgs) : 3072;
    int64_t want = (target + tiles - 1) / tiles;
    const int64_t max_split = (n + kGramKT * 8 - 1) / (kGramKT * 8);
    if (want > max_split) want = max_split;
    const int64_t cap = (int64_t(1) << 28) / (g.Mt * kGramBM * g.Npad); // partial buffer <= 2^28 elements
    if (want > cap) want = cap;
    if (want < 1) want = 1;
    g.kchunk = (n + want - 1) / want;
    g.kchunk = ((g.kchunk + kGramKT - 1) / kGramKT) * kGramKT;
    int64_t ns = (n + g.kchunk - 1) / g.kchunk;
    g.nsplit = int(ns < 1 ? 1 : ns);
    return g;
}

inline void strip_shape(int64_t n, int count, int wgs, int& nsplit, int64_t& kchunk) {
    int64_t want = (int64_t(wgs) + count - 1) / count;
    const int64_t max_split = (n + 8 * kStripChunk - 1) / (8 * kStripChunk);
    if (want > max_split) want = max_split;
    if (want < 1) want = 1;
    kchunk = (n + want - 1) / want;
    kchunk = ((kchunk + 2 * kStripChunk - 1) / (2 * kStripChunk)) * (2 * kStripChunk); // whole pairs of chunks: 16-byte aligned row offsets
    const int64_t ns = (n + kchunk - 1) / kchunk;
    nsplit = int(ns < 1 ? 1 : ns);
}
// 16-row tiles the strip kernel is instantiated for (0: more rows than it takes)
inline int strip_row_tiles(int m) { return m <= 16 ? 1 : (m <= 32 ? 2 : (m <= 48 ? 3 : (m <= 64 ? 4 : 0))); }

// ---- elements of the partial buffer (`work`) a launch needs -----------------------------------------------------------------
inline int64_t syrk_work_elems(int64_t n, int64_t M) {
    int nsplit;
    int64_t kchunk;
    syrk_shape(n, nsplit, kchunk);
    const int64_t SB = syrk_tile_class(M);
    return int64_t(nsplit) * SB * SB;
}
inline int64_t syrk_batch_work_elems(int64_t n, int count) {
    int nsplit;
    int64_t kchunk;
    syrk_batch_shape(n, count, nsplit, kchunk);
    return int64_t(nsplit) * count * 128 * 128;
}
inline int64_t gram_work_elems(int64_t n, int64_t M, int64_t N) {
    if (M <= 0 || N <= 0) return 0;
    const GramShape g = gram_shape(n, M, N);
    return int64_t(g.nsplit) * g.Mt * kGramBM * g.Npad;
}
inline int64_t gram_batch_work_elems(int64_t n, int count) {
    int ns;
    int64_t kc;
    syrk_batch_shape(n, count, ns, kc);
    return int64_t(count) * ns * kGramBM * 128;
}
inline int64_t strip_work_elems(int64_t n, int count, int m_max) {
    int ns;
    int64_t kc;
    strip_shape(n, count, kStripWgsMax, ns, kc); // (sized for the widest spread set_strip_workgroups allows)
    const int mt = strip_row_tiles(m_max);
    return int64_t(count) * ns * 16 * (mt ? mt : 4) * kStripW;
}

// What the last block build launched by this host thread ran (kernels.hpp: last_build_launch): every launcher of
// kernels_gram.hip / kernels_strip.hip / the csc builds records it; the kernel-level test entry reports it.
struct BuildLaunchInfo {
    enum : int { NONE = 0, SYRK = 1, SYRK_BATCH = 2, GRAM = 3, GRAM_BATCH = 4, STRIP = 5, BLOCK_GRAM_CSC = 6, GRAM_CSC = 7 };
    int kind = NONE;
    int nsplit = 0;
    int64_t kchunk = 0;
    int tile = 0;        // SB (syrk), MT (strip), 128 (gram_batch)
    int n128 = 0, n64 = 0; // general Gram: N tiles of either width
    int vec16 = 0;       // the 16-byte-load variant ran (VECOK; a 2-bit design always)
    int strip_lt = 0;    // strip_lt_kernel ran
    int symmetric = 0;   // general Gram: the symmetric route
};

} // namespace ahip
