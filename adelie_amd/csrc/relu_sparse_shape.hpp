// relu_sparse_shape.hpp — how the builder and the structured sweep of a convex-relu design over a sparse base matrix
// (kernels_relu_sparse.hip) cut their grids: one wavefront per (column of Z, row tile, word of kReluSpWordBits gates).  Free of
// device code: the launcher and a stand-alone host program of the tests include it.
#pragma once
#include <cstdint>

namespace ahip {

constexpr int kReluSpWordBits = 32;        // gates per packed mask word (one gather of a word serves 32 gates)
constexpr int64_t kReluSpTileUnit = 4096;  // a row tile is a multiple of this many rows
constexpr int64_t kReluSpMaxTiles = 16;    // at most this many row tiles, whatever n

struct ReluSparseShape {
    int64_t tile_rows = 0; // tile t owns the rows [t * tile_rows, min(n, (t + 1) * tile_rows))
    int64_t tiles = 0;     // row tiles (partial sums per column of the sweep), 1 .. kReluSpMaxTiles
    int64_t words = 0;     // mask words per row
};

// Row tiles: a long column of Z is shared by several wavefronts, at most kReluSpMaxTiles of them so that the sweep's partial
// sums stay at kReluSpMaxTiles m d values; a tile grows in steps of kReluSpTileUnit rows once n passes 16 units.
inline ReluSparseShape relu_sparse_shape(int64_t n, int64_t m) {
    ReluSparseShape sh;
    const int64_t span = kReluSpTileUnit * kReluSpMaxTiles;
    int64_t mult = (n + span - 1) / span;
    if (mult < 1) mult = 1;
    sh.tile_rows = kReluSpTileUnit * mult;
    sh.tiles = (n + sh.tile_rows - 1) / sh.tile_rows;
    if (sh.tiles < 1) sh.tiles = 1;
    sh.words = (m + kReluSpWordBits - 1) / kReluSpWordBits;
    return sh;
}

// elements of the caller's work buffer: the tiles' partial sums of the m * d columns of the unsigned half
inline int64_t relu_sparse_sweep_work_elems(int64_t n, int64_t d, int64_t m) {
    return relu_sparse_shape(n, m).tiles * d * m + 16;
}

} // namespace ahip
