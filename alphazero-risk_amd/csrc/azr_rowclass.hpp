// azr_rowclass.hpp — border-class row order of the board cells of a workgroup tile and the row tables built from it (shared by
// the multi-board inference towers, azr_tower_sb / _sc / _fx.hip, and the training conv kernel t_conv_rs, azr_train_conv.hpp).
//
// A 3x3 SAME conv on the 6x7 board is an implicit GEMM whose M rows are board cells; a tap (dy, dx) has no in-board source
// for the cells of one board edge.  If the rows of a workgroup's tile are ordered so that whole 16-row MFMA tiles lie on one
// edge, the (tile, tap) pairs without any source are skipped altogether — exact zeros left out, results unchanged.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace azr {

// Row order = border classes, corners counted with the COLUMN classes: a cell with x = 0 has no in-board source under the
// three taps with dx = -1 whatever its y, so all 7 x = 0 cells of a board (corners included) share tiles, likewise x = 5;
// the y = 0 / y = 6 classes are the 4 non-corner cells.  Pad rows (no cell: zero under every tap) top up class tiles.
//   NB = 4 (176 rows):  tile 0 = 16 cells x=0 | 1 = 16 cells x=5 | 2 = the other 12 x=0 + 4 pads | 3 = the other 12 x=5 + 4 pads
//                       | 4 = 16 cells y=0 | 5 = 16 cells y=6 | 6..10 = the 80 interior cells          => 18 of 99 tile-taps skipped
//   NB = 3 (128 rows):  the corners go where they complete a tile: tile 0 = 16 of the 18 cells y=0 (all but board 0's corners)
//                       | 1 = 16 of the 18 cells y=6 | 2 = the 15 cells x=0, y=1..5 + board 0's (0,0) | 3 = same for x=5 with (5,0)
//                       | 4..7 = board 0's (0,6) and (5,6), the 60 interior cells, 2 pads              => 12 of 72
//   NB = 2 (96 rows):   tile 0 = 14 cells x=0 + 2 pads | 1 = 14 cells x=5 + 2 pads | 2 = 8 cells y=0 + 8 pads
//                       | 3 = 8 cells y=6 + 8 interior | 4, 5 = interior                               =>  9 of 54
template <int NB>
__host__ __device__ __forceinline__ constexpr int row_of(int b, int pos)
{
    const int y = pos / 6, x = pos - y * 6;
    if (NB == 4) {
        if (x == 0) { const int q = b * 7 + y; return q < 16 ? q : 32 + (q - 16); }
        if (x == 5) { const int q = b * 7 + y; return q < 16 ? 16 + q : 48 + (q - 16); }
        if (y == 0) return 64 + b * 4 + (x - 1);
        if (y == 6) return 80 + b * 4 + (x - 1);
        return 96 + b * 20 + (y - 1) * 4 + (x - 1);
    } else if (NB == 3) {
        const bool corner0 = b == 0 && (x == 0 || x == 5);          // board 0's corners complete the column tiles
        if (y == 0) return corner0 ? (x == 0 ? 47 : 63) : (b == 0 ? x - 1 : 4 + (b - 1) * 6 + x);
        if (y == 6) return corner0 ? (x == 0 ? 64 : 65) : 16 + (b == 0 ? x - 1 : 4 + (b - 1) * 6 + x);
        if (x == 0) return 32 + b * 5 + (y - 1);
        if (x == 5) return 48 + b * 5 + (y - 1);
        return 66 + b * 20 + (y - 1) * 4 + (x - 1);
    } else {
        if (x == 0) return b * 7 + y;
        if (x == 5) return 16 + b * 7 + y;
        if (y == 0) return 32 + b * 4 + (x - 1);
        if (y == 6) return 48 + b * 4 + (x - 1);
        return 56 + b * 20 + (y - 1) * 4 + (x - 1);
    }
}
// bit mt set = tile mt has no in-board source cell under this tap (tap 9 = "no tap": everything skipped)
template <int NB>
__host__ __device__ constexpr uint32_t skip_mask(int tap)
{
    if (tap > 8) return 0xffffffffu;
    const int ty = tap / 3, tx = tap - 3 * ty;
    if (NB == 4) return (tx == 0 ? 0x5u : tx == 2 ? 0xAu : 0u) | (ty == 0 ? 0x10u : ty == 2 ? 0x20u : 0u);
    if (NB == 3) return (ty == 0 ? 0x1u : ty == 2 ? 0x2u : 0u) | (tx == 0 ? 0x4u : tx == 2 ? 0x8u : 0u);
    return (tx == 0 ? 0x1u : tx == 2 ? 0x2u : 0u) | (ty == 0 ? 0x4u : 0u);
}
// first pad lane (fragment column) of tile mt; 16 = the tile has no pad rows
template <int NB>
__host__ __device__ constexpr int pad_from(int mt)
{
    if (NB == 4) return (mt == 2 || mt == 3) ? 12 : 16;
    if (NB == 3) return mt == 7 ? 14 : 16;
    return mt < 2 ? 14 : mt == 2 ? 8 : 16;
}

// ---- the row tables a kernel builds in LDS once per launch: rowof[board * 42 + pos] = row_of, rowcell[row] = cell_code of the
// row's cell (PAD_CELL for a pad row), taprow[tap][row] = the row a 3x3 tap reads for that row (the zero row ZR where there is none).
// The two rules, per element (host side: tests/helpers/rowclass_probe.hip):
constexpr int PAD_CELL = 0xffff;
__host__ __device__ __forceinline__ constexpr int cell_code(int b, int pos) { return (pos / 6) | ((pos % 6) << 4) | (b << 8); }   // y | x << 4 | board << 8
// the row a row with cell code `ci` reads under tap t: the row of the neighbouring cell of the same board, or the zero row `zr` for a
// pad row, a tap that leaves the board and tap 9 ("no tap", the second half of the stem's last k-step; TAPS = 9: t is a tap)
template <int TAPS, class Row>
__host__ __device__ __forceinline__ constexpr int tap_source_row(int t, int ci, int zr, const Row* rowof)
{
    int src = zr;
    if ((TAPS <= 9 || t < 9) && ci != PAD_CELL) {
        const int y = (ci & 15) + t / 3 - 1, x = ((ci >> 4) & 15) + t % 3 - 1;
        if ((unsigned)y < 7u && (unsigned)x < 6u) src = rowof[(ci >> 8) * 42 + y * 6 + x];
    }
    return src;
}

// The builder (k_tower_sb, k_tower_sc; k_tower_fx and t_conv_rs apply the two rules in loops of their own, profiles/tower_common_isa.txt):
// TAPS = 10 for a tower (tap 9 = all zero row), 9 for a plain 3x3 conv.  Two barriers: the pad marks are visible | the cell codes and
// rowof are visible; taprow is visible behind the CALLER's next barrier.
template <int NB, int THREADS, int TAPS>
__device__ __forceinline__ void build_row_tables(uint8_t* rowof, uint8_t* taprow, uint16_t* rowcell)
{
    const int tid = threadIdx.x;
    constexpr int ROWS = 42 * NB, ZR = (ROWS + 15) / 16 * 16;
    for (int i = tid; i < ZR; i += THREADS) rowcell[i] = 0xffffu;
    __syncthreads();
    for (int i = tid; i < ROWS; i += THREADS) {
        const int b = i / 42, pos = i - b * 42, r = row_of<NB>(b, pos);
        rowof[i] = (uint8_t)r;
        rowcell[r] = (uint16_t)cell_code(b, pos);
    }
    __syncthreads();
    for (int i = tid; i < TAPS * ZR; i += THREADS) {
        const int t = i / ZR, r = i - t * ZR;
        taprow[i] = (uint8_t)tap_source_row<TAPS>(t, rowcell[r], ZR, rowof);
    }
}

}  // namespace azr
