// prints the border-class row tables of csrc/azr_rowclass.hpp (host side of the same constexpr functions the kernels use):
//   NB MT | row_of[NB*42] | skip_mask[9] | pad_from[MT]
// and, called with the argument `taprow`, one more part per line:  | taprow[10][ZR]
// taprow = the source-row table the kernels build in LDS (build_row_tables), computed here by the same per-element rules:
// rowcell[row] = cell_code of the row's cell or PAD_CELL, taprow[tap][row] = tap_source_row
#include <hip/hip_runtime.h>
#include <stdio.h>
#include <string.h>

#include "azr_rowclass.hpp"

template <int NB>
static void dump(bool with_taprow)
{
    const int MT = (42 * NB + 15) / 16, ZR = MT * 16;
    printf("%d %d |", NB, MT);
    for (int b = 0; b < NB; b++)
        for (int pos = 0; pos < 42; pos++) printf(" %d", azr::row_of<NB>(b, pos));
    printf(" |");
    for (int t = 0; t < 9; t++) printf(" %u", azr::skip_mask<NB>(t));
    printf(" |");
    for (int mt = 0; mt < MT; mt++) printf(" %d", azr::pad_from<NB>(mt));
    if (!with_taprow) { printf("\n"); return; }
    printf(" |");
    int rowof[42 * NB], rowcell[ZR];
    for (int r = 0; r < ZR; r++) rowcell[r] = azr::PAD_CELL;
    for (int i = 0; i < 42 * NB; i++) {
        rowof[i] = azr::row_of<NB>(i / 42, i % 42);
        rowcell[rowof[i]] = azr::cell_code(i / 42, i % 42);
    }
    for (int t = 0; t < 10; t++)
        for (int r = 0; r < ZR; r++) printf(" %d", azr::tap_source_row<10>(t, rowcell[r], ZR, rowof));
    printf("\n");
}

int main(int argc, char** argv)
{
    const bool with_taprow = argc > 1 && !strcmp(argv[1], "taprow");
    dump<2>(with_taprow);
    dump<3>(with_taprow);
    dump<4>(with_taprow);
    return 0;
}
