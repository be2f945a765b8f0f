// sinv_lists.h -- the task lists of the selected inversion (block Takahashi recurrence) as a value: built on the host from a
// slot map and the level groups of the factorisation, with tiles named by array and index.  SelectedInverse (tile_sinv.h)
// resolves the names to addresses and issues the lists.  Host only: nothing of the device API here or in anything this file
// includes.
//
// Z = (L L^T)^-1 on the tile pattern of L, root group first; with j's off-diagonal rows I_j and Y_r = L_rj Linv_j:
//     Z_rj = - sum_{s in I_j} Z~_rs Y_s    (r in I_j; Z~_rs = Z_rs for r >= s, else Z_sr^T)
//     Z_jj = Linv_j^T Linv_j - sum_{r in I_j} Y_r^T Z_rj
// The columns of a group are independent: I_j holds ancestors of j only, and those sit in higher groups, whose Z is complete
// when the group runs.
#pragma once
#include <stdint.h>

#include <array>
#include <string>
#include <vector>

#include "tile_tasks.h"

namespace apex {

enum SinvArray : uint8_t { kSinvL, kSinvLinv, kSinvZ, kSinvY };   // SinvRef::array
struct SinvRef {   // one tile: of L or Z by slot, of Linv by tile column, of Y by index inside the group's Y block
    uint8_t array;
    int64_t tile;
};
struct SinvProdH { SinvRef A, B; int op; };           // SinvProd (tile_tasks.h) by name; op: the kSinv* bits
struct SinvTaskH { SinvRef C; int first, count; };    // SinvTask by name

struct SinvLists {
    std::vector<SinvTaskH> tasks;
    std::vector<SinvProdH> prods;
    // per level group, root group first: the tasks [g[k], g[k + 1]) of its Y (k = 0), off-diagonal Z (1), diagonal Z (2) launch
    std::vector<std::array<int, 4>> groups;
    int64_t n[3] = {0, 0, 0};   // tile products per kind: Y, off-diagonal Z, diagonal Z
    int64_t y_max = 0;          // Y tiles of the largest group
};

// slot[I * nt + J] (I >= J): the tile's slot, -1 where absent.  group_cols: the level groups' columns in the execution order of
// the factorisation (leaves first).  Inside a group all Y, then all off-diagonal Z, then all diagonal Z; columns in the
// group's order, rows ascending; in a diagonal task the Linv^T Linv term first.  The device sums in list order, so this order
// decides the bits.  Returns "" or why the pattern is refused: Z~_rs for r, s in I_j must be a tile of L -- tile-level symbolic
// fill makes every I_j a clique; checked, not assumed.
std::string build_sinv_lists(int nt, const int* slot, const std::vector<std::vector<int>>& group_cols, SinvLists* out);

}  // namespace apex
