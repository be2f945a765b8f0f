// host_harness_tile_order.cpp -- tile_order (csrc/plan_lists.h) as a host program for tests/test_pg_asm_ref_host.py: the
// permutation PoseGraphSolver::set_structure applies to whole tiles of vertices.  No GPU, no HIP.
//   argv: nt nested_dissection leaf        stdin: one "a b" pair of adjacent tiles per line
//   stdout: "ok" and perm[0 .. nt), the internal position of every caller tile
#include <stdio.h>
#include <stdlib.h>

#include <vector>

#include "plan_lists.h"

int main(int argc, char** argv) {
    if (argc != 4) { fprintf(stderr, "usage: %s nt nested_dissection leaf < pairs\n", argv[0]); return 2; }
    const int nt = atoi(argv[1]), nd = atoi(argv[2]), leaf = atoi(argv[3]);
    if (nt <= 0 || nt > 4096 || leaf <= 0) { fprintf(stderr, "bad arguments\n"); return 2; }
    std::vector<uint8_t> adj((size_t)nt * nt, 0);
    int a, b;
    while (scanf("%d %d", &a, &b) == 2) {
        if (a < 0 || b < 0 || a >= nt || b >= nt) { fprintf(stderr, "pair out of range\n"); return 2; }
        if (a != b) { adj[(size_t)a * nt + b] = 1; adj[(size_t)b * nt + a] = 1; }
    }
    const std::vector<int> perm = apex::tile_order(nt, adj, nd != 0, leaf);
    std::vector<char> hit(nt, 0);
    for (int p : perm) {
        if (p < 0 || p >= nt || hit[p]) { printf("not a permutation\n"); return 1; }
        hit[p] = 1;
    }
    printf("ok");
    for (int p : perm) printf(" %d", p);
    printf("\n");
    return 0;
}
