// host_harness_diag_lower.cpp -- PlanOptions::diag_lower (csrc/plan_lists.h) as a host program for
// tests/test_diag_update_lower_host.py: the option is read by the launches alone, so the structure, every task list, the dataflow
// units with their waits and the factorisation's launch sequence of one plan are byte for byte the same with it on and off.
// No GPU, no HIP: the lists are built on the stand-in bases.
//   argv: nt factor_flow        stdin: one "I J" pair (I > J) per off-diagonal tile of the lower-triangular structure
//   stdout: "ok" units  updates  diagonal-target updates in the level lists  ... in the dataflow launches  schedule ops
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <string>
#include <vector>

#include "plan_lists.h"

namespace {
template <typename T>
bool same_bytes(const std::vector<T>& a, const std::vector<T>& b) {
    return a.size() == b.size() && (a.empty() || memcmp(a.data(), b.data(), a.size() * sizeof(T)) == 0);
}
struct Built { apex::PlanStructure s; apex::PlanLists l; std::vector<apex::SchedOp> ops; };
}  // namespace

int main(int argc, char** argv) {
    if (argc != 3) { fprintf(stderr, "usage: %s nt factor_flow < tiles\n", argv[0]); return 2; }
    const int nt = atoi(argv[1]), flow = atoi(argv[2]);
    if (nt <= 0 || nt > 1024) { fprintf(stderr, "bad arguments\n"); return 2; }
    std::vector<uint8_t> present((size_t)nt * nt, 0);
    for (int I = 0; I < nt; ++I) present[(size_t)I * nt + I] = 1;
    int a, b;
    while (scanf("%d %d", &a, &b) == 2) {
        if (b < 0 || a <= b || a >= nt) { fprintf(stderr, "tile out of range\n"); return 2; }
        present[(size_t)a * nt + b] = 1;
    }
    Built built[2];
    for (int on = 0; on < 2; ++on) {
        apex::PlanOptions o;
        o.flow_cols = flow;
        o.diag_lower = on;
        Built& x = built[on];
        x.s = apex::plan_structure(nt, present, o);
        if (x.s.refused) { printf("refused: %s\n", x.s.message.c_str()); return 1; }
        const std::string e = apex::build_plan_lists(x.s, present, o, reinterpret_cast<double*>(apex::kStandInTiles),
                                                     reinterpret_cast<double*>(apex::kStandInLinv), &x.l);
        if (!e.empty()) { printf("lists: %s\n", e.c_str()); return 1; }
        x.ops = apex::factor_schedule(apex::schedule_input(x.s, x.l, apex::ScheduleSwitches()), 0, x.s.n_levels());
    }
    const apex::PlanLists &l0 = built[0].l, &l1 = built[1].l;
    static_assert(sizeof(apex::FactorUnit) == 3 * sizeof(void*) + 10 * sizeof(int), "FactorUnit has no padding: its bytes can be compared");
    static_assert(sizeof(apex::GemmTask) == 3 * sizeof(void*) && sizeof(apex::PotrfTask) == 2 * sizeof(void*) + 8, "no padding but PotrfTask's tail");
    if (!same_bytes(l0.units, l1.units)) { printf("the dataflow units differ\n"); return 1; }
    for (size_t i = 0; i < l0.units.size(); ++i)
        if (memcmp(l0.units[i].wait_val, l1.units[i].wait_val, sizeof l0.units[i].wait_val) != 0 || l0.units[i].pub != l1.units[i].pub) { printf("unit %zu waits differ\n", i); return 1; }
    if (!same_bytes(l0.upd, l1.upd) || !same_bytes(l0.panel, l1.panel) || !same_bytes(l0.upd_rounds, l1.upd_rounds)) { printf("the level lists differ\n"); return 1; }
    if (l0.potrf.size() != l1.potrf.size()) { printf("the potrf lists differ\n"); return 1; }
    for (size_t i = 0; i < l0.potrf.size(); ++i)
        if (l0.potrf[i].A != l1.potrf[i].A || l0.potrf[i].Linv != l1.potrf[i].Linv || l0.potrf[i].K != l1.potrf[i].K) { printf("potrf %zu differs\n", i); return 1; }
    if (built[0].s.slot != built[1].s.slot || built[0].s.group_of != built[1].s.group_of) { printf("the structures differ\n"); return 1; }
    if (built[0].ops.size() != built[1].ops.size()) { printf("the schedules differ in length\n"); return 1; }
    for (size_t i = 0; i < built[0].ops.size(); ++i) {
        const apex::SchedOp &x = built[0].ops[i], &y = built[1].ops[i];
        if (x.op != y.op || x.stream != y.stream || x.event != y.event || x.list != y.list || x.first != y.first || x.count != y.count || x.arrive != y.arrive) {
            printf("schedule op %zu differs\n", i);
            return 1;
        }
    }
    if (l0.n_diag_upd[0] != l1.n_diag_upd[0] || l0.n_diag_upd[1] != l1.n_diag_upd[1]) { printf("the counts differ\n"); return 1; }
    printf("ok %zu %zu %lld %lld %zu\n", l1.units.size(), l1.upd.size(), (long long)l1.n_diag_upd[0], (long long)l1.n_diag_upd[1], built[1].ops.size());
    return 0;
}
