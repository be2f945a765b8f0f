// plan_lists_check.cpp -- the host-only planning code as a plain program, for a host sanitizer: plan_structure, build_plan_lists
// on the stand-in bases, build_sinv_lists, factor_schedule + check_schedule of both phases, for a few structures.  Includes the
// host-only headers alone (no HIP header on the include path); exits non-zero on any violation or error string.
//   c++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all -pthread -I apex-solver_amd/csrc \
//       tools/plan_lists_check.cpp apex-solver_amd/csrc/{plan_lists,factor_schedule,sinv_lists}.cpp
#include <stdio.h>

#include <algorithm>

#include <string>
#include <vector>

#include "factor_schedule.h"
#include "plan_lists.h"
#include "sinv_lists.h"

using namespace apex;

static std::vector<uint8_t> lower(int nt, const std::vector<std::pair<int, int>>& entries) {
    std::vector<uint8_t> p((size_t)nt * nt, 0);
    for (int i = 0; i < nt; ++i) p[(size_t)i * nt + i] = 1;
    for (const auto& e : entries) p[(size_t)std::max(e.first, e.second) * nt + std::min(e.first, e.second)] = 1;
    return p;
}

static int n_bad = 0;
static void fail(const char* name, const std::string& what) { printf("FAIL %s: %s\n", name, what.c_str()); ++n_bad; }

// want_refused: 0 the plan must build and prove race free; else the structure must come back refused that way
static void run(const char* name, int nt, const std::vector<uint8_t>& present, const PlanOptions& o, int want_refused = 0) {
    const PlanStructure s = plan_structure(nt, present, o);
    if (s.refused != want_refused) return fail(name, "refused = " + std::to_string(s.refused) + " (" + s.message + ")");
    PlanLists l;
    const std::string e = build_plan_lists(s, present, o, reinterpret_cast<double*>(kStandInTiles), reinterpret_cast<double*>(kStandInLinv), &l);
    if (want_refused) {
        if (e.empty() || !l.potrf.empty()) fail(name, "lists were built from a refused structure");
        else printf("ok   %s: refused (%s)\n", name, e.c_str());
        return;
    }
    if (!e.empty()) return fail(name, e);
    const ScheduleInput in = schedule_input(s, l, ScheduleSwitches());
    size_t n_ops = 0;
    for (int ph = 0; ph < 2; ++ph) {
        const std::vector<SchedOp> ops = ph == 0 ? factor_schedule(in, 0, s.n_local_groups) : factor_schedule(in, s.n_local_groups, s.n_levels());
        std::string why;
        if (check_schedule(ops, l.potrf, l.panel, l.upd, l.units, &why) != 0) return fail(name, "phase " + std::to_string(ph) + ": " + why);
        n_ops += ops.size();
    }
    SinvLists sl;
    const std::string se = build_sinv_lists(nt, s.slot.data(), s.group_cols, &sl);
    if (!se.empty()) return fail(name, se);
    printf("ok   %s: %d groups (%d local), %lld slots, %zu updates in %zu rounds, %zu units, %zu calls, %zu inversion tasks\n", name, s.n_levels(),
           s.n_local_groups, (long long)s.n_slots, l.upd.size(), l.upd_rounds.size(), l.units.size(), n_ops, sl.tasks.size());
}

int main() {
    std::vector<std::pair<int, int>> e;
    for (int i = 0; i < 12; ++i) for (int j = 0; j < i; ++j) e.push_back({i, j});
    run("dense12", 12, lower(12, e), PlanOptions());

    e.clear();   // a chain 0-1-...-7 with a leaf hanging off every second link
    for (int i = 1; i < 8; ++i) e.push_back({i, i - 1});
    for (int k = 0; k < 4; ++k) e.push_back({8 + k, 2 * k + 1});
    run("chain+leaves", 12, lower(12, e), PlanOptions());

    e.clear();
    for (int i = 0; i < 48; ++i) for (int j = std::max(0, i - 3); j < i; ++j) e.push_back({i, j});
    const std::vector<uint8_t> band = lower(48, e);
    for (int world : {1, 2, 4})
        for (int rank = 0; rank < world; ++rank) {
            PlanOptions o;
            o.rank = rank; o.world = world;
            run(("band48/world" + std::to_string(world) + "/rank" + std::to_string(rank)).c_str(), 48, band, o);
        }
    // the same band with its middle separator ordered last: two subtrees under a shared top, which two ranks do cut
    e.clear();
    auto place = [](int i) { return i < 22 ? i : (i < 25 ? 45 + (i - 22) : i - 3); };
    for (int i = 0; i < 48; ++i) for (int j = std::max(0, i - 3); j < i; ++j) e.push_back({place(i), place(j)});
    const std::vector<uint8_t> cut = lower(48, e);
    for (int rank = 0; rank < 2; ++rank) {
        PlanOptions o;
        o.rank = rank; o.world = 2;
        run(("band48 dissected/world2/rank" + std::to_string(rank)).c_str(), 48, cut, o);
    }
    PlanOptions own;
    own.world = 2; own.own_all = true; own.flow_cols = 3; own.flow_rows = 64; own.two_side = 2;
    run("band48 dissected/own_all, flow 3", 48, cut, own);

    PlanOptions small;
    small.max_updates = 10;
    run("dense12, max_updates 10", 12, lower(12, [] { std::vector<std::pair<int, int>> d; for (int i = 0; i < 12; ++i) for (int j = 0; j < i; ++j) d.push_back({i, j}); return d; }()), small, 1);

    const std::vector<int> perm = tile_order(48, [&] { std::vector<uint8_t> a(band); for (int i = 0; i < 48; ++i) for (int j = 0; j < i; ++j) a[(size_t)j * 48 + i] = a[(size_t)i * 48 + j]; return a; }(), true, 8);
    std::vector<char> hit(48, 0);
    for (int v : perm) if (v >= 0 && v < 48) hit[v] = 1;
    for (char h : hit) if (!h) { fail("tile_order", "not a permutation"); break; }
    if (plan_owners(48, cut, 2).size() != 48 || !plan_owners(48, band, 2).empty()) fail("plan_owners", "the dissected band is cut, the chain is not");

    printf("%s\n", n_bad ? "FAILED" : "all clean");
    return n_bad ? 1 : 0;
}
