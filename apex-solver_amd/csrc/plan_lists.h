// plan_lists.h -- everything a tile plan derives from its 0/1 tile structure before it touches a device, as two values:
// PlanStructure (symbolic fill, partition of the elimination tree, slot map, level groups, the refusals that are host
// arithmetic) and PlanLists (the task lists of the factorisation, of both forms of both triangular sweeps and of the PCG, the
// dataflow units in list-schedule order, the first-writer flags).  TilePlan (tile_plan.h) allocates the tiles, has the lists
// built on their addresses and uploads them; factor_schedule() and build_sinv_lists() read the same two values.  Host only: no
// HIP type here or in anything this file includes.
#pragma once
#include <stdint.h>

#include <string>
#include <utility>
#include <vector>

#include "factor_schedule.h"
#include "tile_tasks.h"

namespace apex {

// The task records name tiles by address (the kernels read them as they are; check_schedule identifies tiles by address).
// Callers without a device build the lists on these stand-in bases: addresses that identify tiles, nothing more -- nothing
// built on them may be launched.
constexpr uintptr_t kStandInTiles = uintptr_t(1) << 44, kStandInLinv = uintptr_t(1) << 45;

// The inputs that shape the structure and the lists.  (The switches that shape only the launch sequence enter ScheduleInput.)
struct PlanOptions {
    int rank = 0, world = 1;   // distributed factorisation: the elimination tree is cut for `world` ranks, the lists are rank's
    bool own_all = false;      // self-test: cut the tree for `world` ranks but let this rank own every subtree
    int two_side = 1;          // second side stream: 0 off, 1 by plan size, 2 always
    int flow_cols = -1, flow_rows = 24;   // dataflow launch: trailing groups of at most so many columns / off-diagonal tiles per column; 0 off, < 0 by cost model
    int64_t max_updates = 80000000LL;     // tile products per factorisation a plan may hold (12.7 s at 45 TF/s)
    double cost_limit_ms = 0.0;           // a plan predicted to cost more per solve is refused; <= 0: no limit
    // Updates of DIAGONAL tiles (A == B) compute the 48 x 48 blocks on and left of the diagonal only (chol_kernels.hip).  Read by
    // the launches alone (TilePlan::issue): the structure, the lists and the schedule are the same either way
    // (tests/test_diag_update_lower_host.py)
    int diag_lower = 1;
};

using PlanCols = std::vector<std::vector<int>>;

struct PlanStructure {
    int nt = 0;
    PlanCols col_rows;            // per tile column: its off-diagonal rows after fill, ascending (parent = the first)
    std::vector<int> cls;         // per tile column: 0 another rank's, 1 this rank's, 2 top (shared)
    std::vector<int> owner;       // per tile column: owning rank, -1 top
    int n_top_cols = 0;
    double local_frac = 1.0;      // this rank's share of the tile operations below the top
    // slot order: touched non-top | touched top | fill non-top | fill top; inside the non-top parts owner by owner
    std::vector<int> slot, diag_slot;   // [nt * nt] (-1: no tile), [nt]
    std::vector<std::pair<int64_t, int64_t>> own_range, own_fill;   // per rank: first slot, count of the touched / fill tiles of its columns
    int64_t n_t_nt = 0, n_f_nt = 0, n_slots = 0, n_touched = 0;
    int64_t n_potrf = 0, n_trsm = 0, n_upd = 0;   // tile operations of one factorisation of every column
    // The level groups in execution order: this rank's columns level by level, then the shared top columns level by level
    // (a plan that is not distributed has the first kind only); other ranks' columns get no tasks at all.
    int n_true_levels = 0, n_local_groups = 0;   // elimination-tree levels (heights above the leaves); groups of this rank's columns
    PlanCols group_cols, row_cols;               // per group: its columns; per tile row: the columns of this rank and of the top with a tile there
    std::vector<int> group_of;                   // per column: its group (-1: another rank's)
    double predicted_ms = 0.0;                   // predict_solve_ms of this structure
    int refused = 0;                             // 1 update list beyond max_updates, 3 predicted cost above cost_limit_ms
    std::string message;                         // ... and the refusal in words

    int n_levels() const { return (int)group_cols.size(); }   // level GROUPS: local groups first, then the top groups
    bool distributed() const { return n_local_groups < n_levels(); }
    int slot_of(int I, int J) const { return slot[(size_t)I * nt + J]; }
};

struct PlanLists {
    std::vector<PotrfTask> potrf;
    std::vector<GemmTask> panel, upd;
    std::vector<std::pair<int64_t, int64_t>> upd_rounds;   // per conflict-free update round: first task, count
    std::vector<Level> lv;                                 // [n_levels + 1] (factor_schedule.h)
    std::vector<int> bwd_step;                             // [n_levels + 1] first task of each backward-sweep step (root group first)
    std::vector<TriTask> fwd, bwd;                         // the sweeps level by level
    std::vector<FlowTask> flow_fwd, flow_bwd;              // ... and as one dataflow launch each
    int n_flow_local = 0;   // distributed plans: the forward dataflow tasks of phase 0 (the rest: the top columns, phase 1)
    int n_flow_parts = 0;   // 144-vectors of the dataflow sweeps' partial array
    std::vector<int> sym_row_ptr; std::vector<SymEntry> sym_entries; std::vector<SymTile> sym_tiles;   // PCG: the tiles non-zero before fill
    std::vector<FactorUnit> units;   // dataflow factorisation: [phase 0 units | phase 1 units]
    struct Flow { int g0 = 0, g1 = 0, first = 0, n = 0; double sim_us = 0.0; } flow[2];   // per phase: the groups inside its launch, its units, their simulated makespan
    bool two_side_plan = false;   // what PlanOptions::two_side came to for this plan
    // The FIRST update of every fill tile (a tile of L that is structurally zero in S) is flagged -- bit 0 of GemmTask::C in the
    // level lists, kFlowFirstWriter in the dataflow units -- and does not read its target (beta = 0): the fill tiles are then
    // neither cleared before a factorisation nor read by those updates.  first_ok: this plan qualifies (not distributed, has
    // fill tiles, no dataflow launch over shared top groups).
    bool first_ok = false;
    // updates whose target is a diagonal tile (A == B): [0] in the level lists that run, [1] in the dataflow launches (whole-tile
    // units once, 48 x 48 units once per tile and writer)
    int64_t n_diag_upd[2] = {0, 0};
};

// The switches that shape only the launch sequence: they and a plan's two values make its ScheduleInput.
struct ScheduleSwitches {
    bool overlap = true;
    int overlap_min = 2;   // U2 batches smaller than this stay on the main stream (swept 1..1024: flat up to 64)
    bool split_u1 = true;
    int split_u1_min = 4;
    // U2 batches of at least this many tasks get the flood gate.  Before U2 was split into U2a / U2b the gate was worth 0.3-0.4 ms
    // on final-13682 (8.3 -> 7.9, any threshold 2 .. 250); after the split it is neutral there (7.6-7.7 either way), +2-3 % on the
    // dense fronts of ladybug / venice, -2 % on sphere2500's small batches: kept for the large batches only
    int gate_min = 256;
    bool skip_idle_wait = false;   // tests only: bring back the round-3 schedule bug (no wait after a level without side-stream work)
    bool flow_on = true;           // the dataflow launches run (run-time state: off once one has timed out)
};
inline ScheduleInput schedule_input(const PlanStructure& s, const PlanLists& l, const ScheduleSwitches& w) {
    const PlanLists::Flow* f = l.flow;
    return ScheduleInput{l.lv, l.upd_rounds, s.n_levels(), s.n_local_groups, w.overlap, w.overlap_min, w.split_u1, w.split_u1_min, l.two_side_plan,
                         w.gate_min, w.skip_idle_wait, w.flow_on, {{f[0].g0, f[0].g1, f[0].first, f[0].n}, {f[1].g0, f[1].g1, f[1].first, f[1].n}}};
}

// Nested-dissection order of the tile graph.  adj: symmetric nt x nt 0/1 adjacency in the CALLER's tile order.  Returns
// perm[old] = new.  The last n_fixed_last tiles keep their places (the last tile may hold padding rows; a bundle-adjustment
// problem also parks its hub cameras there): they are eliminated last and left out of the dissection.
std::vector<int> tile_order(int nt, const std::vector<uint8_t>& adj, bool nested_dissection, int leaf, int n_fixed_last = 1);

// Predicted milliseconds of one factorisation + both sweeps of a plan with these operation counts on one MI355X: the tile
// products at the rate the factorisation sustains end to end on the headline shape (0.251 TFLOP in 6.5 ms = 38-40 TF/s, DESIGN
// section 5; panel products count 45 / 81, a diagonal tile's Cholesky + inverse a third of a product), the sweeps at two
// passes over the tiles of L at 4.2 TB/s, 30 us of dependent launches per elimination-tree level.  Host arithmetic on the
// structure: every rank of a distributed plan arrives at the same number.
double predict_solve_ms(int64_t n_potrf, int64_t n_trsm, int64_t n_upd, int64_t n_tiles, int n_levels);

// present: lower-triangular nt x nt 0/1 structure (I >= J) in the FINAL order.  A refused structure comes back complete, with
// `refused` and `message` set; no lists may be built from it.
PlanStructure plan_structure(int nt, const std::vector<uint8_t>& present, const PlanOptions& opts);

// The owner rank of every tile column (-1: shared top) that plan_structure arrives at for `world` ranks; empty when the plan
// will not be distributed.
std::vector<int> plan_owners(int nt, const std::vector<uint8_t>& present, int world);

// The lists of a plan on the tile arrays at `tiles` / `linv`, in this order: the level task lists, the two sweeps, the PCG
// lists, the dataflow launches, the first writers.  Returns "" or an error message.
std::string build_plan_lists(const PlanStructure& s, const std::vector<uint8_t>& present, const PlanOptions& opts, double* tiles,
                             double* linv, PlanLists* out);

}  // namespace apex
