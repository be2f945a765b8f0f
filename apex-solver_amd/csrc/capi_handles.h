// capi_handles.h -- the opaque handles of include/apexgpu.h and what their entry points answer alike, for capi.cpp (bundle
// adjustment), capi_pg.cpp (pose graphs), capi_debug.cpp (host arithmetic, lockstep solve) and tile_debug.cpp.  The solver
// behind a handle is reached through with_handle() (capi_guard.h), which is where the rule of the boundary lives.
#pragma once
#include <string>
#include <vector>

#include "capi_guard.h"
#include "pg_solver.h"
#include "solver.h"
#include "tile_plan.h"

namespace apex {
// what apexgpu_debug_tiles_* (tile_debug.cpp) keeps per handle: a TilePlan on a matrix the caller chooses
struct TileSession {
    int device = 0;
    hipStream_t stream = nullptr;
    DeviceBuffer<double> rhs, x, work;   // kept for the handle's life: the captured sweeps hold their addresses
    DeviceBuffer<double> pcg_work;       // 6 * n_pad doubles, allocated by the first pcg call
    TilePlan plan;                       // (declared last: its graph execs go before the buffers they point into)
};
}  // namespace apex

struct apexgpu_solver : apex::Handle<apex::Solver> {};
struct apexgpu_pg_solver : apex::Handle<apex::PoseGraphSolver> {};
struct apexgpu_tiles : apex::Handle<apex::TileSession> {};

using apex::guarded;
using apex::with_handle;

static_assert(sizeof(apexgpu_lm_config) == sizeof(apex::LmConfig), "LmConfig layout");
static_assert(sizeof(apexgpu_lm_iter) == sizeof(apex::LmIterRecord), "LmIterRecord layout");
static_assert(sizeof(apexgpu_lm_result) == sizeof(apex::LmResult), "LmResult layout");
static_assert(sizeof(apexgpu_gn_config) == sizeof(apex::GnConfig), "GnConfig layout");
static_assert(sizeof(apexgpu_dl_config) == sizeof(apex::DlConfig), "DlConfig layout");
static_assert(sizeof(apexgpu_dl_iter) == sizeof(apex::DlIterRecord), "DlIterRecord layout");
static_assert(sizeof(apex::DoglegStepInfo) == 8 * sizeof(double), "DoglegStepInfo layout");
static_assert(APEXGPU_NUM_STAGES == apex::kNumStages, "stage count");
static_assert(APEXGPU_PG_NUM_STAGES == apex::kPgNumStages, "pose-graph stage count");

// The optimise calls: the ABI's config / result / history structs are the loops' own (layouts asserted above).
template <typename S, typename Cfg, typename Iter, typename CCfg, typename CIter>
int optimize_call(S& s,int (S::*loop)(Cfg*, apex::LmResult*, Iter*, int), CCfg* cfg, apexgpu_lm_result* result, CIter* history, int history_capacity) {
    if (!cfg || !result) return APEXGPU_ERR_INVALID_INPUT;
    return (s.*loop)(reinterpret_cast<Cfg*>(cfg), reinterpret_cast<apex::LmResult*>(result), reinterpret_cast<Iter*>(history), history ? history_capacity : 0);
}

template <typename S>
int covariance_stats(S* s, double out[6], double* group_ms, int group_cap) {
    if (!out) return APEXGPU_ERR_INVALID_INPUT;
    const apex::TilePlan& tp = s->plan();
    const apex::SelectedInverse& inv = tp.inverse();
    int64_t y = 0, zo = 0, zd = 0;
    inv.op_counts(&y, &zo, &zd);
    const std::vector<double>& ms = inv.group_ms();
    out[0] = (double)inv.bytes(); out[1] = (double)y; out[2] = (double)zo; out[3] = (double)zd; out[4] = tp.n_levels();
    int n = 0;
    if (group_ms)
        for (; n < group_cap && n < (int)ms.size(); ++n) group_ms[n] = ms[n];
    out[5] = n;
    return APEXGPU_OK;
}

// What both handles answer alike (tile_backend.h), over the handle's solver type: the option names they share (false: not one
// of them), the four counters, the stage-timing switch.
template <typename S>
bool shared_option(S* s, const std::string& n, int value) {
    if (n == "graphs") s->enable_graphs(value != 0);
    else if (n == "update_overlap") { s->enable_overlap(value != 0); if (value > 1) s->set_overlap_min(value); }
    else if (n == "tri_dataflow") s->enable_tri_flow(value != 0);
    else if (n == "split_u1") s->set_split_u1(value);
    else if (n == "flood_gate") s->set_gate_min(value);
    else if (n == "two_side") s->set_two_side(value);
    else if (n == "diag_update_lower") s->set_diag_lower(value != 0);
    else if (n == "eager_step_eval") s->set_eager_step_eval(value != 0);
    else if (n == "one_wait") s->set_one_wait(value != 0);
    else if (n == "factor_flow") s->set_factor_flow(value, 0);          // max columns per level group inside the dataflow launch (0: off)
    else if (n == "factor_flow_rows") s->set_factor_flow(s->plan().factor_flow_cols(), value);
    else if (n == "debug_poison_sweep") s->debug_poison_next_solve(value);   /* tests: 1 / 2 = the next solve's forward / backward dataflow sweep times out */
    else if (n == "debug_poison_factor") s->debug_poison_next_factor();       /* tests: the next factorisation's dataflow launch times out */
    else if (n == "nested_dissection") s->set_nd(value != 0, value > 1 ? value : 0);  /* value > 1: leaf size */
    else if (n == "covariance_timing") s->enable_covariance_timing(value != 0);   /* per level group times of the covariance calls, landmark pass time */
    else return false;
    return true;
}
template <typename S>
int counters(S* s, int64_t out[4]) {
    if (!out) return APEXGPU_ERR_INVALID_INPUT;
    out[0] = s->sweep_timeouts(); out[1] = s->plan().tri_flow() ? 1 : 0; out[2] = s->factor_flow_timeouts(); out[3] = s->plan().factor_flow_groups();
    return APEXGPU_OK;
}
template <typename S>
int stage_timing(S* s, int on) {
    if (on > 1) s->enable_stage_timing_only((uint32_t)on >> 1);   // bit k + 1 of `on`: stage k alone is timed
    else s->enable_stage_timing(on != 0);
    return APEXGPU_OK;
}
