// tile_plan.h -- tile-sparse symmetric positive definite system: structure, factorisation, solves.
//
// Shared by the bundle-adjustment backend (reduced camera matrix S) and the pose-graph backend
// (H = J^T J + lambda I).  A matrix of nt x nt tiles of 144 x 144 doubles, lower triangle only:
//   build()   the device half of a plan: everything derived from the 0/1 tile structure -- symbolic Cholesky fill, partition,
//             slot map, level groups, batched task lists -- is a host value (plan_lists.h: PlanStructure, PlanLists) that
//             build() has made, allocates the tiles for and uploads; the plan keeps both and never writes them again
//   factor() / solve()   level-scheduled tile Cholesky and triangular solves, replayed as hipGraphs
//   pcg()     Jacobi-preconditioned CG on the unfactored tiles: a class of its own, tile_pcg.h
//   inverse() the selected inversion of the held factor (marginal covariances): a class of its own, tile_sinv.h
//
// Distributed factorisation (set_partition(rank, world) before build()): the elimination tree is cut below its top
// separators into `world` groups of independent subtrees.  A rank factorises the columns of ITS subtrees only (the
// "local" levels), the updates every rank adds to the shared top tiles are summed in ONE exchange, and the few top
// columns -- latency-bound, a small fraction of the flops -- are factorised redundantly by every rank.  The
// triangular solves follow the same pattern: local forward sweep, one n_pad-vector exchange for the top blocks,
// replicated top sweeps, local backward sweep, one n_pad-vector exchange that assembles x on every rank.
// factor()/solve() run the phases and issue the exchange lists (exchange()) through the communicator hook in between;
// factor_phase()/solve_phase() expose the same phases so that several instances can be driven in lockstep inside one process (tests).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <array>
#include <functional>
#include <string>
#include <utility>
#include <vector>

#include "chol_kernels.h"
#include "device_buffer.h"
#include "factor_schedule.h"
#include "plan_lists.h"
#include "rank_exchange.h"
#include "tile_pcg.h"
#include "tile_sinv.h"

namespace apex {

// Everything a TilePlan allocates through HIP, as a base of its own: release() drops all of it with one assignment (no list
// of members to keep in step), and the base is destroyed after ~TilePlan has destroyed the graph execs that point into it.
struct TilePlanMemory {
    DeviceBuffer<double> tiles_, linv_;
    DeviceBuffer<int> slot_, diag_slot_, flag_;
    DeviceBuffer<int> cls_;          // per tile column: 0 another rank's, 1 this rank's, 2 top (shared)
    DeviceBuffer<double> exch_;
    DeviceBuffer<int> gate_cnt_;     // [levels + 1] potrf workgroups that have started, per level
    DeviceBuffer<PotrfTask> potrf_tasks_;
    DeviceBuffer<GemmTask> trsm_tasks_, upd_tasks_;
    DeviceBuffer<TriTask> tri_fwd_, tri_bwd_;
    DeviceBuffer<FlowTask> flow_fwd_, flow_bwd_;   // dataflow triangular sweeps (single-GPU plans)
    DeviceBuffer<double> flow_part_;               // one 144-vector per off-diagonal tile
    DeviceBuffer<int> flow_flags_;                 // cnt[nt] | done[nt] | error word
    PinnedBuffer<int> flow_err_host_;              // [0] the error word behind the last solve(), [1..2] debug_occupy_cus
    DeviceBuffer<FactorUnit> flow_units_;          // dataflow factorisation of the top groups: [phase 0 units | phase 1 units]
    DeviceBuffer<int> flow_ver_;                   // per tile slot: finished strips of in-launch writers
    DeviceBuffer<unsigned long long> flow_trace_;
    DeviceBuffer<SymTile> sym_tiles_;              // the tiles non-zero before fill (scale_sym, TilePcg)
};

class TilePlan : private TilePlanMemory {
   public:
    TilePlan() = default;
    ~TilePlan();
    TilePlan(const TilePlan&) = delete;
    TilePlan& operator=(const TilePlan&) = delete;

    // present: lower-triangular nt x nt 0/1 structure (I >= J) in the FINAL order.
    // Returns "" on success or an error message.
    std::string build(int nt, const std::vector<uint8_t>& present, hipStream_t stream);

    // ---- distributed factorisation ----
    // one exchange over the ranks, in place, enqueued on `stream`; false = a collective failed (its text is with the hook's owner)
    using Comm = std::function<bool(const ExchangeList& list, hipStream_t stream)>;
    void set_partition(int rank, int world) { opts_.rank = rank; opts_.world = world; }  // before build()
    // self-test: cut the tree for `world` ranks but let THIS rank own every subtree -- the distributed schedule
    // (local levels, top levels, phased sweeps) then runs complete on one rank with no-op exchanges
    void set_own_all(bool on) { opts_.own_all = on; }
    void set_comm(Comm c) { comm_ = std::move(c); }
    bool distributed() const { return structure_.distributed(); }
    int n_top_columns() const { return structure_.n_top_cols; }
    double local_work_fraction() const { return structure_.local_frac; }  // this rank's share of the tile operations below the top
    // below the top tiles (summed after the local factorisation) the tiles of rank o's columns are contiguous: [first, first + count).
    // The local phase of rank o reads no other rank's columns, so a reduce to their owner (half the traffic of an all-reduce) is enough.
    int part_world() const { return opts_.world; }
    std::pair<int64_t, int64_t> owner_slot_range(int o) const { return structure_.own_range[o]; }
    // What the ranks exchange at the plan's points, each following one phase below: 1 (behind factor_phase(0)) the sums of the
    // top tiles, touched and fill; 2 (behind factor_phase(1)) the max of the factorisation's two failure words; 3, 4 (behind
    // solve_phase(0), (1)) the sum of the exchange vector.  factor() and solve() issue these lists through the hook.
    ExchangeList exchange(int point) const;
    void factor_phase(int phase);                  // 0: local levels, 1: top levels (after the top tiles were summed)
    int* flag_dev() const { return flag_; }       // [0] first failed tile column + 1, [1] the dataflow factorisation's error word
    // 0: local forward sweep, top blocks of the right-hand side packed into the exchange vector [summed over the ranks];
    // 1: top sweeps + local backward sweep, this rank's blocks of x packed into the vector [summed]; 2: x := the vector
    void solve_phase(int phase, const double* rhs, double* x, double* work);

    int nt() const { return structure_.nt; }
    int64_t n_pad() const { return (int64_t)structure_.nt * kNB; }
    int64_t n_slots() const { return structure_.n_slots; }
    int64_t n_touched_slots() const { return structure_.n_touched; }  // tiles non-zero before fill come first
    int n_levels() const { return structure_.n_levels(); }   // level GROUPS: local groups first, then the top groups
    const std::vector<std::vector<int>>& group_columns() const { return structure_.group_cols; }   // per level group, execution order: its tile columns
    // tile operations of one factorisation: potrf+inverse, panel products, trailing updates (each 2*144^3 flop for the last two)
    void op_counts(int64_t* potrf, int64_t* trsm, int64_t* upd) const { *potrf = (int64_t)lists_.potrf.size(); *trsm = (int64_t)lists_.panel.size(); *upd = (int64_t)lists_.upd.size(); }
    double* tiles() const { return tiles_; }
    const double* linv() const { return linv_; }   // [nt] inverses of the diagonal tiles of L (written by the factorisation)
    const int* slot_host() const { return structure_.slot.data(); }
    int slot(int I, int J) const { return structure_.slot_of(I, J); }
    TileMap tilemap() const { return TileMap{tiles_, slot_, structure_.nt}; }
    const int* diag_slot_dev() const { return diag_slot_; }
    void enable_graphs(bool on) { use_graphs_ = on; }
    void enable_overlap(bool on) { sw_.overlap = on; }  // before the first factor()
    void set_overlap_min(int n) { sw_.overlap_min = n; }
    void set_two_side(int mode) { opts_.two_side = mode; }   // 0 off, 1 by plan size (default), 2 always (tests); before build()
    void set_gate_min(int n) { sw_.gate_min = n; }   // flood gate in front of U2 batches of at least n tasks (0: off); before the first factor()
    // The top of the elimination tree as one dataflow launch (k_factor_flow): the trailing level groups of a phase whose
    // groups have at most max_cols columns each, every column with at most max_rows off-diagonal tiles.  0 columns: off;
    // < 0 (default): where the launch starts is chosen by a cost model.  Before build().
    void set_factor_flow(int max_cols, int max_rows) { opts_.flow_cols = max_cols; if (max_rows > 0) opts_.flow_rows = max_rows; }
    // level groups inside the dataflow launches THAT RUN: none once a launch has timed out
    int factor_flow_groups() const { return !sw_.flow_on ? 0 : (lists_.flow[0].g1 - lists_.flow[0].g0) + (lists_.flow[1].g1 - lists_.flow[1].g0); }
    int factor_flow_cols() const { return opts_.flow_cols; }
    // Updates of diagonal tiles compute the 48 x 48 blocks on and left of the diagonal only (default; chol_kernels.hip,
    // "diag_lower").  Any time: the captured factorisations are dropped.
    void set_diag_lower(bool on);
    bool diag_lower() const { return opts_.diag_lower != 0; }
    int64_t n_diag_updates() const { return lists_.n_diag_upd[0] + (sw_.flow_on ? lists_.n_diag_upd[1] : 0); }   // of the factorisation that runs
    double factor_flow_sim_us() const { return lists_.flow[0].sim_us + lists_.flow[1].sim_us; }
    int factor_flow_units() const { return lists_.flow[0].n + lists_.flow[1].n; }
    // A dataflow factorisation whose waits ran into their spin limit leaves the tiles half updated: factor() reports it here
    // (once) and the plan goes back to the level launches for good; the caller re-assembles and factorises again.
    // tools/flow_bench: per-unit stamps of the next factorisations (dispatched, inputs ready, done; 100 MHz) + the unit list
    hipError_t enable_flow_trace();
    hipError_t read_flow_trace(std::vector<FactorUnit>* units, std::vector<unsigned long long>* stamps);
    bool refused_too_large() const { return refused_ == 1; }
    bool refused_no_memory() const { return refused_ == 2; }
    bool refused_by_cost() const { return refused_ == 3; }
    double predicted_ms() const { return structure_.predicted_ms; }          // of the structure the last build() saw (also when it refused)
    void set_cost_limit_ms(double ms) { opts_.cost_limit_ms = ms; }     // before build(); <= 0: no limit
    void set_max_updates(int64_t n) { opts_.max_updates = n > 0 ? n : PlanOptions().max_updates; }   // (tests lower it to force the refusal on a small problem)
    bool factor_flow_gave_up() { const bool g = flow_gave_up_; flow_gave_up_ = false; return g; }
    void set_split_u1(int min_tasks) { sw_.split_u1 = min_tasks > 0; if (min_tasks > 0) sw_.split_u1_min = min_tasks; }   // before the first factor()
    hipError_t read_flags(int* failed_at);   // pivot flag of the last factorisation (syncs)
    void enable_tri_flow(bool on);   // triangular sweeps as one dataflow launch each (default) or level by level
    bool tri_flow() const { return tri_flow_; }
    // The dataflow sweeps bound their waits (chol_kernels.hip, flow_wait): a sweep that gave up leaves a WRONG x and raises
    // an error word, which solve() posts to pinned host memory behind the sweeps (in a distributed plan after a max over
    // the ranks, so that every rank takes the same decision).  Valid once the plan's stream has been synchronised behind
    // solve(); reading clears it.  The caller repeats that solve with enable_tri_flow(false).
    bool sweep_timed_out();
    bool sweep_timed_out_peek() const { return flow_err_host_ && flow_err_host_[0] != 0; }   // the same word, not cleared
    int sweep_timeouts() const { return n_sweep_timeouts_; }
    // tests only: the next solve()'s forward (1) / backward (2) dataflow sweep runs into its spin limit on purpose
    void debug_poison_next_solve(int which) { poison_ = which; }
    // tests only: the next factorisation's dataflow launch cannot finish (one version counter is made unreachable)
    void debug_poison_next_factor() { poison_factor_ = true; }
    // tests only: block n_cus compute units (all of their LDS) for `micros`, starting now, on a stream of their own;
    // returns once the blocking workgroups are resident (or after 200 ms)
    hipError_t debug_occupy_cus(int n_cus, int micros);

    // async on the plan's stream.  own_touched_only: (distributed plans) this rank adds to the tiles of its own columns and
    // of the shared top only -- tree-sharded landmarks; the other ranks' tiles are then left alone
    // skip_fill (round 5): the assembly is for the Cholesky factorisation of a single-GPU plan whose first writers are flagged
    // (first_writers_flagged()): the fill tiles are not cleared -- their first update does not read them
    hipError_t zero_tiles(bool own_touched_only = false, bool skip_fill = false);
    bool first_writers_flagged() const { return lists_.first_ok; }
    void add_diag(int n_valid, double add_valid, double pad_value);  // diagonal += / padding rows := value
    void diag(double* out) const;                        // out[n_pad] = diagonal
    void scale_sym(const double* scale);                 // A := D A D on the unfactored tiles, D = diag(scale[n_pad])
    // Cholesky in place; *failed_at = 0 or (tile column + 1) of the first non-positive pivot.  Syncs.
    // defer_flags: do not wait for the pivot flag (single-rank plans only): the caller enqueues the sweeps behind the
    // factorisation and calls read_flags() at its own synchronisation point (Solver::solve_augmented: one host wait per solve)
    hipError_t factor(int* failed_at, bool defer_flags = false);
    // x = (L L^T)^-1 rhs ; work: 2*n_pad doubles ; all on the plan's stream, no sync.  hipErrorUnknown: a collective of
    // the distributed sweeps failed (the communicator's own message is with the caller)
    hipError_t solve(const double* rhs, double* x, double* work);
    // y = A x on the UNFACTORED tiles (deterministic two-pass symmetric product), no sync
    void sym_matvec(const double* x, double* y) { pcg_.matvec(x, y); }
    // Jacobi-PCG on the UNFACTORED tiles; work: 6*n_pad doubles; syncs once per iteration
    hipError_t pcg(const double* rhs, double* x, double* work, int max_iter, double tol, int* iters) { tiles_written(); return pcg_.solve(rhs, x, work, max_iter, tol, iters); }
    const double* pcg_scalars() const { return pcg_.scalars(); }   // device: ExplicitPcgScalars as the last pcg() left them (tests)

    // The tiles hold a valid factor L only between a successful single-rank factorisation + sweeps (the CALLER says so with
    // set_factor_valid(true) once it has read the pivot flags) and the next write of the tiles: zero_tiles, add_diag,
    // scale_sym, factor, pcg, a new build() clear the flag.  Every such write and every factor declared valid starts a new
    // epoch, by which the selected inversion knows whether its Z is of the factor now held.
    void set_factor_valid(bool on) { factor_valid_ = on; ++factor_epoch_; }
    bool factor_valid() const { return factor_valid_; }
    // marginal covariances of the held factor (tile_sinv.h), on a view of the plan as it is at this call
    SelectedInverse& inverse();
    const SelectedInverse& inverse() const { return inverse_; }   // its counters and times

   private:
    std::string refuse_by_memory();
    std::string upload();   // the device step of build(): lists_ and the maps of structure_ to the device, work arrays, streams, events
    ScheduleInput input() const;
    void issue(const std::vector<SchedOp>& ops);   // one HIP call per op
    void enqueue_factor(int g0, int g1) { issue(factor_schedule(input(), g0, g1)); }
    void enqueue_solve(const double* rhs, double* x, double* work);
    void launch_fwd_group(int lv, double* bvec, double* yvec, hipStream_t s);
    void enqueue_dist_solve(int phase, const double* rhs, double* x, double* work);
    bool run_graph(int which, const double* rhs, double* x, double* work);
    void release();

    PlanOptions opts_;          // what shapes structure_ and lists_ (the setters, before build())
    ScheduleSwitches sw_;       // what shapes the launch sequence only (input()); flow_on: run-time state, see factor_flow_gave_up
    PlanStructure structure_;   // written by build() alone
    PlanLists lists_;           // written by build() alone (release() empties it)
    int n_flow_fwd() const { return (int)lists_.flow_fwd.size(); }   // the dataflow sweeps: tasks of the forward / backward launch
    int n_flow_bwd() const { return (int)lists_.flow_bwd.size(); }
    int n_sym_tiles() const { return (int)lists_.sym_tiles.size(); }
    Comm comm_;
    hipStream_t stream_ = nullptr;
    hipStream_t side_ = nullptr;  // trailing updates that the next level does not need (factor_schedule)
    hipStream_t side2_ = nullptr; // U2b2: the bulk of U2 (targets four levels up and more)
    hipStream_t so_ = nullptr;    // U1o: updates of the next level's off-diagonal tiles, beside its potrf
    // the handles behind the schedule's stream and event ids (issue)
    hipStream_t stream_of(uintptr_t s) const { return s == kMain ? stream_ : s == kSide ? side_ : s == kSide2 ? side2_ : so_; }
    std::vector<std::array<hipEvent_t, kLevelEvents>> ev_;
    int* flow_err_host_dev_ = nullptr;                     // the device address of flow_err_host_ (mapped pinned memory)
    int n_sweep_timeouts_ = 0;
    int poison_ = 0;
    bool poison_factor_ = false;
    hipStream_t occ_stream_ = nullptr;
    bool post_sweep_status(bool reduce);   // false: the max-reduction over the ranks failed
    int refused_ = 0;                       // why the last build() gave up: 1, 3 PlanStructure::refused, 2 tiles beyond the free memory
    bool flow_gave_up_ = false;
    bool tri_flow_ = true;
    enum Graph { kGraphFactor, kGraphSweeps, kGraphFactorTop, kGraphDistSolve0, kGraphDistSolve1, kGraphs };   // (run_graph)
    hipGraphExec_t graph_exec_[kGraphs] = {};
    const double* graph_rhs_[kGraphs] = {};
    double *graph_x_[kGraphs] = {}, *graph_work_[kGraphs] = {};
    bool graph_failed_[kGraphs] = {};
    void tiles_written() { factor_valid_ = false; ++factor_epoch_; }   // the one place (with set_factor_valid) that touches these two
    bool factor_valid_{false};
    uint64_t factor_epoch_ = 0;
    SelectedInverse inverse_;
    TilePcg pcg_;
    bool use_graphs_ = true;
};

}  // namespace apex
