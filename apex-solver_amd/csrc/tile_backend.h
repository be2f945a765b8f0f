// tile_backend.h -- what the two backends that factorise on a TilePlan share (solver.h: S of bundle adjustment, pg_solver.h: H of a
// pose graph): the plan, the stream and their order of destruction, the state of one solve and the trial-step protocol on it, the switches that go to the plan,
// the protocol around one direct solve -- speculative factorisation, one host wait, the repairs of a dataflow launch that gave up --
// and the Dog-Leg step on that solve (TrBackend, tr_loop.h): its state, its host protocol and its tail of vector kernels, once.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <initializer_list>
#include <string>

#include "column_map.h"
#include "device_buffer.h"
#include "dogleg_kernels.h"
#include "dogleg_scalars.hpp"
#include "jacobi_scaling.h"
#include "lm_loop.h"
#include "stage_timer.h"
#include "step_state.h"
#include "tile_plan.h"
#include "tr_loop.h"

namespace apex {

// HIP_TRY(expr): the text of a failure goes to err_; HIP_TRY(expr, err): to *err (a step on a thread that does not own err_)
#define HIP_TRY(expr, ...)                                    \
    do {                                                      \
        int _rc = check_hip((expr), #expr, ##__VA_ARGS__);    \
        if (_rc != kOk) return _rc;                           \
    } while (0)

class TileBackend : public TrBackend {
   public:
    void enable_graphs(bool on) { tp_.enable_graphs(on); }
    void enable_overlap(bool on) { tp_.enable_overlap(on); }
    void enable_tri_flow(bool on) { tp_.enable_tri_flow(on); }
    int sweep_timeouts() const { return tp_.sweep_timeouts(); }   // dataflow sweeps that gave up and were repeated level by level
    void debug_poison_next_solve(int which) { tp_.debug_poison_next_solve(which); }
    void debug_poison_next_factor() { tp_.debug_poison_next_factor(); }
    void set_split_u1(int min_tasks) { tp_.set_split_u1(min_tasks); }
    void set_overlap_min(int n) { tp_.set_overlap_min(n); }
    void set_gate_min(int n) { tp_.set_gate_min(n); }
    void set_two_side(int mode) { tp_.set_two_side(mode); }
    void set_diag_lower(bool on) { tp_.set_diag_lower(on); }
    void set_factor_flow(int max_cols, int max_rows) { tp_.set_factor_flow(max_cols, max_rows); }
    int factor_flow_timeouts() const { return n_factor_flow_timeouts_; }
    // "one_wait": one host wait per direct solve (direct_solve), 0 = the flags are waited for where they are raised.
    // "eager_step_eval": what the LM loop asks next of every solve -- the step statistics and the trial point with its cost --
    // is enqueued behind the step and read at the solve's own wait: step_stats / eval_step then answer from the host, without a
    // launch or a wait of their own (three device round trips per LM iteration become one).
    void set_one_wait(bool on) { one_wait_ = on; }
    void set_eager_step_eval(bool on) { eager_eval_ = on; }
    void set_nd(bool on, int leaf) { use_nd_ = on; if (leaf > 0) nd_leaf_ = leaf; }
    void enable_covariance_timing(bool on) { tp_.inverse().enable_timing(on); }
    void enable_stage_timing(bool on) { timer_.enable(on); }
    void enable_stage_timing_only(uint32_t stage_mask) { timer_.enable_only(stage_mask); }
    void reset_stage_times() { timer_.reset(); }
    int stage_times(double* ms, int64_t* launches) { return timer_.times(ms, launches); }   // averaged HIP-event time per stage since reset
    int n_levels() const { return tp_.n_levels(); }
    const TilePlan& plan() const { return tp_; }
    const char* last_error() const override { return err_.c_str(); }
    // The trial-step protocol behind a solve, on StepState (step_state.h): answers the solve posted at its own wait are served from
    // the host, else the hooks below are enqueued and read back with one wait.
    int step_stats(double out3[3]) final;       // |g|, |step|, predicted reduction
    int eval_step(double* trial_cost) final;    // x (+) step into the trial set, its cost
    int commit_step() final;
    int discard_step() final;                   // reference semantics: trial (+) (-step), not a snapshot -- unless keeps_current_on_discard()
    // The Dog-Leg step (tr_loop.h), to ONE host wait, fresh or reused.  Fresh: solve_for_dogleg with dl_mode_ on, whose finish_step
    // runs enqueue_dogleg_tail behind the step: the inner products, the Gram pass, the combine (one lane), the blended step into
    // the step vector, the trial point and its cost, one copy of DoglegScalars -- posted as the solve's answers, so step_stats /
    // eval_step answer from the host.  Reused: the tail from the combine on; the six sums of the last fresh solve, the gradient
    // and the cached Gauss-Newton step are all it reads.  Checked in this order: the solver's refusal, radius and mu
    // (kInvalidInput), reuse without a cache (kInvalidState); only then is anything allocated.
    int dogleg_step(double mu, double radius, int reuse, DoglegStepInfo* out) final;

   protected:
    // stats_stage: the solver's stage the Dog-Leg tail and the Gram pass are booked under; n_partial: the blocks of a reduction
    TileBackend(int device, int n_stages, int nd_leaf, int stats_stage, int n_partial)
        : device_(device), nd_leaf_(nd_leaf), timer_(n_stages), n_partial_(n_partial), stats_stage_(stats_stage) {}
    int fail(int code, const std::string& msg) { err_ = msg; return code; }
    int check_hip(hipError_t e, const char* what, std::string* err = nullptr);   // err: where the text goes instead of err_
    void begin_solve(double lambda) { st_.begin_solve(); last_lambda_ = lambda; }
    // finish_step's eager evaluation, enqueued behind the step; then, when finish_step has waited, the answers of THIS solve
    int enqueue_eager_eval();
    void post_eager_answers() { st_.post_answers(answers_from_sums(eager_host_)); }
    int answers_of_step(bool trial, StepAnswers* out);
    // The sweeps and the step on the system rebuild_system() built, to the one host wait.  speculative: the factorisation is
    // enqueued here with its flags deferred to that wait; else the caller has factorised and read them.
    int direct_solve(bool speculative, double lambda, double* step_out, double* grad_out);
    int factor_fresh(double lambda, double reg, int* failed);   // factor_now on the system rebuild_system(lambda, reg) has just built, flags waited for; a give-up is repaired
    int factor_again(double lambda, double reg, int* failed);   // after a dataflow factorisation that gave up
    // Device vectors in internal order to the caller's columns of `out`, with ONE host wait for all segments: each is copied to the
    // host, unscaled when Jacobi scaling is on -- the caller's variables are the scaled ones: a step is divided by s, a gradient
    // multiplied by it, kPlain is left as it is -- and scattered by its map, 0 to the map's untouched columns.
    enum class ExportAs { kPlain, kStep, kGradient };
    struct ExportSegment { const double* dev; const ColumnMap* map; const JacobiScaling* scale; };
    int export_columns(std::initializer_list<ExportSegment> segs, ExportAs as, double* out);
    // Every lower tile whose slot is below slot_bound to the host (a wait per tile) and, by the map, into both triangles of the
    // dense row-major matrix `out` of leading dimension ld.  The padding rows are not in the map and stay out.
    int export_tiles_dense(const ColumnMap& map, int64_t ld, int64_t slot_bound, double* out);

    // What the protocol asks of a solver ("The direct solve's hooks, by name").
    virtual int rebuild_system(double lambda, double reg) = 0;            // the matrix (diagonal + reg) and right-hand side, ready to factorise
    virtual int factor_now(int* failed, bool defer_flags) = 0;           // tp_.factor under the solver's stage timer
    virtual int enqueue_sweeps() = 0;                                     // tp_.solve into the solver's step vector
    virtual int finish_step(double* step_out, double* grad_out) = 0;     // the rest of the step, eager evaluation, export; ends in the host wait
    virtual int recover_factor(double lambda, int failed, bool gave_up) = 0;   // a factorisation with a failed pivot or a give-up: a good factor, or the error
    virtual const int* own_flag() const { return nullptr; }              // a device flag of the solver's own, read at the speculative solve's wait
    virtual int own_flag_raised() { return kOk; }                         // ... and the failure it stands for
    virtual void keep_factor() { tp_.set_factor_valid(true); }            // pivots read, sweeps clean: the covariance calls may invert this factor
    // ... and the trial-step protocol (same section)
    virtual int enqueue_step_stats() = 0;                                 // the step's sums into step_sums()
    virtual int enqueue_trial_point(double* sumsq_out) = 0;               // current (+) step into the trial set, the sum of squares there
    virtual int enqueue_retract(int from, double sign, int to) = 0;       // set `to` = set `from` (+) sign * step, ready to be evaluated
    // true: discard_step leaves the current parameter set as it is (it still holds x: the trial point is in the other set) instead of
    // retracting the trial point by -step.  The parameters then come back bit for bit, and differ from the reference solver's, which
    // applies the negative step, by the rounding of x (+) d (+) (-d).  Only an SO3 pose graph answers true.
    virtual bool keeps_current_on_discard() const { return false; }
    virtual double* step_sums(int* n) = 0;                                // device: the *n sums of enqueue_step_stats, the trial point's slot behind them
    virtual StepAnswers answers_from_sums(const double* h) const = 0;     // a host copy of those *n + 1 doubles as named answers
    virtual void params_moved() {}                                        // the current parameters are other ones now (commit, discard)
    // ... and the Dog-Leg step (same section)
    virtual int dogleg_refusal() = 0;                                     // kOk, or why this handle takes no Dog-Leg call now (its text in err_)
    virtual int dogleg_segments(DlSegment out[2]) = 0;                    // the pieces of gradient and step (1 | 2), a and h left out
    virtual void enqueue_jv_gram(const double* const a[2], const double* const b[2], double* out3) = 0;   // {|J a|^2, (J a).(J b), |J b|^2}, a and b per segment
    virtual int solve_for_dogleg(double mu) = 0;                          // the solver's solve_augmented(mu) behind its checks, no export; dl_mode_ is on
    virtual void dogleg_trial_begins() {}                                 // the tail is about to write the trial point of the BLENDED step, all of it

    // everything of a Dog-Leg step behind the solve, up to the copy to dl_host_: a finish_step in dl_mode_ calls it with fresh
    int enqueue_dogleg_tail(bool fresh);
    // The solvers' parity export jv_gram behind their own refusals: a, b in the caller's columns, gathered through the segments'
    // maps and zero-padded, to out3.  One wait; booked under the stats stage; the Dog-Leg cache stays.
    int jv_gram_columns(const double* a, const double* b, double out3[3]);
    void drop_dogleg_cache() { have_dl_cache_ = false; }
    // What a setter did to the handle.  Each solver has ONE function over these, voided_by(), that says which cached state the
    // change voids (a pending step and trial point, the Dog-Leg cache, and what else the solver keeps): the table of DESIGN.md,
    // "What a change voids".  The solve path (assemblies, factorisations, exports that assemble) keeps its own direct calls.
    enum class Change { kStructure, kParams, kLoss, kPriors, kInformation, kScalingOff, kScalingVectors };
    // set_structure: they are sized by the old structure, dogleg_step allocates them again
    void release_dogleg_buffers() { for (int k = 0; k < 2; ++k) { dl_h_[k].reset(); dl_a_[k].reset(); } dls_.reset(); }

    int device_;
    StepState st_;
    double last_lambda_ = 0.0;
    bool one_wait_ = true, eager_eval_ = true;
    bool scaled_ = false;   // Jacobi column scaling is on: the solver's JacobiScaling holders are what the system is scaled by
    int n_factor_flow_timeouts_ = 0;
    bool use_nd_ = true;
    int nd_leaf_;
    std::string err_;
    hipStream_t stream_ = nullptr;
    // destroys stream_ when the members below it and every member of the solver are gone: the solver's destructor synchronises the
    // stream, then its buffers are freed, then the plan and the rest here in reverse order of declaration, then this runs
    struct StreamLast { hipStream_t& s; ~StreamLast() { if (s) (void)hipStreamDestroy(s); } } stream_last_{stream_};
    TilePlan tp_;   // the tiles, their factorisation and solves
    StageTimer timer_;
    PinnedBuffer<double> eager_host_;   // the eager evaluation's sums as step_sums() lays them out: read by answers_from_sums only
    DeviceBuffer<double> partial_;   // reduction scratch of the solver's kernels and the tail's: the solver allocates 3 n_partial_ or more
    const int n_partial_;
    bool dl_mode_ = false;   // inside a fresh dogleg_step: finish_step runs the tail instead of the LM evaluation and the export

   private:
    // Dog-Leg state, allocated by the first dogleg_step
    const int stats_stage_;
    DeviceBuffer<double> dl_h_[2], dl_a_[2];   // per segment: the cached (unscaled) Gauss-Newton step; D^2 g, the direction the Gram pass prices g_s with
    DeviceBuffer<DoglegScalars> dls_;          // sums[] is kept from the last fresh solve
    PinnedBuffer<DoglegScalars> dl_host_;
    DeviceBuffer<double> jv_out_;              // jv_gram_columns' three sums
    double dl_radius_ = 0.0;
    bool have_dl_cache_ = false;   // the gradient, dl_h_, dls_->sums belong to one solve and the scaling is what it was then
};

}  // namespace apex
