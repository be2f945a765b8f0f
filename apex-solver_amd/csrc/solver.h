// solver.h -- host side of the MI355X bundle-adjustment backend (one instance per optimize()).
//
// Mirrors the reference's SparseSchurComplementSolver + the LM loop that drives it
// (src/linalg/sparse/explicit_schur.rs:1038-1243, src/optimizer/levenberg_marquardt.rs:702-1031)
// with every per-observation / per-landmark / per-camera stage on the device.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <string>
#include <thread>
#include <utility>
#include <vector>

#include "ba_kernels.h"
#include "ba_prior_kernels.h"
#include "ba_scalars.h"
#include "chol_kernels.h"
#include "schur_jacobi_pcg.h"
#include "schur_pairs.h"
#include "rank_exchange.h"
#include "tile_backend.h"

namespace apex {

enum Stage { kStAssembleCam = 0, kStAssembleLm, kStScatter, kStAllReduce, kStFactor, kStTriSolve, kStBackSub, kStStats,
             kStRetract, kStCost, kNumStages };

int mode_mask(int mode);  // 4 POSE + 2 LANDMARK + INTRINSIC of an APEXGPU_MODE_*
void shard_range(int64_t n_pt, const int64_t* ptr, int rank, int world, int64_t* lo, int64_t* hi);

class Solver : public TileBackend {
   public:
    Solver(int64_t n_cam, int64_t n_pt, int64_t n_obs, int mode, int device);
    ~Solver();

    int set_structure(const uint32_t* cam_idx, const uint32_t* pt_idx, const double* obs_uv, const int64_t* intr_col,
                      const int64_t* pose_col, const int64_t* pt_col, const uint8_t* fix_pose, const uint8_t* fix_intr,
                      const uint8_t* fix_pt, double huber_delta);
    // The loss of every ProjectionFactor block (pg_loss.hpp), in place of set_structure's huber_delta until the next
    // set_structure.  kInvalidInput, and nothing changes: a kind or parameter pg_loss_make refuses, and a loss whose corrector
    // can take its second arm (pg_loss_first_arm_only).  Voids a pending trial step, the projection records and
    // the landmark covariance's linearisation, as set_params does.
    int set_loss(int kind, double p0, double p1);
    void get_loss(int* kind, double out2[2]) const;
    // PriorFactor blocks on camera poses (intr false: data [tx,ty,tz,qw,qx,qy,qz], seven rows over the six pose columns) or on
    // camera intrinsics (intr true: data [f,k1,k2]; nine-column handles only), beside the projection factors (DESIGN.md §17;
    // prior_factor.rs:93-105 as PoseGraphSolver::set_priors restates it, plus a scalar weight w per block: r <- w r, J <- w J).
    // huber_delta / weight may be NULL (none / 1).  Replaces the set of its kind, n = 0 clears it; set_structure clears both.
    // Voids a pending trial step, the Dog-Leg cache and the factor the covariance calls read.  kInvalidInput (nothing changes): a
    // camera that does not exist, a NaN, a weight that is not finite and positive, intrinsics priors on a six-column handle.
    // kInvalidState: before set_structure, and on a sharded handle (multi-rank priors are not built).
    int set_priors(bool intr, int64_t n, const uint32_t* cam, const double* data, const double* huber_delta, const double* weight);
    int get_prior_residual(double* pose_r7_out, double* intr_r3_out);   // corrected, the caller's order; either may be NULL
    int64_t n_priors(bool intr) const { return intr ? intr_pri_.n : pose_pri_.n; }
    int set_params(const double* poses, const double* intr, const double* points);
    int get_params(double* poses, double* intr, double* points);
    void set_cg_params(int max_iter, double tol) { cg_max_iter_ = max_iter; cg_tol_ = tol; }

    // hot path
    int cost(double* out) override;                         // A16 on the current parameters
    int solve_augmented(double lambda, int variant, double* step_out, double* grad_out) override;
    int assemble_only(double lambda);
    int parameter_norm(double* out) override;
    int lm_optimize(LmConfig* cfg, LmResult* res, LmIterRecord* hist, int hist_cap);
    // Dog-Leg (tr_loop.h): what the reference's DogLeg computes on a bundle-adjustment problem -- there on a sparse
    // Cholesky of the whole H + mu I (optimizer/mod.rs:681-693), here on the Schur path: solve_augmented(mu, 0) damps Hcc and Hll by
    // the identity.  dogleg_step is TileBackend's; what this solver puts in are the hooks below: two segments (the camera and the
    // landmark half of g and the step, blended into dcam_ / dl_), the Gram pass over the observations (k_ba_jv_gram) and
    // solve_for_dogleg.  A failed factorisation is kFactorizationFailed (a raised landmark flag kSingularMatrix) WITHOUT the
    // regularisation ladder: the loop raises mu.  Refused, nothing changing: kInvalidState on a matrix-free handle (the option or
    // the automatic fallback: the PCG step is inexact, S is never factorised) and on several ranks.
    int dogleg_optimize(DlConfig* cfg, LmResult* res, DlIterRecord* hist, int hist_cap);   // variant != 0: kInvalidInput
    // parity export: {|J a|^2, (J a).(J b), |J b|^2} at the current parameters; a, b total-dof entries in the caller's column
    // order, as given (no scaling); single rank
    int jv_gram(const double* a, const double* b, double out3[3]);
    // Jacobi column scaling (optimizer/mod.rs:749-763; AssemblyBackend::compute_column_norms / apply_column_scaling,
    // linearizer/mod.rs:229-262).  With a scaling set, solve_augmented returns the SCALED step and gradient (what the
    // reference's solver returns for J diag(s)); the unscaled step stays on the device for eval_step.
    int column_norms(double* norms_out);                    // total_dof, global column order, at the current parameters
    int set_column_scaling(const double* scaling);          // total_dof, global column order; NULL: off
    int set_jacobi_scaling(bool on) override;               // on: s = 1 / (1 + norms) at the current parameters

    // the phases of the distributed Cholesky solve, for the single-process lockstep test (see solver.hip)
    int dist_phase(int phase, double lambda);
    // What the ranks exchange at point 0 (behind the assembly; for_factor as assemble() takes it) and at the plan's points 1..4
    // (TilePlan::exchange).  assemble() and the plan issue these lists; the lockstep test plays the same ones.
    ExchangeList exchange(int point, bool for_factor) const;
    int export_step(double* step_out, double* grad_out);
    double dist_local_fraction() const { return tp_.local_work_fraction(); }
    int dist_top_columns() const { return tp_.n_top_columns(); }

    // parity / debug exports
    int get_residual(double* r_out);
    int get_jacobian_blocks(double* jc_out, double* jl_out);
    int get_schur(double* S_out, double* gred_out);  // reference camera-side order, dense
    // Marginal camera covariances: the 9 x 9 camera blocks of (H + lambda I)^-1 -- by the Schur-complement identity exactly
    // the diagonal blocks of S^-1, S the reduced camera matrix the LAST solve_augmented factorised (variant 0 only: at that
    // solve's point, lambda and Jacobi scaling, plus its ladder regularisation if one was needed, apexgpu_info[4]) -- by
    // selected inversion of the tile factor (SelectedInverse::blocks, tile_sinv.h; the reference computes the whole inverse densely,
    // cholesky.rs:240-256).  out[n_cam][9][9], caller's camera order, pose 6 then intrinsics 3 (get_schur's layout).
    // d_c = 6: the intrinsics rows of get_schur's matrix are lambda on the diagonal, so theirs are 1 / lambda, no cross terms.
    // kInvalidState: no valid factor (no direct solve yet, a PCG / matrix-free solve or an export since), several ranks.
    int camera_covariance(double* out);
    // Marginal landmark covariances: the 3 x 3 landmark blocks of the inverse of the same matrix camera_covariance describes,
    //     Sigma_ll = V_l^-1 + sum_{i,j in obs(l)} U_i^T Z_{c(i) c(j)} U_j,   U_i = W_il V_l^-1   (Schur-complement identity)
    // with Z = S^-1 on the factor's tile pattern (reused when a camera_covariance call computed it for this factor, else the
    // selected inversion runs first), the landmark records and the cameras of the parameter set the factor was linearised at
    // (factor_lin_; cov_kernels.hip).  out[n_pt][3][3], caller's landmark order, symmetric bit for bit.  kInvalidState where
    // camera_covariance refuses, and when the factor's linearisation is gone (set_parameters or new scaling since the solve).
    int landmark_covariance(double* out);
    // [0] device bytes of the landmark pass, [1] observation pairs sum k (k + 1) / 2, [2] 1 if the last call recomputed Z,
    // [3] ms of the landmark kernels alone in the last call ("covariance_timing" on, else 0)
    void landmark_covariance_stats(double out[4]) const { out[0] = (double)lc_.bytes; out[1] = (double)lc_.pairs; out[2] = lc_.recomputed ? 1.0 : 0.0; out[3] = lc_.ms; }
    int get_landmark_blocks(double* hinv_out, double* gl_out);
    // H = J^T J of the corrected Jacobian at the current parameters as a full symmetric CSC matrix in the global column
    // order (what SparseSchurComplementSolver::get_hessian caches, explicit_schur.rs:1146-1160, 1236-1238).  Two-call
    // pattern: with colptr == NULL only *nnz_out is set.
    int get_hessian_csc(int64_t* nnz_out, int64_t* colptr, int64_t* rowidx, double* values);
    int schur_matvec(double lambda, const double* x_in, double* y_explicit, double* y_implicit);
    int64_t tile_count() const { return tp_.n_slots(); }
    int n_tile_rows() const { return nt_; }
    double last_reg() const { return last_reg_; }
    int last_pcg_iters() const { return last_pcg_iters_; }
    void enable_graphs(bool on) { use_graphs_ = on; TileBackend::enable_graphs(on); }   // (set_structure hands use_graphs_ to the plan again)
    int debug_occupy_cus(int n_cus, int micros) { return check_hip(tp_.debug_occupy_cus(n_cus, micros), "debug_occupy_cus"); }
    // before set_structure: the handle will only run the matrix-free variant (2, IterativeSchurSolver).  S is never formed, so
    // neither is its tile structure beyond the diagonal blocks the Schur-Jacobi preconditioner needs, nor the pair list: the
    // set-up and the LM iteration no longer depend on the fill of S (a photo collection whose S is dense: tools/structure_sweep.py)
    void set_matrix_free_only(bool on) { matrix_free_only_opt_ = on; }
    // Automatic variant selection (round 5; the LM dispatch of levenberg_marquardt.rs:1039-1082 never fails on the fill of S,
    // so a drop-in backend may not either): when the tile plan of S is refused at set_structure -- its update list beyond
    // TilePlan's limit, or (single rank) its tiles beyond the free HBM -- the handle is built matrix-free only by itself and
    // variants 0 / 1 are answered by the matrix-free PCG (IterativeSchurSolver semantics, implicit_schur.rs:835-946): variant 0
    // at that solver's own defaults (500 iterations, 1e-9: implicit_schur.rs:94-95), variant 1 at the caller's cg parameters.
    // "auto_variant" 0 restores the refusal.  variant_used() / variant_reason() say what happened (apexgpu_variant_info).
    void set_device_pair_recs(bool on) { device_pair_recs_ = on; }   // before set_structure ("device_pair_list")
    int get_pair_records(uint32_t* recs4_out, int64_t cap_slots);     // tests: the pair records as they sit on the device
    void set_auto_variant(bool on) { auto_variant_ = on; }
    void set_variant_cost_permille(int permille) { variant_cost_permille_ = permille < 0 ? 0 : permille; }   // before set_structure (see choose_and_build_plan)
    // [0] predicted ms per solve of the direct path (tile Cholesky + sweeps; 0: never evaluated -- "matrix_free_only"), [1] of the
    // matrix-free PCG at IterativeSchurSolver's cap, [2] what set_structure chose: 0 direct, 1 matrix-free by predicted cost,
    // 2 matrix-free because the plan was refused (size / memory), 3 matrix-free by the caller's option, [3] the cap behind [1]
    void variant_costs(double out[4]) const { out[0] = pred_direct_ms_; out[1] = pred_mf_ms_; out[2] = variant_choice_; out[3] = 500.0; }
    void set_max_tile_updates(int64_t n) { tp_.set_max_updates(n); }   // tests: force the refusal on a small problem
    int variant_used(int asked) const { return (auto_fallback_ && asked != 2) ? 2 : asked; }
    bool auto_fallback() const { return auto_fallback_; }
    const std::string& variant_reason() const { return fallback_reason_; }
    void set_schur_form(int v) { rows_form_ = v == 4 ? 4 : 3; }   // 4 queued layout (default; nine-column cameras), 3 one running block per wave
    bool has_structure() const { return have_structure_; }
    void set_hubs_last(bool on) { hubs_last_ = on; }
    int n_hubs() const { return n_hubs_; }
    void set_dist_factor(bool on) { dist_factor_ = on; }   // before set_structure
    void set_tree_sharding(bool on) { tree_sharding_ = on; }  // before set_structure
    void set_dist_selftest(int world) { dist_selftest_ = world; }  // before set_structure; single rank only
    int owned_landmarks(uint8_t* mask) const;
    bool tree_sharded() const { return tree_shard_; }
    double schur_scatter_pairs() const { return (double)n_pairs_; }
    double pair_blocks() const { return (double)n_pair_blocks_; }
    double pair_slots() const { return (double)n_pair_slots_; }
    // the form that RUNS (4 = the queued layout: nine-column cameras)
    int schur_form() const { return (rows_form_ == 4 && !pair_queued_) ? 3 : rows_form_; }
    const double* setup_seconds() const { return setup_s_; }
    double touched_tiles() const { return (double)n_present_; }
    double local_obs() const { return (double)o_orig_h_.size(); }

    // multi-GPU (one process per GPU; landmarks sharded, S and g_red all-reduced over RCCL)
    int comm_init(int world, int rank, const void* unique_id128);          // RCCL over xGMI (production)
    int comm_init_shm(int world, int rank, const char* name);              // host shared memory (bring-up / tests, comm.h)
    int set_shard(int rank, int world);  // without RCCL: assemble only this rank's landmark range

    int dc() const { return dc_; }
    int64_t cam_dof_internal() const { return n_c_; }

   private:
    // the direct solve's hooks (tile_backend.h)
    int rebuild_system(double lambda, double reg) override { return assemble(lambda, reg, true); }
    int factor_now(int* failed_at, bool defer_flags) override;
    int enqueue_sweeps() override;
    int finish_step(double* step_out, double* grad_out) override;
    int recover_factor(double lambda, int failed, bool gave_up) override;
    const int* own_flag() const override { return flags_; }
    int own_flag_raised() override { return fail(kSingularMatrix, "Landmark block is singular"); }
    void keep_factor() override;
    int enqueue_step_stats() override;
    int enqueue_trial_point(double* sumsq_out) override;
    int enqueue_retract(int from, double sign, int to) override { retract_sets(from, sign, to, n_pt_); return kOk; }
    // BaScalars::step, the camera and the landmark half of the step's sums, and trial_sumsq behind them -- read here only
    double* step_sums(int* n) override { *n = 6; return scal_.get()->step; }
    StepAnswers answers_from_sums(const double* h) const override { return {sqrt(h[0] + h[3]), sqrt(h[1] + h[4]), 0.5 * (h[2] + h[5]), h[6]}; }
    void params_moved() override { orec_fresh_ = false; }
    void retract_sets(int from, double sign, int to, int64_t n_pt);
    void voided_by(Change why);   // the one place a setter's change voids cached state (solver.hip)
    BAView view(int which) const;
    TileMap tilemap() const;
    // for_factor: the result feeds tp_.factor() (a distributed plan then leaves the top tiles to the factorisation's
    // own exchange); otherwise S is complete on every rank (PCG, exports, the ladder's diagonal read)
    int assemble(double lambda, double diag_extra, bool for_factor = false);
    int assemble_local(double lambda, double diag_extra, bool for_factor = false);
    int assemble_finish();
    int assemble_implicit(double lambda);
    int implicit_pcg_solve(double lambda, int max_iter, double tol);
    int implicit_matvec(const double* x, double lam_local, double* y, bool reduce);
    // the prior add-ons (ba_prior_kernels.h), each enqueued behind the kernel it extends and only when a set is non-empty
    bool have_priors() const { return pose_pri_.n > 0 || intr_pri_.n > 0; }
    BaPriorView prior_view() const;
    void enqueue_prior_eval(int which, bool cost_only);            // -> pri_diag_, pri_g_ (unless cost_only), pri_cost_ of parameter set `which`
    void enqueue_prior_cost(int which, double* sumsq);             // *sumsq += the prior rows' squares at set `which`
    int column_norms_sq_device();   // -> n2 in cam_scale_.dev / pt_scale_.dev (camera part all-reduced over the shards)
    int factor_with_ladder(double lambda);
    int ladder(double lambda);
    int pcg_solve();
    // the Dog-Leg hooks (tile_backend.h)
    int dogleg_refusal() override;                 // no parameters, a matrix-free handle, several ranks
    int dogleg_segments(DlSegment out[2]) override;
    void enqueue_jv_gram(const double* const a[2], const double* const b[2], double* out3) override;
    int solve_for_dogleg(double mu) override;      // solve_augmented(mu, 0) without the ladder, finish_step in dl_mode_
    void dogleg_trial_begins() override { trial_pts_written_ = false; }   // (the retraction writes all of the blended step's trial point)
    void stage_begin(int st);
    void stage_end(int st);
    // The steps of set_structure in the order it runs them (solver.hip).  Setup is the state of one call, its comments say
    // which thread owns what; a step that runs on the uploader thread writes its error text to `err`, never to err_.
    struct Setup;
    void device_thread_body(Setup& su);
    hipError_t device_ready(const Setup& su);
    int validate_indices(Setup& su);
    void choose_and_build_plan(Setup& su);
    void planner_body(Setup& su);
    int adopt_host_structure(Setup& su);
    void uploader_body(Setup& su);
    int upload_observation_lists(Setup& su, std::string* err);
    void build_column_maps(const Setup& su);
    int upload_fixed_masks(const Setup& su, std::string* err);
    int alloc_work_arrays(std::string* err);
    int upload_pair_lists(Setup& su, const PairDeviceTables& dtab, bool recs_on_device);
    void hand_lists_to_free_thread(Setup& su);

    // sizes
    int64_t n_cam_, n_pt_, n_obs_;
    int mode_, dc_;
    int64_t n_c_ = 0, n_c_pad_ = 0;
    int nt_ = 0;
    double huber_delta_ = 1.0;
    PgLoss loss_;
    bool loss_set_ = false;   // set_loss has replaced huber_delta_ (until the next set_structure)
    // what the launchers of the linearising kernels take: the loss of the general instantiations, or NULL where the
    // huber_delta kernels compute it (no set_loss; no loss, L2 and Huber given through set_loss: view())
    const PgLoss* general_loss() const {
        return loss_set_ && loss_.kind != kLossNone && loss_.kind != kLossL2 && loss_.kind != kLossHuber ? &loss_ : nullptr;
    }
    bool have_structure_ = false, have_params_ = false;
    double last_reg_ = 0.0;
    int last_pcg_iters_ = 0;
    int cg_max_iter_ = 200;   // SparseSchurComplementSolver::new (explicit_schur.rs:211-212)
    double cg_tol_ = 1e-6;
    int64_t n_pairs_ = 0, n_present_ = 0;
    // shard
    RankExchange ranks_;        // rank, world, the communicator and every collective (rank_exchange.h)
    int pad_rank_ = 0;          // rank that writes the identity on the padding rows of the last tile (assemble_local)
    int64_t lm_lo_ = 0, lm_hi_ = 0;  // landmark range owned by this rank
    using MakeComm = std::function<std::unique_ptr<Communicator>(std::string* err)>;
    int adopt_comm(int world, int rank, const MakeComm& make);   // what comm_init and comm_init_shm share

    // host copies
    std::vector<int> o_orig_h_;
    std::thread free_thread_;   // unmaps the set-up's host lists off the caller's path

    // device (stream_ and tp_ are TileBackend's: ~Solver joins free_thread_ and synchronises the stream, the buffers below are freed, then the plan, the stream last)
    // host -> device copies of caller (pageable) memory through two pinned chunks: the DMA of one overlaps the memcpy into the other
    int upload_staged(void* dst_dev, const void* src_host, size_t bytes);
    PinnedBuffer<char> pin_[2];
    hipEvent_t pin_ev_[2] = {nullptr, nullptr};
    bool pin_busy_[2] = {false, false};   // pin_ev_[b] has been recorded behind a DMA out of pin_[b] and not waited for yet
    DeviceBuffer<double> poses_[2], intr_[2], pts_[2];
    DeviceBuffer<double> camp_[2];  // prepared cameras of the two parameter sets
    DeviceBuffer<PairTask> ptasks_;     // rows_form_ 3: the sorted camera-pair list (schur_pairs.h)
    DeviceBuffer<PairChunk> pchunks_;
    DeviceBuffer<PairBlock> pblocks_;
    DeviceBuffer<PairRec> precs_;
    DeviceBuffer<PairQDesc> pqdesc_;    // rows_form_ 4 (and d_c = 9): the queued layout's descriptors, else null
    DeviceBuffer<uint8_t> o_slot_, wg_cam_n_;   // camera staging lists of the landmark-major kernels (BAView::o_slot)
    DeviceBuffer<uint32_t> wg_cam_list_;
    bool matrix_free_only_opt_ = false;   // the caller's option ("matrix_free_only")
    bool matrix_free_only_ = false;       // the effective state of the structure that is built: the option, or the automatic selection
    bool trial_pts_written_ = false;   // the back-substitution of this solve has written the trial points (enqueue_trial_point skips them)
    bool device_pair_recs_ = true;   // queued layout: the pair records are written by the device (k_build_pair_recs_q), not built on the host and copied
    bool auto_variant_ = true, auto_fallback_ = false;   // see set_auto_variant
    int variant_cost_permille_ = 1000, variant_choice_ = 0;
    double pred_direct_ms_ = 0.0, pred_mf_ms_ = 0.0;
    std::string fallback_reason_;
    // the parameter set (0 / 1) whose linearisation the held factor is of, -1 when it can no longer be known; and whether Jacobi
    // scaling was on for it (the scale vectors are kept until new scaling overwrites them)
    int factor_lin_ = -1;
    bool factor_scaled_ = false;
    // landmark covariance pass (landmark_covariance): built on the first call by lc_setup, released by set_structure
    struct LandmarkCov {
        DeviceBuffer<int> lists, err;   // [small | large] landmark lists (landmark_cov_lists.h), error word
        DeviceBuffer<double> out;       // [n_pt][9], internal order
        int n_small = 0, n_large = 0;
        int64_t pairs = 0;
        size_t bytes = 0;
        bool recomputed = false;        // the last call recomputed Z
        double ms = 0.0;                // ... and took this long in the landmark kernels ("covariance_timing" on, else 0)
        void release();
    };
    int lc_setup();
    LandmarkCov lc_;
    bool orec_fresh_ = false;   // orec_ holds the records of the current parameters' last linearisation
    const double* backsub_records() const { return orec_fresh_ ? orec_ : nullptr; }   // the projection records of THIS linearisation
    DeviceBuffer<double> orec_;   // [local observations][4] projection records written by k_landmark_reduce (pair kernel, record form)
    int n_ptasks_ = 0;
    int64_t n_pair_blocks_ = 0, n_pair_slots_ = 0;
    bool pair_queued_ = false;       // what build_pair_lists arrived at (PairLists::queued)
    int rows_form_ = 4;              // 4 (default): the sorted pair list in the QUEUED layout (every lane group owns a block, no fold:
                                     // schur_pairs.h); 3: the same list reduced over the lanes of a wave (k_schur_pairs_r: every block
                                     // S(ci, cj) stored once by one wave, no atomics, no LDS accumulators: what six-column cameras
                                     // run).  Select before set_structure.  (Rounds 1-3 also carried a global-atomics form, 135 ms,
                                     // and two LDS row forms, 9.7 / 6.0 ms: deleted in rounds 4 and 6.)
    DeviceBuffer<uint32_t> o_cam_, o_pt_, co_pt_;
    DeviceBuffer<double> o_uv_, co_uv_;   // [local observations][2]: BAView reads them as double2
    DeviceBuffer<int> co_rank_;
    DeviceBuffer<int> o_orig_, pt_ptr_, cam_ptr_, cam_obs_;
    DeviceBuffer<uint8_t> fix_pose_, fix_intr_, fix_pt_;
    DeviceBuffer<double> g_c_, g_red_, dcam_, hinv_, g_l_, dl_;
    DeviceBuffer<BaScalars> scal_;         // scalar outputs, by field: a device address, never read through on the host (the reduction scratch partial_ is TileBackend's)
    DeviceBuffer<int> flags_;              // [0] landmark inversion error
    std::vector<int> cmap_, cinv_;   // external camera -> internal camera and back
    bool hubs_last_ = true;     // order cameras covisible with > max(16, 10 sqrt(n_cam)) others last (ba_structure.h)
    int n_hubs_ = 0, n_border_tiles_ = 1;
    bool dist_factor_ = true;   // world > 1: factorise the elimination tree's subtrees on their owner ranks (tile_plan.h)
    bool tree_sharding_ = true; // ... and give every landmark to the rank whose columns it touches (set_structure)
    bool tree_shard_ = false;   // what set_structure arrived at
    int dist_selftest_ = 0;
    std::vector<int> lmap_;     // external landmark -> internal landmark (identity unless tree sharded)
    // The caller's global columns against the internal order (column_map.h), built by set_structure: the camera side (n_c_ entries;
    // six-column cameras leave their intrinsic columns untouched) and the landmarks (3 n_pt).  Every export scatters ALL 3 n_pt
    // landmark entries, a sharded rank's too.  Invariant: the entries of dl_ / g_l_ / hinv_ (and lmu_) of landmarks this rank does
    // not own, outside [lm_lo_, lm_hi_), are zero -- alloc_work_arrays zeroed them and nothing else writes them: the landmark-major
    // kernels run over the rank's own workgroups only and there is no collective over these buffers.  Whatever writes them whole
    // (an in-place all-gather, a debug import) breaks what export_step, step_stats and retract read.
    ColumnMap cam_map_, pt_map_;
    DeviceBuffer<uint8_t> lam_mask_;  // tree sharding: cameras whose diagonal block gets lambda on this rank
    DeviceBuffer<double> tile_work_;   // 6 n_c_pad: what tp_.pcg asks for (tile_plan.h; tp_.solve / solve_phase: 2 n_pad); ladder() reads the diagonal into it
    // matrix-free variant: the {pt, u_l} records and the scaled x of the operator (implicit_matvec); the loop and its preconditioner
    DeviceBuffer<double> lmu_, mf_xs_;
    SchurJacobiPcg sj_pcg_;
    // PriorFactor blocks on the cameras: each set sorted by internal camera (stable) with a CSR over the cameras; the vectors of
    // the last evaluation -- diag(P) and P's gradient over the camera columns [n_c_pad], the cost per camera [n_cam]
    struct PriorSet {
        int n = 0;
        DeviceBuffer<int> ptr, slot, cam;
        DeviceBuffer<double> data;
    };
    PriorSet pose_pri_, intr_pri_;
    DeviceBuffer<double> pri_diag_, pri_g_, pri_cost_, pri_res_;
    JacobiScaling cam_scale_, pt_scale_;   // Jacobi scaling, internal order ([n_c_pad] with 1 on the padding, [3 n_pt]); on: TileBackend::scaled_
    bool use_graphs_ = true;
    double setup_s_[6] = {0, 0, 0, 0, 0, 0};  // set_structure by phase: order + tile structure, landmark / camera lists, tile plan, Schur lists, uploads, total
};

}  // namespace apex
