// pg_solver.h -- host side of the MI355X pose-graph backend (BASELINE.json configs[1]): SE3, SE2 and SO3 vertices.
//
// Mirrors SparseCholeskySolver (src/linalg/sparse/cholesky.rs:159-230) driven by the LM loop
// (src/optimizer/levenberg_marquardt.rs:823-1031) on a problem of BetweenFactor<SE3> blocks
// (src/factors/between_factor.rs:268-322) as bin/pose_graph_g2o.rs:748-830 builds it:
// H = J^T J is assembled block-sparse (6x6 blocks) straight from the edges into 144x144 tiles,
// H + lambda I is factorised by the level-scheduled tile Cholesky of TilePlan -- no Schur complement.
//
// One class, three manifolds.  The orchestration (speculative factor, one wait per iteration, eager step evaluation,
// scaling, covariance, exports) does not care what a vertex is: it sees dof_ tangent columns and amb_ stored doubles per
// vertex, kNB / dof_ vertices per tile.  Only prepare / assemble / priors / cost / retract / exports differ, and the
// launchers of pg_kernels.h take manifold_ for that: the same kernels instantiated for Se3Manifold (6, 7), Se2Manifold
// (3, 3) or So3Manifold (3, 4), and two assemblies -- the 3-DOF manifolds SE2 and SO3 (rotation averaging,
// BetweenFactor<SO3>: between_factor.rs:13,55) always the row-owned assembly over the incident-edge lists of pg2_lists.h, SE3
// the atomic edge scatter by default and the row-owned assembly (bit-reproducible runs) under the option
// "row_owned_assembly".  Row-owned is a property of the handle (row_owned_), fixed by set_structure: the lists, the sorted
// priors and their slots live with the structure of row-owned handles only.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <string>
#include <vector>

#include "pg_kernels.h"
#include "tile_backend.h"

namespace apex {

enum PgStage { kPgAssemble = 0, kPgFactor, kPgTriSolve, kPgStats, kPgRetract, kPgCost, kPgNumStages };

class PoseGraphSolver : public TileBackend {
   public:
    PoseGraphSolver(int64_t n_v, int64_t n_e, int device, int manifold = kManifoldSE3);
    ~PoseGraphSolver() override;

    int set_structure(const uint32_t* e_from, const uint32_t* e_to, const double* meas7, const int64_t* pose_col,
                      const uint8_t* fix6, double huber_delta);
    int set_params(const double* poses7);
    int set_priors(int64_t n, const uint32_t* vertex, const double* data7, const double* huber_delta);   // PriorFactor blocks
    // The loss of every BetweenFactor block (pose_graph_g2o.rs:413-436; pg_loss.hpp), in place of set_structure's huber_delta.
    // Priors keep their per-block Huber delta.  Drops a pending step and the Dog-Leg cache like set_priors.
    int set_loss(int kind, double p0, double p1);
    void get_loss(int* kind, double out2[2]) const;
    // Edge information matrices: info [n_e][dof * dof] row-major, the caller's edge order; NULL: none.  Every
    // matrix is checked on the host (finite, symmetric to 1e-12 max|Omega|, positive definite) before anything changes; the
    // upper triangle is what is stored.  Drops a pending step and the Dog-Leg cache like set_loss; set_structure clears it.
    int set_information(const double* info);
    int get_information(int* present, double* info_out) const;   // info_out [n_e][dof * dof], full and symmetric; may be NULL
    int get_prior_residual(double* r7_out);
    int get_params(double* poses7);

    int cost(double* out) override;
    int solve_augmented(double lambda, int variant, double* step_out, double* grad_out) override;
    int parameter_norm(double* out) override;
    int lm_optimize(LmConfig* cfg, LmResult* res, LmIterRecord* hist, int hist_cap);
    // Gauss-Newton and Dog-Leg (tr_loop.h).  dogleg_step is TileBackend's; what this solver puts in are the hooks below: one
    // segment (g_, d_), the Gram pass over the edges (k_pg_jv_gram) and solve_damped as the fresh solve.
    int gn_optimize(GnConfig* cfg, LmResult* res, LmIterRecord* hist, int hist_cap);
    int dogleg_optimize(DlConfig* cfg, LmResult* res, DlIterRecord* hist, int hist_cap);
    // parity export: {|J a|^2, (J a).(J b), |J b|^2} at the current parameters; a, b in the caller's column order, as given
    int jv_gram(const double* a, const double* b, double out3[3]);
    // Jacobi column scaling (optimizer/mod.rs:749-763), same contract as Solver's
    int column_norms(double* norms_out);
    int set_column_scaling(const double* scaling);
    int set_jacobi_scaling(bool on) override;

    // parity / debug exports (caller's edge and column order)
    int get_residual(double* r_out);
    int get_jacobian_blocks(double* j_out);
    int get_hessian(double lambda, double* H_out, double* g_out);  // dense J^T J + lambda I, J^T r
    // Marginal covariances (SparseCholeskySolver::compute_covariance_matrix + extract_variable_covariances,
    // cholesky.rs:240-256, core/problem.rs:1128-1147): the 6 x 6 diagonal blocks of the inverse of the matrix the LAST
    // solve_augmented factorised -- J^T J + lambda I at that solve's point and lambda, in the scaled variables when Jacobi
    // scaling was on (what get_hessian(lambda) returns at the same point) -- by selected inversion of the tile factor
    // (SelectedInverse::blocks, tile_sinv.h).  out[n_v][6][6], caller's vertex order, columns as get_hessian's.  kInvalidState when
    // no valid factor is held (no solve yet, or an export / assembly since).
    int covariance(double* out);

    // "row_owned_assembly": read by the next set_structure.  false on a manifold that has the row-owned assembly only.
    bool set_row_owned_option(bool on) {
        if (!on && pg_row_owned(manifold_)) return false;
        opt_row_owned_ = on;
        return true;
    }
    bool row_owned() const { return row_owned_; }

    int64_t n_vertices() const { return n_v_; }
    int manifold() const { return manifold_; }
    int dof() const { return dof_; }           // tangent columns per vertex: 6 | 3 | 3
    int ambient() const { return amb_; }       // stored doubles per vertex / measurement / prior: 7 | 3 | 4
    int n_tile_rows() const { return tp_.nt(); }
    int64_t tile_count() const { return tp_.n_slots(); }
    int64_t touched_tiles() const { return tp_.n_touched_slots(); }

   private:
    // the direct solve's hooks (tile_backend.h)
    int rebuild_system(double lambda, double reg) override;
    int factor_now(int* failed, bool defer_flags) override;
    int enqueue_sweeps() override;
    int finish_step(double* step_out, double* grad_out) override;
    int recover_factor(double lambda, int failed, bool gave_up) override;
    PGView view(int which) const;
    int enqueue_step_stats() override;
    int enqueue_trial_point(double* sumsq_out) override;
    int enqueue_retract(int from, double sign, int to) override;   // retraction + the prepared poses of the result
    // SO3: a rejected trial step restores the parameters bit for bit (tile_backend.h).  SE3 and SE2 keep the reference's
    // apply_negative_parameter_step, trial (+) (-step), and the bits their tests pin.
    bool keeps_current_on_discard() const override { return manifold_ == kManifoldSO3; }
    // scal_: [1..3] the step's sums, [4] the trial point's sum of squares -- read here only
    double* step_sums(int* n) override { *n = 3; return scal_ + 1; }
    StepAnswers answers_from_sums(const double* h) const override { return {sqrt(h[0]), sqrt(h[1]), 0.5 * h[2], h[3]}; }
    void voided_by(Change why);   // the one place a setter's change voids cached state (pg_solver.hip)
    int assemble(double lambda);
    int solve_damped(double lambda, double* step_out, double* grad_out);   // solve_augmented behind its checks; the fresh Dog-Leg solve
    // the Dog-Leg hooks (tile_backend.h)
    int dogleg_refusal() override { return have_params_ ? kOk : fail(kInvalidState, "Block structure not built or parameters not set"); }
    int dogleg_segments(DlSegment out[2]) override;
    void enqueue_jv_gram(const double* const a[2], const double* const b[2], double* out3) override;
    int solve_for_dogleg(double mu) override { return solve_damped(mu, nullptr, nullptr); }

    int64_t n_v_, n_e_;
    int manifold_, dof_, amb_, stride_, prior_stride_, vpt_;   // vpt_: vertices per tile = kNB / dof_
    int64_t n_ = 0, n_pad_ = 0;
    double huber_delta_ = 0.0;
    bool loss_set_ = false;   // set_loss has replaced huber_delta_ (until the next set_structure)
    PgLoss loss_;             // kLossNone unless loss_set_
    bool have_structure_ = false, have_params_ = false;
    bool opt_row_owned_ = false;   // the option as last set; becomes row_owned_ at set_structure
    bool row_owned_;               // this structure is assembled row-owned: the manifold is (pg_row_owned) or the option was set
    std::vector<int> vmap_;  // caller's vertex -> internal vertex
    ColumnMap map_;          // ... and per tangent column: the caller's pose_col against the internal order (column_map.h)
    DeviceBuffer<double> poses_[2], posep_[2];
    DeviceBuffer<uint32_t> e_from_, e_to_;
    int n_prior_ = 0;
    DeviceBuffer<uint32_t> prior_v_;
    DeviceBuffer<int> inc_ptr_, prior_slot_;   // row-owned handles only: incident-edge CSR, the caller's index of each sorted prior
    DeviceBuffer<uint32_t> inc_edge_;
    DeviceBuffer<double> prior_data_;
    DeviceBuffer<double> prior_res_;   // staging of get_prior_residual
    DeviceBuffer<double> meas_;
    DeviceBuffer<double> info_;        // [n_e][InfoPack<dof>::kStride] packed upper triangles; empty: no information
    std::vector<double> info_host_;    // the same on the host (get_information)
    DeviceBuffer<uint8_t> fix_;
    DeviceBuffer<double> g_, rhs_, d_, work_, scal_;   // (the reduction scratch partial_ is TileBackend's)
    JacobiScaling scale_;              // Jacobi scaling, internal order, [n_pad] with 1 on the padding; on: TileBackend::scaled_
};

}  // namespace apex
