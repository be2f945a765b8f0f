// tr_loop.h -- the Gauss-Newton and Dog-Leg loops, beside the Levenberg-Marquardt loop of lm_loop.h and over the same backend
// protocol: linearise + solve at the current point, statistics, trial point and its cost, keep or undo.
//
//   GaussNewton::optimize_with_mode   src/optimizer/gauss_newton.rs:559-720   (defaults :236-255)
//   DogLeg::optimize_with_mode        src/optimizer/dog_leg.rs:1143-1354      (defaults :353-399, state :725-745)
// Gauss-Newton needs nothing LmBackend does not have: it is solve_augmented(0) (solve_normal_equation) with every step kept.
// Dog-Leg needs one call more, dogleg_step; TrBackend adds it.  TileBackend (tile_backend.h) implements it once for both device
// backends: the pose-graph one (pg_solver.h) solves on its sparse Cholesky, the bundle-adjustment one (solver.h) on the Schur
// solver -- the reference hands a DogLeg configured with SparseSchurComplement a sparse Cholesky of the whole H + mu I
// (optimizer/mod.rs:681-693), which computes the same step.
#pragma once
#include "lm_loop.h"

namespace apex {

struct GnConfig {               // GaussNewtonConfig; fields the loop does not read (min_diagonal, max_condition_number) are not reproduced
    int max_iterations;         // 50
    double cost_tolerance;      // 1e-6
    double parameter_tolerance; // 1e-8
    double gradient_tolerance;  // 1e-10
    double min_cost_threshold;  // < 0: None
    double timeout_s;           // <= 0: None
    int variant;                // 0: the sparse Cholesky solver
    int use_jacobi_scaling;     // false (:247)
};

struct DlConfig {               // DogLegConfig; fields the loop does not read (trust_region_increase_factor -- the loop grows by the
                                // literal 3, dog_leg.rs:908 --, min_step_quality, min_relative_decrease, max_condition_number) are not reproduced
    int max_iterations;                    // 50
    double cost_tolerance;                 // 1e-6
    double parameter_tolerance;            // 1e-8
    double gradient_tolerance;             // 1e-10
    double trust_region_radius;            // 1e4; in/out
    double trust_region_min;               // 1e-12
    double trust_region_max;               // 1e12
    double trust_region_decrease_factor;   // 0.5
    double good_step_quality;              // 0.75
    double poor_step_quality;              // 0.25
    double mu;                             // initial_mu 1e-4; in/out
    double min_mu;                         // 1e-8
    double max_mu;                         // 1.0
    double mu_increase_factor;             // 10
    double min_cost_threshold;             // < 0: None
    double timeout_s;                      // <= 0: None
    int variant;                           // 0: the sparse Cholesky solver
    int use_jacobi_scaling;                // true (:378)
    int enable_step_reuse;                 // true (:388)
};

struct DlIterRecord {  // one row of the Dog-Leg history; radius and mu AFTER the iteration's update, like LmIterRecord::damping
    double cost, radius, mu, rho, accepted, gradient_norm, step_norm, predicted_reduction, trial_cost, step_type, beta, reused;
};

// what dogleg_step reports (the C ABI's out8)
struct DoglegStepInfo {
    double gradient_norm;         // |g_s|                                  (dog_leg.rs:1046, :986)
    double step_norm;             // |step|, UNSCALED: what apply_parameter_step returns (optimizer/mod.rs:330)
    double predicted_reduction;   // -s.g - 1/2 s.Hs in the scaled variables (:948-960)
    double step_type;             // DoglegStepType (dogleg_combine.hpp)
    double alpha, beta;
    double scaled_step_norm;      // |step_s|
    double reused;                // 1: built from the cache
};

class TrBackend : public LmBackend {
   public:
    // compute_optimization_step_generic (dog_leg.rs:963-1089) at radius, then the trial point and its cost, so that step_stats /
    // eval_step / commit_step / discard_step follow as after solve_augmented.
    //   reuse = 0: (H + mu I) h = -g at the current point, Cauchy point, dog leg; h, g and the products with H are cached.
    //              kSingularMatrix / kFactorizationFailed: the linear solve failed (the caller may raise mu).
    //   reuse = 1: the step from the CACHED h, g, p_c at the new radius, priced with the Hessian of the last solve -- no
    //              assembly, no factorisation, wherever the parameters are now.  kInvalidState without a cache.
    virtual int dogleg_step(double mu, double radius, int reuse, DoglegStepInfo* out) = 0;
};

// History rows of run_gauss_newton are LmIterRecord with damping = 0, rho = 0 (Gauss-Newton has no step quality), accepted = 1.
int run_gauss_newton(LmBackend& b, GnConfig* cfg, LmResult* res, LmIterRecord* hist, int hist_cap);
int run_dogleg(TrBackend& b, DlConfig* cfg, LmResult* res, DlIterRecord* hist, int hist_cap);

}  // namespace apex
