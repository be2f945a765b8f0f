// tr_loop.cpp -- see tr_loop.h
#include "tr_loop.h"

#include <math.h>
#include <string.h>

#include <algorithm>
#include <chrono>

namespace apex {

namespace {

using Clock = std::chrono::steady_clock;
double seconds_since(Clock::time_point t0) { return std::chrono::duration<double>(Clock::now() - t0).count(); }

// process_jacobian_generic (optimizer/mod.rs:749-763): the scaling is taken from the Jacobian of iteration 0 and lives in the
// optimizer for this optimize() only
struct ScalingGuard {
    LmBackend& b;
    bool on = false;
    int begin(bool want) {
        if (!want) return kOk;
        const int rc = b.set_jacobi_scaling(true);
        on = rc == kOk;
        return rc;
    }
    ~ScalingGuard() { if (on) b.set_jacobi_scaling(false); }
};

// compute_step_quality (optimizer/mod.rs:668-675)
double step_quality(double cur_cost, double new_cost, double pred) {
    const double actual = cur_cost - new_cost;
    return (fabs(pred) < 1e-15) ? (actual > 0.0 ? 1.0 : 0.0) : actual / pred;
}

}  // namespace

int run_gauss_newton(LmBackend& b, GnConfig* cfg, LmResult* res, LmIterRecord* hist, int hist_cap) {
    const auto t0 = Clock::now();
    double cur_cost = 0.0;
    int rc = b.cost(&cur_cost);  // initialize_optimization_state
    if (rc != kOk) return rc;
    memset(res, 0, sizeof *res);
    res->initial_cost = cur_cost;
    res->cost_evaluations = 1;
    ScalingGuard scaling{b};
    rc = scaling.begin(cfg->use_jacobi_scaling != 0);
    if (rc != kOk) return rc;
    int iteration = 0, status = kMaxIterationsReached;
    for (;;) {
        rc = b.solve_augmented(0.0, cfg->variant, nullptr, nullptr);  // solve_normal_equation (gauss_newton.rs:491-503)
        res->jacobian_evaluations++;
        if (rc != kOk) { status = kLinearSolveFailed; break; }
        double st[3];
        rc = b.step_stats(st);
        if (rc != kOk) return rc;
        const double gn = st[0], sn = st[1];
        const double cost_before = cur_cost;   // (:633)
        double new_cost = 0.0;
        rc = b.eval_step(&new_cost);  // apply_step_and_evaluate_cost (:529-556): the step is always kept
        if (rc != kOk) return rc;
        res->cost_evaluations++;
        cur_cost = new_cost;
        rc = b.commit_step();
        if (rc != kOk) return rc;
        res->successful_steps++;
        if (hist && iteration < hist_cap) {
            LmIterRecord& h = hist[iteration];
            h.cost = cur_cost; h.damping = 0.0; h.rho = 0.0; h.accepted = 1.0; h.gradient_norm = gn;
            h.step_norm = sn; h.predicted_reduction = st[2]; h.trial_cost = new_cost;
        }
        res->final_gradient_norm = gn;
        res->final_step_norm = sn;
        double pnorm = 0.0;
        rc = b.parameter_norm(&pnorm);
        if (rc != kOk) return rc;
        const int stt = check_convergence({iteration, cost_before, cur_cost, pnorm, sn, gn, seconds_since(t0), true, cfg->max_iterations,
                                           cfg->gradient_tolerance, cfg->parameter_tolerance, cfg->cost_tolerance, cfg->min_cost_threshold,
                                           cfg->timeout_s, false, 0.0, 0.0});   // (:683-700)
        ++iteration;
        if (stt >= 0) { status = stt; break; }
    }
    res->status = status;
    res->iterations = iteration;
    res->final_cost = cur_cost;
    res->elapsed_s = seconds_since(t0);
    return kOk;
}

int run_dogleg(TrBackend& b, DlConfig* cfg, LmResult* res, DlIterRecord* hist, int hist_cap) {
    const auto t0 = Clock::now();
    constexpr int kMaxCacheReuse = 5;   // MAX_CACHE_REUSE (dog_leg.rs:971)
    double radius = cfg->trust_region_radius, mu = cfg->mu;
    // the optimiser's reuse state (dog_leg.rs:733-739).  have_cache stands for the four cached_* options: set by a fresh solve,
    // cleared by a good or a moderate step.
    bool reuse_on_rejection = false, have_cache = false;
    int reuse_count = 0;
    double cur_cost = 0.0;
    int rc = b.cost(&cur_cost);
    if (rc != kOk) return rc;
    memset(res, 0, sizeof *res);
    res->initial_cost = cur_cost;
    res->cost_evaluations = 1;
    ScalingGuard scaling{b};
    rc = scaling.begin(cfg->use_jacobi_scaling != 0);
    if (rc != kOk) return rc;
    int iteration = 0, status = kMaxIterationsReached;
    for (;;) {
        res->jacobian_evaluations++;   // (the reference assembles every iteration, reused or not: :1184-1191)
        DoglegStepInfo si;
        const bool reused = reuse_on_rejection && cfg->enable_step_reuse && reuse_count < kMaxCacheReuse && have_cache;   // (:973-982)
        if (reused) {
            ++reuse_count;
            rc = b.dogleg_step(mu, radius, 1, &si);
            if (rc != kOk) return rc;
        } else {
            // the Gauss-Newton step with the adaptive mu (:1026-1039)
            bool solved = false;
            for (int attempts = 0; attempts < 10 && mu <= cfg->max_mu; ++attempts) {
                rc = b.dogleg_step(mu, radius, 0, &si);
                if (rc == kOk) { solved = true; break; }
                if (rc != kSingularMatrix && rc != kFactorizationFailed) break;   // (not a failed linear solve: raising mu will not mend it)
                mu = std::min(mu * cfg->mu_increase_factor, cfg->max_mu);
            }
            if (!solved) { status = kLinearSolveFailed; break; }
            have_cache = true;   // (:1078-1082)
        }
        const double gn = si.gradient_norm, sn = si.step_norm, pred = si.predicted_reduction;
        double new_cost = 0.0;
        rc = b.eval_step(&new_cost);  // evaluate_and_apply_step (:1092-1140)
        if (rc != kOk) return rc;
        res->cost_evaluations++;
        const double rho = step_quality(cur_cost, new_cost, pred);
        const bool accepted = rho > 1e-4;   // (:1118)
        // update_trust_region (:905-945)
        if (rho > cfg->good_step_quality) {
            radius = std::min(std::max(radius, 3.0 * sn), cfg->trust_region_max);
            mu = std::max(mu / (0.5 * cfg->mu_increase_factor), cfg->min_mu);
            reuse_on_rejection = false; have_cache = false; reuse_count = 0;
        } else if (rho < cfg->poor_step_quality) {
            radius = std::max(radius * cfg->trust_region_decrease_factor, cfg->trust_region_min);
            reuse_on_rejection = cfg->enable_step_reuse != 0;   // (also behind an ACCEPTED step with 1e-4 < rho < poor: the cache stays)
        } else {
            reuse_on_rejection = false; have_cache = false; reuse_count = 0;
        }
        double cost_reduction = 0.0;
        if (accepted) {
            cost_reduction = cur_cost - new_cost;
            cur_cost = new_cost;
            rc = b.commit_step();
            res->successful_steps++;
        } else {
            rc = b.discard_step();
            res->unsuccessful_steps++;
        }
        if (rc != kOk) return rc;
        if (hist && iteration < hist_cap) {
            DlIterRecord& h = hist[iteration];
            h.cost = cur_cost; h.radius = radius; h.mu = mu; h.rho = rho; h.accepted = accepted ? 1.0 : 0.0; h.gradient_norm = gn;
            h.step_norm = sn; h.predicted_reduction = pred; h.trial_cost = new_cost; h.step_type = si.step_type; h.beta = si.beta;
            h.reused = reused ? 1.0 : 0.0;
        }
        res->final_gradient_norm = gn;
        res->final_step_norm = sn;
        double pnorm = 0.0;
        rc = b.parameter_norm(&pnorm);
        if (rc != kOk) return rc;
        const double cost_before = accepted ? cur_cost + cost_reduction : cur_cost;   // (:1280-1284)
        const int stt = check_convergence({iteration, cost_before, cur_cost, pnorm, sn, gn, seconds_since(t0), accepted, cfg->max_iterations,
                                           cfg->gradient_tolerance, cfg->parameter_tolerance, cfg->cost_tolerance, cfg->min_cost_threshold,
                                           cfg->timeout_s, true, radius, cfg->trust_region_min});   // (:1286-1303)
        ++iteration;
        if (stt >= 0) { status = stt; break; }
    }
    cfg->trust_region_radius = radius; cfg->mu = mu;
    res->status = status;
    res->iterations = iteration;
    res->final_cost = cur_cost;
    res->elapsed_s = seconds_since(t0);
    return kOk;
}

}  // namespace apex
