// step_state.h -- the state of the trial-step protocol the optimiser loops drive (lm_loop.h: solve_augmented, step_stats,
// eval_step, then commit_step or discard_step), as a plain value with its transitions.  No HIP here: TileBackend
// (tile_backend.h) does the device work around it, tests/host_harness_step_state.cpp walks it on the host.
#pragma once
#include <math.h>
#include <stdint.h>

#include "lm_loop.h"

namespace apex {

// compute_cost: 0.5 * norm_l2()^2 of the residual whose sum of squares is ss (optimizer/mod.rs:358-361), in that arithmetic
inline double cost_from_sumsq(double ss) {
    const double nrm = sqrt(ss);
    return 0.5 * nrm * nrm;
}

// what a solve can answer at its own host wait, so that step_stats / eval_step need no launch and no wait of their own
struct StepAnswers {
    double gradient_norm = 0.0;         // gradient.norm_l2()          (levenberg_marquardt.rs:746)
    double step_norm = 0.0;             // step.norm_l2()              (:890)
    double predicted_reduction = 0.0;   // compute_predicted_reduction (:721-727)
    double trial_sumsq = 0.0;           // sum of squared corrected residuals at the trial point
};

struct StepState {
    bool have_step = false, have_trial = false;   // a step at the current parameters is on the device; the other set holds current (+) step
    int cur = 0;               // index of the current parameter set (0/1); the other one is the trial set
    int64_t serial = 0, answers_serial = -1;   // the solves counted; == : `answers` are THIS solve's, its trial point is in place
    StepAnswers answers;
    const char* refusal = "";  // the text that goes with the last kInvalidState
    // a solve starts: its evaluation overwrites the trial set, so an earlier eval_step is void, and so are earlier answers
    void begin_solve() { have_step = have_trial = false; ++serial; }
    void step_computed() { have_step = true; }
    void post_answers(const StepAnswers& a) { answers = a; answers_serial = serial; }
    bool answered() const { return answers_serial == serial; }
    // set_params and its kin: parameters or system changed under the step.  invalidate_step: the step alone is stale (an assembly
    // over its system, new scaling, a failed solve); a trial point already written stays committable.
    void invalidate() { have_step = have_trial = false; }
    void invalidate_step() { have_step = false; }
    // step_stats / eval_step: kOk with *served the answers of this solve, or null: the caller computes them (eval_step: and
    // says trial_written).  Served to eval_step they mean the trial point is in place.
    Status ask_stats(const StepAnswers** served) { return ask(served, false); }
    Status ask_trial(const StepAnswers** served) { return ask(served, true); }
    void trial_written() { have_trial = true; }
    Status commit() {   // the trial set becomes the current one
        if (!have_trial) return refuse("no trial point");
        cur ^= 1;
        have_step = have_trial = false;
        return kOk;
    }
    Status begin_discard() { return have_trial ? kOk : refuse("no trial point"); }   // the caller moves the trial point back, waits ...
    Status finish_discard() { const Status rc = begin_discard(); if (rc == kOk) invalidate(); return rc; }
   private:
    Status refuse(const char* why) { refusal = why; return kInvalidState; }
    Status ask(const StepAnswers** served, bool trial) {
        if (!have_step) return refuse("no step computed");
        *served = answered() ? &answers : nullptr;
        if (trial && *served) have_trial = true;
        return kOk;
    }
};

}  // namespace apex
