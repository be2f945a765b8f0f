// dogleg_scalars.hpp -- the sixteen doubles of a Dog-Leg step by name: what the tail of TileBackend::dogleg_step leaves on the
// device and copies to the host with the solve's one wait.  The layout is the kernels' (dogleg_kernels.h): the dots and the Gram
// pass write three sums each, the combine its seven answers behind them, the blend and the cost kernel one sum each.  No HIP here.
#pragma once
#include <math.h>

#include "step_state.h"
#include "tr_loop.h"

namespace apex {

struct DoglegScalars {
    double sums[6];   // g.g, h.h, g.h (launch_dl_dots); g.Hg, g.Hh, h.Hh (the Gram pass) -- kept from the last fresh solve: the cache
    double alpha, beta, c_g, c_h, scaled_step_norm, predicted_reduction, step_type;   // launch_dl_combine's out7
    double step_sumsq;    // |step|^2, unscaled (launch_dl_blend reads c_g, c_h)
    double trial_sumsq;   // the sum of squared corrected residuals at the trial point
    double pad;
};
static_assert(sizeof(DoglegScalars) == 16 * sizeof(double), "DoglegScalars: sixteen doubles, no padding between them");

// |g_s|, |step|, -s.g - 1/2 s.Hs (dog_leg.rs:1046, 1222, 948-960) and the trial point's sum of squares
inline StepAnswers dogleg_answers(const DoglegScalars& s) { return {sqrt(s.sums[0]), sqrt(s.step_sumsq), s.predicted_reduction, s.trial_sumsq}; }

inline DoglegStepInfo dogleg_step_info(const DoglegScalars& s, bool reused) {
    return {sqrt(s.sums[0]), sqrt(s.step_sumsq), s.predicted_reduction, s.step_type, s.alpha, s.beta, s.scaled_step_norm, reused ? 1.0 : 0.0};
}

}  // namespace apex
