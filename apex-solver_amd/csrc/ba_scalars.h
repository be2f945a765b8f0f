// ba_scalars.h -- the scalar outputs of the bundle-adjustment solver's reductions (Solver, solver.h): one device struct, every
// slot a field with one writer.
#pragma once
#include <stddef.h>

namespace apex {

struct BaScalars {
    double step[6];          // enqueue_step_stats: {g.g, d.d, the predicted reduction's sum} of the camera half, then of the landmark half
    double trial_sumsq;      // the trial point's sum of squares: TileBackend reads it as step_sums()[6], directly behind the six
    double cost_sumsq;       // cost()
    double param_sumsq[3];   // parameter_norm: poses, intrinsics, points
};
static_assert(offsetof(BaScalars, trial_sumsq) == offsetof(BaScalars, step) + 6 * sizeof(double),
              "step_sums() hands out step[0..5] with the trial point's slot behind them (tile_backend.hip)");

}  // namespace apex
