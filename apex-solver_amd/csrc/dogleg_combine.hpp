// dogleg_combine.hpp -- Powell's dog leg as plain arithmetic on seven scalars, shared by the host (tr_loop's test harness) and
// the device (k_dl_combine, dogleg_kernels.hip).
//
// Reference semantics (file:line under the apex-solver tree), everything in the SCALED variables (g = g_s, h = h_s, H = D J^T J D):
//   compute_cauchy_point_and_alpha   src/optimizer/dog_leg.rs:776-803   alpha = g.g / g.Hg when |g.Hg| > 1e-15, else 1; p_c = -alpha g
//   compute_dog_leg_step             dog_leg.rs:818-902                 |h| <= Delta: h; |p_c| >= Delta: (Delta / |g|)(-g);
//                                                                       else p_c + beta (h - p_c) with the two-formula beta
//   compute_predicted_reduction      dog_leg.rs:948-960                 -s.g - 1/2 s.Hs
// The reference works on the vectors; here every step is step = c_g (-g) + c_h h, so its norm, its products with g and with H
// are combinations of the six inner products g.g, h.h, g.h, g.Hg, g.Hh, h.Hh -- which is what lets a reused iteration
// (dog_leg.rs:969-1017: the cached g, h, p_c under a smaller radius, priced with the Hessian of the last solve) run without a
// single pass over the edges.
#pragma once
#include <math.h>

#ifndef APEX_DL_HD
#ifdef __HIPCC__
#define APEX_DL_HD __host__ __device__ inline
#else
#define APEX_DL_HD inline
#endif
#endif

namespace apex {

enum DoglegStepType : int { kStepGaussNewton = 0, kStepSteepestDescent = 1, kStepDogLeg = 2 };   // StepType of dog_leg.rs

struct DoglegSums {
    double gg, hh, gh;   // g.g, h.h, g.h
    double uu, uw, ww;   // g.Hg, g.Hh, h.Hh  (|Jg|^2, (Jg).(Jh), |Jh|^2 with the scaled J)
};

struct DoglegStep {
    double alpha, beta;           // beta: 0 unless the step is a dog leg
    double c_g, c_h;              // step = c_g (-g) + c_h h
    double step_norm;             // |step| in the scaled variables
    double predicted_reduction;   // c_g g.g - c_h g.h - 1/2 (c_g^2 g.Hg - 2 c_g c_h g.Hh + c_h^2 h.Hh)
    int type;                     // DoglegStepType
};

APEX_DL_HD DoglegStep dogleg_combine(const DoglegSums& s, double delta) {
    DoglegStep o;
    o.alpha = fabs(s.uu) > 1e-15 ? s.gg / s.uu : 1.0;
    o.beta = 0.0;
    const double gn_norm = sqrt(s.hh), sd_norm = sqrt(s.gg), cauchy_norm = fabs(o.alpha) * sd_norm;
    if (gn_norm <= delta) {
        o.type = kStepGaussNewton; o.c_g = 0.0; o.c_h = 1.0;
    } else if (cauchy_norm >= delta) {
        o.type = kStepSteepestDescent; o.c_g = delta / sd_norm; o.c_h = 0.0;
    } else {
        // v = h - p_c = h + alpha g:  a = v.v, b = p_c.v, c = |p_c|^2 - Delta^2
        const double a = s.hh + 2.0 * o.alpha * s.gh + o.alpha * o.alpha * s.gg;
        const double b = -o.alpha * s.gh - o.alpha * o.alpha * s.gg;
        const double c = cauchy_norm * cauchy_norm - delta * delta;
        const double d2 = b * b - a * c;
        double beta;
        if (d2 < 0.0) beta = 1.0;
        else if (fabs(a) < 1e-15) beta = 1.0;
        else {
            const double d = sqrt(d2);
            beta = b <= 0.0 ? (-b + d) / a : -c / (b + d);
        }
        beta = beta < 0.0 ? 0.0 : (beta > 1.0 ? 1.0 : beta);   // (f64::clamp)
        o.type = kStepDogLeg; o.beta = beta;
        o.c_g = o.alpha * (1.0 - beta); o.c_h = beta;   // p_c + beta (h - p_c)
    }
    const double n2 = o.c_g * o.c_g * s.gg - 2.0 * o.c_g * o.c_h * s.gh + o.c_h * o.c_h * s.hh;
    o.step_norm = sqrt(n2 > 0.0 ? n2 : 0.0);
    o.predicted_reduction = o.c_g * s.gg - o.c_h * s.gh - 0.5 * (o.c_g * o.c_g * s.uu - 2.0 * o.c_g * o.c_h * s.uw + o.c_h * o.c_h * s.ww);
    return o;
}

}  // namespace apex
