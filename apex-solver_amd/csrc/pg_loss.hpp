// pg_loss.hpp -- the robust loss family of the pose-graph front end and the corrector that turns rho(s) into a rescaled
// residual and Jacobian, as plain arithmetic shared by the host (apexgpu_loss_evaluate, tests/host_harness_loss.cpp) and the
// device (the general-loss instantiations of pg_kernels.hip).
//
// Reference semantics (file:line under the apex-solver tree), branch for branch and operation for operation:
//   LossFunction::evaluate(s) -> [rho, rho', rho'']   src/core/loss_functions.rs
//       L2 176-178, L1 238-249, Huber 364-380, Cauchy 497-507, Fair 587-606, Geman-McClure 676-686, Welsch 761-769,
//       Tukey biweight 850-868, Andrews wave 951-968, Ramsay Ea 1039-1054, trimmed mean 1134-1140, Lp norm 1209-1223,
//       Barron general 1318-1354, Student t 1447-1460; AdaptiveBarron is Barron (1569-1574)
//   the constants each new() precomputes and the parameters it refuses   loss_functions.rs:340-351, 472-484, 575-582, ...
//   Corrector::new                                    src/core/corrector.rs:143-181
// The reference is reproduced as coded, also where its rho' is not the derivative of its rho (Fair's 0.5 / (c + |x|); the
// rho'(0) = 1/2 of Welsch, Tukey, Andrews and Ramsay), with its s < f64::EPSILON fall-backs, its .max(f64::MIN) clamps
// (f64::MIN is -DBL_MAX: they only stop a NaN), its x.max(EPSILON) divisors and Barron's two special cases.
#pragma once
#include <float.h>
#include <math.h>

#ifndef APEX_LOSS_HD
#ifdef __HIPCC__
#define APEX_LOSS_HD __host__ __device__ inline
#else
#define APEX_LOSS_HD inline
#endif
#endif

namespace apex {

// (the APEXGPU_LOSS_* values of include/apexgpu.h)
enum PgLossKind : int {
    kLossNone = 0, kLossL2, kLossL1, kLossHuber, kLossCauchy, kLossFair, kLossGemanMcClure, kLossWelsch, kLossTukey,
    kLossAndrews, kLossRamsay, kLossTrimmedMean, kLossLpNorm, kLossBarron, kLossTDistribution, kLossKindCount
};

struct PgLoss {
    int kind = kLossNone;
    double p0 = 0.0, p1 = 0.0;    // scale | p | nu | Barron's alpha,  Barron's scale
    double scale = 0.0;           // the scale of the kinds that have one (Barron: p1)
    double scale2 = 0.0;          // scale * scale
    double inv_scale2 = 0.0;      // 1 / scale2: Cauchy's and Geman-McClure's c, Welsch's and Ramsay's inv_scale2
    double threshold = 0.0;       // Andrews: pi * scale
    double half_nu_plus_1 = 0.0;  // Student t: (nu + 1) / 2
};

constexpr double kLossEps = DBL_EPSILON;   // f64::EPSILON
constexpr double kLossF64Min = -DBL_MAX;   // f64::MIN
constexpr double kLossPi = 3.14159265358979323846;   // std::f64::consts::PI

// What each new() does: false where it returns InvalidInput (scale <= 0, p <= 0, nu <= 0) or the kind is unknown.
// Barron's alpha is unrestricted.  One deliberate deviation: the reference's `scale <= 0.0` lets a NaN parameter through
// (and then evaluates to NaN everywhere); here !(p > 0) refuses it, so a NaN never reaches a kernel.
inline bool pg_loss_make(int kind, double p0, double p1, PgLoss* out) {
    PgLoss l;
    l.kind = kind; l.p0 = p0; l.p1 = p1;
    switch (kind) {
        case kLossNone: case kLossL2: case kLossL1: break;
        case kLossLpNorm: if (!(p0 > 0.0)) return false; break;
        case kLossTDistribution:
            if (!(p0 > 0.0)) return false;
            l.half_nu_plus_1 = (p0 + 1.0) / 2.0;
            break;
        case kLossBarron:
            if (!(p1 > 0.0)) return false;
            l.scale = p1; l.scale2 = p1 * p1;
            break;
        case kLossHuber: case kLossCauchy: case kLossFair: case kLossGemanMcClure: case kLossWelsch: case kLossTukey:
        case kLossAndrews: case kLossRamsay: case kLossTrimmedMean:
            if (!(p0 > 0.0)) return false;
            l.scale = p0; l.scale2 = p0 * p0;
            l.inv_scale2 = 1.0 / l.scale2;
            l.threshold = kLossPi * p0;
            break;
        default: return false;
    }
    *out = l;
    return true;
}

// True where pg_loss_evaluate returns rho'' > 0 for no s >= 0, so that pg_corrector always takes its first arm (alpha = 0,
// residual_scaling = sqrt(rho')): the losses one scalar per residual block expresses, the only ones the bundle-adjustment
// kernels run.  Read off pg_loss_evaluate kind by kind: every rho'' there is minus a product of non-negative
// factors, 0, or the L2 fall-back, except
//   Andrews   (0.25 / scale) cos(x / scale) / x is positive for x < pi scale / 2, whatever the scale;
//   Lp norm   e0 e1 s^e2 with e0 = p / 2 > 0, e1 = e0 - 1: positive exactly when p > 2;
//   Barron    (alpha - 2) / (4 scale^2) inner^(alpha / 2 - 2) outside its two special cases: positive exactly when alpha > 2
//             (alpha within 1e-6 of 2 is the L2 special case, within 1e-6 of 0 the Cauchy one; a NaN alpha fails both tests
//             below and is refused with the rest).
inline bool pg_loss_first_arm_only(const PgLoss& l) {
    switch (l.kind) {
        case kLossAndrews: return false;
        case kLossLpNorm: return l.p0 <= 2.0;
        case kLossBarron: return fabs(l.p0 - 2.0) < 1e-6 || l.p0 < 2.0;
        default: return true;
    }
}

APEX_LOSS_HD void pg_loss_set(double rho[3], double a, double b, double c) { rho[0] = a; rho[1] = b; rho[2] = c; }

// rho = {rho(s), rho'(s), rho''(s)} at the squared norm s.  The kind is uniform over a launch: no divergence.
APEX_LOSS_HD void pg_loss_evaluate(const PgLoss& l, double s, double rho[3]) {
    switch (l.kind) {
        case kLossL1: {
            if (s < kLossEps) break;   // near zero: L2
            const double sqrt_s = sqrt(s);
            pg_loss_set(rho, 2.0 * sqrt_s, 1.0 / sqrt_s, -1.0 / (2.0 * s * sqrt_s));
            return;
        }
        case kLossHuber: {
            if (!(s > l.scale2)) break;
            const double r = sqrt(s);
            const double rho1 = fmax(l.scale / r, kLossF64Min);
            pg_loss_set(rho, 2.0 * l.scale * r - l.scale2, rho1, -rho1 / (2.0 * s));
            return;
        }
        case kLossCauchy: {
            const double sum = 1.0 + s * l.inv_scale2;
            const double inv = 1.0 / sum;
            pg_loss_set(rho, l.scale2 * log(sum) / 2.0, fmax(inv, kLossF64Min), -l.inv_scale2 * (inv * inv));
            return;
        }
        case kLossFair: {
            if (s < kLossEps) break;
            const double abs_x = fabs(sqrt(s));
            const double c_plus_x = l.scale + abs_x;
            pg_loss_set(rho, l.scale * l.scale * (abs_x / l.scale - log(1.0 + abs_x / l.scale)), 0.5 / c_plus_x,
                        -1.0 / (4.0 * s * c_plus_x * c_plus_x));
            return;
        }
        case kLossGemanMcClure: {
            const double denom = 1.0 + s * l.inv_scale2;
            const double inv = 1.0 / denom;
            const double inv2 = inv * inv;
            pg_loss_set(rho, s * inv, inv2, -2.0 * l.inv_scale2 * inv2 * inv);
            return;
        }
        case kLossWelsch: {
            const double exp_term = exp(-s * l.inv_scale2);
            pg_loss_set(rho, (l.scale2 / 2.0) * (1.0 - exp_term), 0.5 * exp_term, -0.5 * l.inv_scale2 * exp_term);
            return;
        }
        case kLossTukey: {
            const double x = sqrt(s);
            if (x > l.scale) { pg_loss_set(rho, l.scale2 / 6.0, 0.0, 0.0); return; }
            const double ratio = x / l.scale;
            const double ratio2 = ratio * ratio;
            const double om = 1.0 - ratio2;
            const double om_sq = om * om;
            pg_loss_set(rho, (l.scale2 / 6.0) * (1.0 - om * om_sq), 0.5 * om_sq, -(ratio / l.scale2) * om);
            return;
        }
        case kLossAndrews: {
            const double x = sqrt(s);
            if (x > l.threshold) { pg_loss_set(rho, 2.0 * l.scale2, 0.0, 0.0); return; }
            const double arg = x / l.scale;
            const double sin_val = sin(arg), cos_val = cos(arg);
            pg_loss_set(rho, l.scale2 * (1.0 - cos_val), 0.5 * sin_val, (0.25 / l.scale) * cos_val / fmax(x, kLossEps));
            return;
        }
        case kLossRamsay: {
            const double x = sqrt(s);
            const double ax = l.scale * x;
            const double exp_term = exp(-ax);
            pg_loss_set(rho, l.inv_scale2 * (1.0 - exp_term * (1.0 + ax)), 0.5 * exp_term,
                        -(l.scale / (4.0 * fmax(x, kLossEps))) * exp_term);
            return;
        }
        case kLossTrimmedMean: {
            if (s <= l.scale2) pg_loss_set(rho, s / 2.0, 0.5, 0.0);
            else pg_loss_set(rho, l.scale2 / 2.0, 0.0, 0.0);
            return;
        }
        case kLossLpNorm: {
            if (s < kLossEps) break;
            const double e0 = l.p0 / 2.0;
            const double e1 = e0 - 1.0;
            const double e2 = e1 - 1.0;
            pg_loss_set(rho, pow(s, e0), e0 * pow(s, e1), e0 * e1 * pow(s, e2));
            return;
        }
        case kLossBarron: {
            const double alpha = l.p0;
            if (fabs(alpha) < 1e-6) {   // Cauchy
                const double denom = 1.0 + s / l.scale2;
                const double inv = 1.0 / denom;
                pg_loss_set(rho, (l.scale2 / 2.0) * log(denom), fmax(inv, kLossF64Min), -inv * inv / l.scale2);
                return;
            }
            if (fabs(alpha - 2.0) < 1e-6) break;   // L2
            const double x = sqrt(s);
            const double normalized = x / l.scale;
            const double normalized2 = normalized * normalized;
            const double inner = fabs(alpha) / 2.0 * normalized2 + 1.0;
            const double power = pow(inner, alpha / 2.0);
            pg_loss_set(rho, (fabs(alpha) / l.scale2) * (power - 1.0), 0.5 * pow(inner, alpha / 2.0 - 1.0),
                        (alpha - 2.0) / (4.0 * l.scale2) * pow(inner, alpha / 2.0 - 2.0));
            return;
        }
        case kLossTDistribution: {
            const double inner = 1.0 + s / l.p0;
            const double denom = l.p0 + s;
            pg_loss_set(rho, l.half_nu_plus_1 * log(inner), l.half_nu_plus_1 / denom, -l.half_nu_plus_1 / (denom * denom));
            return;
        }
        default: break;
    }
    pg_loss_set(rho, s, 1.0, 0.0);   // L2, no loss, and the fall-backs above
}

// Corrector::new (corrector.rs:143-181).  First arm (s == 0 or rho'' <= 0): r~ = sqrt(rho') r, J~ = sqrt(rho') J.  Second arm:
// r~ = residual_scaling r, J~ = sqrt(rho') (J - alpha_sq_norm r r^T J).
struct PgCorrector {
    double sqrt_rho1, residual_scaling, alpha_sq_norm;
};

APEX_LOSS_HD PgCorrector pg_corrector(const double rho[3], double s) {
    const double sqrt_rho1 = sqrt(rho[1]);
    if (s == 0.0 || rho[2] <= 0.0) return PgCorrector{sqrt_rho1, sqrt_rho1, 0.0};
    const double d = fmax(1.0 + 2.0 * s * rho[2] / rho[1], 0.0);
    const double alpha = 1.0 - sqrt(d);
    return PgCorrector{sqrt_rho1, sqrt_rho1 / (1.0 - alpha), alpha / s};
}

APEX_LOSS_HD PgCorrector pg_loss_corrector(const PgLoss& l, double s) {
    double rho[3];
    pg_loss_evaluate(l, s, rho);
    return pg_corrector(rho, s);
}

}  // namespace apex
