// pg2_device.hpp -- per-edge SE2 pose-graph math behind the kernels of pg_kernels.hip, and Se2Manifold, the trait through
// which the manifold-generic kernels there reach it.
//
// APEX_HD (host+device) like pg_device.hpp, so tests/host_harness_se2.cpp runs the same code on the CPU.
//
// Reference semantics (file:line under the apex-solver tree):
//   SE2 = translation + unit complex, vector form [x, y, theta]   crates/apex-manifolds/src/se2.rs:27-63
//   inverse / compose / log / adjoint                             se2.rs:213-328
//   exp, right_jacobian, right_jacobian_inv                       se2.rs:468-534, 577-613
//   small-angle branches: theta^2 against SMALL_ANGLE_THRESHOLD   crates/apex-manifolds/src/lib.rs:61
//   LieGroup::between                                             lib.rs:401-419
//   BetweenFactor<SE2>::linearize                                 src/factors/between_factor.rs:268-322
//       r = Log((k1^-1 k0) * meas),  dr/dk0 = Jr^-1(r) Adj(meas^-1),
//       dr/dk1 = Jr^-1(r) (Adj(meas^-1) (-Adj((k1^-1 k0)^-1)))
//   PriorFactor on an SE2 variable                                src/factors/prior_factor.rs:96-108
//
// A pose travels prepared as p[4] = {x, y, re, im} (SE2::from_xy_angle: re = cos theta, im = sin theta); the parameter
// vector is v[3] = {x, y, theta}.  Tangents are [x, y, theta]; Jacobians are dense row-major 3 x 3 (their last row is
// (0, 0, +-1): the compiler folds the constants once everything is inlined).
#pragma once
#include <stddef.h>
#include <stdint.h>

#include <type_traits>

#include "pg_device.hpp"

namespace apex {

constexpr int kPose2Stride = 4;   // doubles per prepared SE2 pose / measurement
constexpr double kPi = 3.14159265358979323846;

// theta as SE2 -> DVector returns it (UnitComplex::angle = atan2(im, re), se2.rs:55-63): values already in (-pi, pi] are
// their own image and keep their bits
APEX_HD double se2_wrap_angle(double th) {
    if (th > -kPi && th <= kPi) return th;
    return atan2(sin(th), cos(th));
}
APEX_HD void se2_prepare(const double* __restrict__ v3, double* __restrict__ p4) {
    p4[0] = v3[0]; p4[1] = v3[1]; p4[2] = cos(v3[2]); p4[3] = sin(v3[2]);
}
APEX_HD double se2_angle(const double* p4) { return atan2(p4[3], p4[2]); }

APEX_HD void se2_inv(const double* __restrict__ a, double* __restrict__ o) {
    const double re = a[2], im = -a[3];
    o[0] = -(re * a[0] - im * a[1]);
    o[1] = -(im * a[0] + re * a[1]);
    o[2] = re; o[3] = im;
}
APEX_HD void se2_mul(const double* __restrict__ a, const double* __restrict__ b, double* __restrict__ o) {
    o[0] = (a[2] * b[0] - a[3] * b[1]) + a[0];
    o[1] = (a[3] * b[0] + a[2] * b[1]) + a[1];
    o[2] = a[2] * b[2] - a[3] * b[3];
    o[3] = a[2] * b[3] + a[3] * b[2];
}
// k1^-1 k0 written as a.between(b) = a^-1 b
APEX_HD void se2_between(const double* __restrict__ a, const double* __restrict__ b, double* __restrict__ o) {
    double ai[4];
    se2_inv(a, ai);
    se2_mul(ai, b, o);
}
APEX_HD void se2_adjoint(const double* __restrict__ a, double* __restrict__ A) {
    A[0] = a[2]; A[1] = -a[3]; A[2] = a[1];
    A[3] = a[3]; A[4] = a[2];  A[5] = -a[0];
    A[6] = 0.0;  A[7] = 0.0;   A[8] = 1.0;
}

// 1 - cos t without the cancellation of the literal form: sin^2 / (1 + cos) while cos > 0.  The reference's closed forms
// divide (1 - cos t) by t just above its small-angle threshold (|t| = 1e-5), where the literal subtraction keeps five
// digits, and its Jr^-1 entries are quotients with an O(t^3) numerator made of O(1) terms (fp64 error 1e-16 / t^3).
// Measured on Manhattan edges: two literal fp64 evaluations under different libms differ by 4e-11 in J on a sample, and
// the literal Jr^-1 is 3e-6 away from the function's value at a residual angle of 2.15e-5.  The same functions,
// evaluated stably here, agree with an extended-precision evaluation to 1e-15.
APEX_HD double se2_one_minus_cos(double cs, double sn) { return cs > 0.0 ? sn * sn / (1.0 + cs) : 1.0 - cs; }

// sin(t)/t and (1 - cos t)/t with the Taylor branch of the reference
APEX_HD void se2_ab(double th, double cs, double sn, double& a, double& b) {
    const double t2 = th * th;
    if (t2 < kSmallAngle2) { a = 1.0 - t2 / 6.0; b = 0.5 * th - th * t2 / 24.0; }
    else { a = sn / th; b = se2_one_minus_cos(cs, sn) / th; }
}

APEX_HD void se2_log(const double* __restrict__ p, double t[3]) {
    const double th = se2_angle(p);
    double a, b;
    se2_ab(th, cos(th), sin(th), a, b);
    const double den = 1.0 / (a * a + b * b), as = a * den, bs = b * den;
    t[0] = as * p[0] + bs * p[1];
    t[1] = -bs * p[0] + as * p[1];
    t[2] = th;
}
APEX_HD void se2_exp(const double t[3], double* __restrict__ p) {
    const double th = t[2], cs = cos(th), sn = sin(th);
    double a, b;
    se2_ab(th, cs, sn, a, b);
    p[0] = a * t[0] - b * t[1];
    p[1] = b * t[0] + a * t[1];
    p[2] = cs; p[3] = sn;
}
APEX_HD void se2_right_jacobian(const double t[3], double J[9]) {
    const double x = t[0], y = t[1], th = t[2], cs = cos(th), sn = sin(th), t2 = th * th;
    double a, b;
    se2_ab(th, cs, sn, a, b);
    J[0] = a;  J[1] = b; J[3] = -b; J[4] = a;
    J[6] = 0.0; J[7] = 0.0; J[8] = 1.0;
    if (t2 < kSmallAngle2) {
        J[2] = -y / 2.0 + th * x / 6.0;
        J[5] = x / 2.0 + th * y / 6.0;
    } else {
        J[2] = (-y + th * x + y * cs - x * sn) / t2;
        J[5] = (x + th * y - x * cs - y * sn) / t2;
    }
}
APEX_HD void se2_right_jacobian_inv(const double t[3], double J[9]) {
    const double x = t[0], y = t[1], th = t[2], cs = cos(th), sn = sin(th), t2 = th * th;
    J[1] = -th * 0.5; J[3] = -J[1];
    J[6] = 0.0; J[7] = 0.0; J[8] = 1.0;
    if (t2 > kSmallAngle2) {
        // the reference's entries (se2.rs:588-603) regrouped: J00 = t sin t / (2 (1 - cos t)) = (t/2) cot(t/2),
        // J02 = y/2 + x k, J12 = -x/2 + y k with k = (1 - J00) / t -- by its series in u = t/2 below |t| = 0.5, where
        // 1 - J00 cancels (the terms through u^13 leave 1e-15 relative at u = 0.25)
        J[0] = th * sn / (2.0 * se2_one_minus_cos(cs, sn));
        J[4] = J[0];
        double k;
        if (t2 < 0.25) {
            const double u = 0.5 * th, u2 = u * u;
            k = u * (1.0 / 6.0 + u2 * (1.0 / 90.0 + u2 * (1.0 / 945.0 + u2 * (1.0 / 9450.0 + u2 * (1.0 / 93555.0 +
                u2 * (691.0 / 638512875.0 + u2 * (2.0 / 18243225.0)))))));
        } else {
            k = (1.0 - J[0]) / th;
        }
        J[2] = y / 2.0 + x * k;
        J[5] = -x / 2.0 + y * k;
    } else {
        J[0] = 1.0 - t2 / 12.0;
        J[4] = J[0];
        J[2] = y / 2.0 + th * x / 12.0;
        J[5] = -x / 2.0 + th * y / 12.0;
    }
}

// residual only: r = Log((k1^-1 k0) * meas); A = k1^-1 k0 is handed back for the Jacobians
APEX_HD void between2_residual(const double* __restrict__ k0, const double* __restrict__ k1, const double* __restrict__ m,
                               double r[3], double A[4]) {
    double D[4];
    se2_between(k1, k0, A);
    se2_mul(A, m, D);
    se2_log(D, r);
}

// residual + both Jacobians (row-major 3 x 3), the chain J_log * J_compose * J_between as the factor multiplies it
APEX_HD void between2_linearize(const double* __restrict__ k0, const double* __restrict__ k1, const double* __restrict__ m,
                                double r[3], double J0[9], double J1[9]) {
    double A[4], Ai[4], mi[4], Jl[9], Am[9], Aa[9], C[9];
    between2_residual(k0, k1, m, r, A);
    se2_right_jacobian_inv(r, Jl);
    se2_inv(m, mi);
    se2_adjoint(mi, Am);          // d(A m)/dA
    se2_inv(A, Ai);
    se2_adjoint(Ai, Aa);          // dA/dk1 = -Adj(A^-1), dA/dk0 = I
#pragma unroll
    for (int i = 0; i < 9; ++i) Aa[i] = -Aa[i];
    m3_mul(Am, Aa, C);
    m3_mul(Jl, Am, J0);
    m3_mul(Jl, C, J1);
}

// ---- the loss correction of one 3-row block (r, J0, J1 row-major 3 x 3): what every 3-DOF manifold shares once its own
// linearisation has filled the block (SE2 here, SO3 in pg_so3_device.hpp) ---------------------------------------------------
// r and both Jacobians scaled by sqrt(rho') of the block's loss (pg_huber_scale; corrector.rs:143-181)
APEX_HD void block3_correct(double huber_delta, double r[3], double J0[9], double J1[9]) {
    const double sc = pg_huber_scale(huber_delta, r[0] * r[0] + r[1] * r[1] + r[2] * r[2]);
    if (sc != 1.0) {
#pragma unroll
        for (int i = 0; i < 3; ++i) r[i] *= sc;
#pragma unroll
        for (int i = 0; i < 9; ++i) { J0[i] *= sc; J1[i] *= sc; }
    }
}

// The same under the general loss (pg_loss.hpp; the type of the loss parameter is the compile-time policy, pg_device.hpp).
// First arm: the lines above with
// sqrt(rho').  Second arm, literally (corrector.rs:241-253, 292-298): r~ = residual_scaling r, J~ = sqrt(rho') (J - a r r^T J).
// false: rho' = 0, the edge contributes nothing; r, J0, J1 are zero.
APEX_HD bool block3_correct(const PgLoss& loss, double r[3], double J0[9], double J1[9]) {
    const PgCorrector c = pg_loss_corrector(loss, r[0] * r[0] + r[1] * r[1] + r[2] * r[2]);
    const double sc = c.sqrt_rho1;
    if (sc == 0.0) {
        r[0] = r[1] = r[2] = 0.0;
#pragma unroll
        for (int i = 0; i < 9; ++i) { J0[i] = 0.0; J1[i] = 0.0; }
        return false;
    }
    if (c.alpha_sq_norm == 0.0) {
        if (sc != 1.0) {
#pragma unroll
            for (int i = 0; i < 3; ++i) r[i] *= sc;
#pragma unroll
            for (int i = 0; i < 9; ++i) { J0[i] *= sc; J1[i] *= sc; }
        }
        return true;
    }
    const double a = c.alpha_sq_norm;
    double w0[3] = {0.0, 0.0, 0.0}, w1[3] = {0.0, 0.0, 0.0};   // r^T J
#pragma unroll
    for (int j = 0; j < 3; ++j) {
        w0[j] = r[0] * J0[j] + r[1] * J0[3 + j] + r[2] * J0[6 + j];
        w1[j] = r[0] * J1[j] + r[1] * J1[3 + j] + r[2] * J1[6 + j];
    }
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
        for (int j = 0; j < 3; ++j) {
            J0[3 * i + j] = sc * (J0[3 * i + j] - a * r[i] * w0[j]);
            J1[3 * i + j] = sc * (J1[3 * i + j] - a * r[i] * w1[j]);
        }
#pragma unroll
    for (int i = 0; i < 3; ++i) r[i] *= c.residual_scaling;
    return true;
}

// one SE2 edge, linearised and corrected under either loss form
APEX_HD void between2_corrected(const double* __restrict__ k0, const double* __restrict__ k1, const double* __restrict__ m,
                                double huber_delta, double r[3], double J0[9], double J1[9]) {
    between2_linearize(k0, k1, m, r, J0, J1);
    block3_correct(huber_delta, r, J0, J1);
}
APEX_HD bool between2_corrected(const double* __restrict__ k0, const double* __restrict__ k1, const double* __restrict__ m,
                                const PgLoss& loss, double r[3], double J0[9], double J1[9]) {
    between2_linearize(k0, k1, m, r, J0, J1);
    return block3_correct(loss, r, J0, J1);
}

// H += A^T B (3 x 3 row-major), g += A^T r
APEX_HD void jtj3_acc(const double* __restrict__ A, const double* __restrict__ B, double* __restrict__ H) {
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
        for (int j = 0; j < 3; ++j) H[3 * i + j] += A[i] * B[j] + A[3 + i] * B[3 + j] + A[6 + i] * B[6 + j];
}
APEX_HD void jtr3_acc(const double* __restrict__ A, const double r[3], double g[3]) {
#pragma unroll
    for (int i = 0; i < 3; ++i) g[i] += A[i] * r[0] + A[3 + i] * r[1] + A[6 + i] * r[2];
}

// PriorFactor on an SE2 variable: r = [x, y, theta] - data, J = I3; returns sqrt(rho') of the block's Huber loss
APEX_HD double prior2_eval(const double* __restrict__ v3, const double* __restrict__ data3, double delta, double r[3]) {
    double s = 0.0;
#pragma unroll
    for (int a = 0; a < 3; ++a) { r[a] = v3[a] - data3[a]; s += r[a] * r[a]; }
    const double sc = pg_huber_scale(delta, s);
#pragma unroll
    for (int a = 0; a < 3; ++a) r[a] *= sc;
    return sc;
}

// x (+) d = x * Exp(d), back in vector form.  x (+) 0 = x: a vector that does not move keeps its bits (all three DOF fixed).
APEX_HD void se2_plus(const double* __restrict__ v3, const double d[3], double* __restrict__ o3) {
    if (d[0] == 0.0 && d[1] == 0.0 && d[2] == 0.0) { o3[0] = v3[0]; o3[1] = v3[1]; o3[2] = v3[2]; return; }
    double p[4], e[4], q[4];
    se2_prepare(v3, p);
    se2_exp(d, e);
    se2_mul(p, e, q);
    o3[0] = q[0]; o3[1] = q[1]; o3[2] = se2_angle(q);
}

// One block-row of H = J^T J and of g = J^T r, owned by vertex v: the loop of k_pg2_assemble, host-compilable so that the
// test harness replays it.  inc_ptr / inc_edge: CSR of the edges incident to each vertex, ascending edge index, a
// self-loop listed once (pg2_lists.h).  Every edge of the list is re-linearised; H_vv and g_v accumulate in registers in
// list order; for an other endpoint u < v the block J_v^T J_u goes to add_off(u, B) -- blocks (v, u) with u < v are touched
// by the owner of row v only, so a plain read-add-write there has no race and duplicate edges sum in list order.
// M: a manifold with 3 tangent DOF (Se2Manifold below | So3Manifold of pg_so3_device.hpp); what it contributes is
// M::linearize on prepared poses of M::kStride doubles, everything after that is 3 x 3 blocks.
template <class M, typename AddOff, typename LossParam>
APEX_HD void pg_row_assemble(uint32_t v, const double* __restrict__ posep, const double* __restrict__ meas,
                             const uint32_t* __restrict__ e_from, const uint32_t* __restrict__ e_to,
                             const int* __restrict__ inc_ptr, const uint32_t* __restrict__ inc_edge, const LossParam& loss,
                             double Hvv[9], double gv[3], AddOff add_off) {
    static_assert(M::kDof == 3, "the row-owned assembly is written for 3 x 3 blocks");
#pragma unroll
    for (int i = 0; i < 9; ++i) Hvv[i] = 0.0;
    gv[0] = gv[1] = gv[2] = 0.0;
    for (int k = inc_ptr[v]; k < inc_ptr[v + 1]; ++k) {
        const uint32_t e = inc_edge[k], a = e_from[e], b = e_to[e];
        double r[3], J0[9], J1[9];
        M::linearize(posep + M::kStride * (size_t)a, posep + M::kStride * (size_t)b, meas + M::kStride * (size_t)e, r, J0, J1);
        if constexpr (std::is_same<LossParam, PgLoss>::value) {   // (an edge with rho' = 0 is skipped)
            if (!block3_correct(loss, r, J0, J1)) continue;
        } else {
            block3_correct(loss, r, J0, J1);
        }
        if (a == b) {   // self-loop: both Jacobians hit the same columns
#pragma unroll
            for (int i = 0; i < 9; ++i) J0[i] += J1[i];
            jtj3_acc(J0, J0, Hvv);
            jtr3_acc(J0, r, gv);
            continue;
        }
        const bool first = a == v;   // (selects, not pointers into the register arrays: no scratch)
        const uint32_t u = first ? b : a;
        double Jv[9], Ju[9];
#pragma unroll
        for (int i = 0; i < 9; ++i) { Jv[i] = first ? J0[i] : J1[i]; Ju[i] = first ? J1[i] : J0[i]; }
        jtj3_acc(Jv, Jv, Hvv);
        jtr3_acc(Jv, r, gv);
        if (u < v) {
            double B[9] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
            jtj3_acc(Jv, Ju, B);
            add_off(u, B);
        }
    }
}

// ---- edge information matrices ------------------------------------------------------------------------
// One SE2 edge with Omega = U^T U under the general corrector, corrected but NOT whitened:
//     r^ = residual_scaling r,   J^ = sqrt(rho') (J - a r (Omega r)^T J),   s = r^T Omega r
// so that the whitened block is r~ = U r^, J~ = U J^ and every product closes with Omega: J~_a^T J~_b = J^_a^T Omega J^_b,
// J~_v^T r~ = J^_v^T Omega r^.  The hot kernels need Omega only.  false: rho' = 0, the edge contributes nothing; r, J0, J1 are zero.
// (block3_weight: the correction alone, on a block any 3-DOF manifold has linearised)
APEX_HD bool block3_weight(const PgLoss& loss, const double* __restrict__ W, double r[3], double J0[9], double J1[9]) {
    double Wr[3];
    info_mv<3>(W, r, Wr);
    const PgCorrector c = pg_loss_corrector(loss, fmax(dotn<3>(r, Wr), 0.0));
    const double sc = c.sqrt_rho1;
    if (sc == 0.0) {
        r[0] = r[1] = r[2] = 0.0;
#pragma unroll
        for (int i = 0; i < 9; ++i) { J0[i] = 0.0; J1[i] = 0.0; }
        return false;
    }
    const double a = c.alpha_sq_norm;
    if (a != 0.0) {
        double w0[3], w1[3];   // a (Omega r)^T J
#pragma unroll
        for (int j = 0; j < 3; ++j) {
            w0[j] = a * (Wr[0] * J0[j] + Wr[1] * J0[3 + j] + Wr[2] * J0[6 + j]);
            w1[j] = a * (Wr[0] * J1[j] + Wr[1] * J1[3 + j] + Wr[2] * J1[6 + j]);
        }
#pragma unroll
        for (int i = 0; i < 3; ++i)
#pragma unroll
            for (int j = 0; j < 3; ++j) { J0[3 * i + j] -= r[i] * w0[j]; J1[3 * i + j] -= r[i] * w1[j]; }
    }
#pragma unroll
    for (int i = 0; i < 9; ++i) { J0[i] *= sc; J1[i] *= sc; }
#pragma unroll
    for (int i = 0; i < 3; ++i) r[i] *= c.residual_scaling;
    return true;
}
APEX_HD bool between2_weighted(const double* __restrict__ k0, const double* __restrict__ k1, const double* __restrict__ m,
                               const PgLoss& loss, const double* __restrict__ W, double r[3], double J0[9], double J1[9]) {
    between2_linearize(k0, k1, m, r, J0, J1);
    return block3_weight(loss, W, r, J0, J1);
}

// M = Omega J (3 x 3 row-major)
APEX_HD void info_mul3(const double* __restrict__ W, const double* __restrict__ J, double* __restrict__ M) {
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
        for (int j = 0; j < 3; ++j) M[3 * i + j] = W[3 * i] * J[j] + W[3 * i + 1] * J[3 + j] + W[3 * i + 2] * J[6 + j];
}

// pg2_assemble_row with information: info holds the packed upper triangle of every edge's Omega (InfoPack<3>: six doubles, the
// caller's edge order).  Row-owned like pg2_assemble_row: the same lists, the same order of summation, no atomics.  The block
// of row v and column u is J^_v^T (Omega J^_u) -- Omega sits between the two Jacobians, so the block of (u, v) is its transpose
// and not the same product with the roles swapped.
template <class Man, typename AddOff>   // (Man: M is the block Omega J below)
APEX_HD void pg_row_assemble_info(uint32_t v, const double* __restrict__ posep, const double* __restrict__ meas,
                                  const uint32_t* __restrict__ e_from, const uint32_t* __restrict__ e_to,
                                  const int* __restrict__ inc_ptr, const uint32_t* __restrict__ inc_edge,
                                  const double* __restrict__ info, const PgLoss& loss, double Hvv[9], double gv[3], AddOff add_off) {
    static_assert(Man::kDof == 3, "the row-owned assembly is written for 3 x 3 blocks");
#pragma unroll
    for (int i = 0; i < 9; ++i) Hvv[i] = 0.0;
    gv[0] = gv[1] = gv[2] = 0.0;
    for (int k = inc_ptr[v]; k < inc_ptr[v + 1]; ++k) {
        const uint32_t e = inc_edge[k], a = e_from[e], b = e_to[e];
        double W[9], r[3], Wr[3], J0[9], J1[9];
        info_unpack<3>(info + InfoPack<3>::kStride * (size_t)e, W);
        Man::linearize(posep + Man::kStride * (size_t)a, posep + Man::kStride * (size_t)b, meas + Man::kStride * (size_t)e, r, J0, J1);
        if (!block3_weight(loss, W, r, J0, J1)) continue;
        info_mv<3>(W, r, Wr);
        double M[9];
        if (a == b) {   // self-loop: both Jacobians hit the same columns
#pragma unroll
            for (int i = 0; i < 9; ++i) J0[i] += J1[i];
            info_mul3(W, J0, M);
            jtj3_acc(J0, M, Hvv);
            jtr3_acc(J0, Wr, gv);
            continue;
        }
        const bool first = a == v;   // (selects, not pointers into the register arrays: no scratch)
        const uint32_t u = first ? b : a;
        double Jv[9], Ju[9];
#pragma unroll
        for (int i = 0; i < 9; ++i) { Jv[i] = first ? J0[i] : J1[i]; Ju[i] = first ? J1[i] : J0[i]; }
        info_mul3(W, Jv, M);
        jtj3_acc(Jv, M, Hvv);
        jtr3_acc(Jv, Wr, gv);
        if (u < v) {
            double B[9] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
            info_mul3(W, Ju, M);
            jtj3_acc(Jv, M, B);
            add_off(u, B);
        }
    }
}

// The per-edge members of a 3-DOF manifold trait that need nothing but its linearisation: D::linearize(k0, k1, m, r, J0, J1)
// fills the uncorrected block, and the loss, the information matrix, the products and the exports are 3 x 3 from there on.
// Se2Manifold and So3Manifold (pg_so3_device.hpp) derive from it (D is the deriving trait).
template <class D>
struct Dof3EdgeOps {
    // u = J~0 a0 + J~1 a1, w = J~0 b0 + J~1 b1 for the corrected Jacobians of one edge (the linearisation of pg_row_assemble:
    // D::linearize, then block3_correct); a0 / b0: the three tangent entries of k0's vertex, a1 / b1 of k1's
    template <typename LossParam>
    static APEX_HD void edge_jv(const double* __restrict__ k0, const double* __restrict__ k1, const double* __restrict__ m, const LossParam& loss,
                                const double a0[3], const double a1[3], const double b0[3], const double b1[3], double u[3], double w[3]) {
        double r[3], J0[9], J1[9];
        D::linearize(k0, k1, m, r, J0, J1);
        (void)block3_correct(loss, r, J0, J1);
#pragma unroll
        for (int i = 0; i < 3; ++i) {
            u[i] = (J0[3 * i] * a0[0] + J0[3 * i + 1] * a0[1] + J0[3 * i + 2] * a0[2]) + (J1[3 * i] * a1[0] + J1[3 * i + 1] * a1[1] + J1[3 * i + 2] * a1[2]);
            w[i] = (J0[3 * i] * b0[0] + J0[3 * i + 1] * b0[1] + J0[3 * i + 2] * b0[2]) + (J1[3 * i] * b1[0] + J1[3 * i + 1] * b1[1] + J1[3 * i + 2] * b1[2]);
        }
    }
    // With Omega (LossWeighted): u = J^0 a0 + J^1 a1, w = J^0 b0 + J^1 b1 for the corrected, not whitened Jacobians of
    // block3_weight; the caller closes the products with Omega: (J~ a).(J~ b) = u^T Omega w.
    static APEX_HD void edge_jv_info(const double* __restrict__ k0, const double* __restrict__ k1, const double* __restrict__ m, const PgLoss& loss,
                                     const double* __restrict__ W, const double a0[3], const double a1[3], const double b0[3], const double b1[3],
                                     double u[3], double w[3]) {
        double r[3], J0[9], J1[9];
        D::linearize(k0, k1, m, r, J0, J1);
        (void)block3_weight(loss, W, r, J0, J1);
#pragma unroll
        for (int i = 0; i < 3; ++i) {
            u[i] = (J0[3 * i] * a0[0] + J0[3 * i + 1] * a0[1] + J0[3 * i + 2] * a0[2]) + (J1[3 * i] * a1[0] + J1[3 * i + 1] * a1[1] + J1[3 * i + 2] * a1[2]);
            w[i] = (J0[3 * i] * b0[0] + J0[3 * i + 1] * b0[1] + J0[3 * i + 2] * b0[2]) + (J1[3 * i] * b1[0] + J1[3 * i + 1] * b1[1] + J1[3 * i + 2] * b1[2]);
        }
    }
    // the literal whitened, corrected residual [3] and Jacobian [3][6] of one edge (info_export_block: factors Omega here)
    static APEX_HD void export_edge_info(const double* __restrict__ k0, const double* __restrict__ k1, const double* __restrict__ m,
                                         const PgLoss& loss, const double* __restrict__ W, double* __restrict__ r_out, double* __restrict__ j_out) {
        double r[3], J0[9], J1[9], Jd[18];
        D::linearize(k0, k1, m, r, J0, J1);
        for (int i = 0; i < 3; ++i)
            for (int j = 0; j < 3; ++j) { Jd[6 * i + j] = J0[3 * i + j]; Jd[6 * i + 3 + j] = J1[3 * i + j]; }
        info_export_block<3>(W, loss, r, Jd, r_out, j_out);
    }
    // corrected residual [3] and Jacobian [3][6] = [dr/dk0 | dr/dk1] of one edge (either may be null); sqrt(rho') is
    // applied inside block3_correct
    template <typename LossParam>
    static APEX_HD void export_edge(const double* __restrict__ k0, const double* __restrict__ k1, const double* __restrict__ m,
                                    const LossParam& loss, double* __restrict__ r_out, double* __restrict__ j_out) {
        double r[3], J0[9], J1[9];
        D::linearize(k0, k1, m, r, J0, J1);
        (void)block3_correct(loss, r, J0, J1);
        if (r_out)
            for (int i = 0; i < 3; ++i) r_out[i] = r[i];
        if (j_out)
            for (int i = 0; i < 3; ++i)
                for (int j = 0; j < 3; ++j) {
                    j_out[6 * i + j] = J0[3 * i + j];
                    j_out[6 * i + 3 + j] = J1[3 * i + j];
                }
    }
};

// The SE2 side of the trait pg_device.hpp describes at Se3Manifold.
struct Se2Manifold : Dof3EdgeOps<Se2Manifold> {
    static constexpr int kDof = 3;                 // tangent columns per vertex
    static constexpr int kAmb = 3;                 // stored doubles per vertex / measurement / prior: x y theta
    static constexpr int kStride = kPose2Stride;   // doubles per prepared pose / measurement (x y cos sin)
    static constexpr int kPriorStride = kStride;   // doubles per prior block: data (kAmb) | the block's Huber delta
    static constexpr bool kPriorOnPrepared = false;   // the prior sees [x, y, theta] itself

    static APEX_HD void prepare(const double* __restrict__ v, double* __restrict__ o) { se2_prepare(v, o); }
    static APEX_HD void plus(const double* x, const double* d, double* o) { se2_plus(x, d, o); }
    static APEX_HD void residual(const double* __restrict__ k0, const double* __restrict__ k1, const double* __restrict__ m, double r[3]) {
        double A[4];
        between2_residual(k0, k1, m, r, A);
    }
    static APEX_HD double prior_residual(const double* __restrict__ x, const double* __restrict__ data, double delta, double r[3]) {
        return prior2_eval(x, data, delta, r);
    }
    static APEX_HD double cost_add_prior(double acc, const double r[3]) {   // the block's squared norm first, then one add
        return acc + (r[0] * r[0] + r[1] * r[1] + r[2] * r[2]);
    }
    static APEX_HD void linearize(const double* __restrict__ k0, const double* __restrict__ k1, const double* __restrict__ m,
                                  double r[3], double J0[9], double J1[9]) {
        between2_linearize(k0, k1, m, r, J0, J1);
    }
};

// The SE2 instantiations under the names they have always had (tests/host_harness_se2.cpp, host_harness_loss.cpp, host_harness_info.cpp)
template <typename AddOff, typename LossParam>
APEX_HD void pg2_assemble_row(uint32_t v, const double* __restrict__ posep, const double* __restrict__ meas,
                              const uint32_t* __restrict__ e_from, const uint32_t* __restrict__ e_to,
                              const int* __restrict__ inc_ptr, const uint32_t* __restrict__ inc_edge, const LossParam& loss,
                              double Hvv[9], double gv[3], AddOff add_off) {
    pg_row_assemble<Se2Manifold>(v, posep, meas, e_from, e_to, inc_ptr, inc_edge, loss, Hvv, gv, add_off);
}
template <typename AddOff>
APEX_HD void pg2_assemble_row_info(uint32_t v, const double* __restrict__ posep, const double* __restrict__ meas,
                                   const uint32_t* __restrict__ e_from, const uint32_t* __restrict__ e_to,
                                   const int* __restrict__ inc_ptr, const uint32_t* __restrict__ inc_edge,
                                   const double* __restrict__ info, const PgLoss& loss, double Hvv[9], double gv[3], AddOff add_off) {
    pg_row_assemble_info<Se2Manifold>(v, posep, meas, e_from, e_to, inc_ptr, inc_edge, info, loss, Hvv, gv, add_off);
}

}  // namespace apex
