// pg_device.hpp -- per-edge SE3 pose-graph math behind the kernels of pg_kernels.hip, and Se3Manifold, the trait through
// which the manifold-generic kernels there reach it.
//
// APEX_HD (host+device) like ba_device.hpp, so tests/host_harness.cpp runs the same code on the CPU.
//
// Reference semantics (file:line under the apex-solver tree):
//   BetweenFactor<SE3>::linearize      src/factors/between_factor.rs:268-322
//       r = Log((k1^-1 k0) * meas),  dr/dk0 = Jr^-1(r) Adj(meas^-1),
//       dr/dk1 = Jr^-1(r) (Adj(meas^-1) (-Adj((k1^-1 k0)^-1)))
//   LieGroup::between                  crates/apex-manifolds/src/lib.rs:401-419
//   SE3 inverse / compose / log / Adj  crates/apex-manifolds/src/se3.rs:242-320, 347-369
//   Q block and Jr^-1 (as coded)       se3.rs:520-558, 652-666
//   SO3 log, Jl^-1                     crates/apex-manifolds/src/so3.rs:313-357, 628-646
//
// Every 6x6 Jacobian on this path is block upper-triangular with equal diagonal blocks,
//     J = [ P  T ]        (Adj = [R, [t]x R; 0, R],  Jr^-1 = [D, B; 0, D])
//         [ 0  P ]
// so a Jacobian travels as the pair (P, T): 18 doubles instead of 36, and J_a^T J_b needs three
// 3x3 products instead of a 6x6x6 one.
#pragma once
#include <stddef.h>

#include <type_traits>

#include "ba_device.hpp"
#include "info_pack.h"
#include "pg_loss.hpp"

namespace apex {

struct Jac6 {  // [P T; 0 P], row-major 3x3 blocks
    double P[9];
    double T[9];
};

APEX_HD void m3_mul(const double* A, const double* B, double* C) {  // C = A B (C must not alias)
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
        for (int j = 0; j < 3; ++j) C[3 * i + j] = A[3 * i] * B[j] + A[3 * i + 1] * B[3 + j] + A[3 * i + 2] * B[6 + j];
}
APEX_HD void m3_tmul(const double* A, const double* B, double* C) {  // C = A^T B
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
        for (int j = 0; j < 3; ++j) C[3 * i + j] = A[i] * B[j] + A[3 + i] * B[3 + j] + A[6 + i] * B[6 + j];
}
APEX_HD void hat3(const double v[3], double M[9]) {
    M[0] = 0.0;   M[1] = -v[2]; M[2] = v[1];
    M[3] = v[2];  M[4] = 0.0;   M[5] = -v[0];
    M[6] = -v[1]; M[7] = v[0];  M[8] = 0.0;
}
// [t]x R
APEX_HD void hat_mul(const double t[3], const double* R, double* C) {
#pragma unroll
    for (int j = 0; j < 3; ++j) {
        C[j] = -t[2] * R[3 + j] + t[1] * R[6 + j];
        C[3 + j] = t[2] * R[j] - t[0] * R[6 + j];
        C[6 + j] = -t[1] * R[j] + t[0] * R[3 + j];
    }
}

// pose as the kernels hold it: translation + unit quaternion [w,x,y,z] (k_pg_prepare normalises twice,
// like SE3::from(DVector), se3.rs:107-113, 200-206)
// (the quaternion's two passes stand alone so that an SO3 vertex with the same quaternion prepares to the same bits, pg_so3_device.hpp)
APEX_HD void quat_normalise_twice(const double* __restrict__ q4, double* __restrict__ o4) {
    double w = q4[0], x = q4[1], y = q4[2], z = q4[3];
#pragma unroll
    for (int pass = 0; pass < 2; ++pass) {
        const double n = sqrt(w * w + x * x + y * y + z * z);
        w /= n; x /= n; y /= n; z /= n;
    }
    o4[0] = w; o4[1] = x; o4[2] = y; o4[3] = z;
}
APEX_HD void pose_normalise(const double* __restrict__ v7, double* __restrict__ o7) {
    o7[0] = v7[0]; o7[1] = v7[1]; o7[2] = v7[2];
    quat_normalise_twice(v7 + 3, o7 + 3);
}

// a^-1 for a = (t, q)
APEX_HD void se3_inv(const double t[3], const double q[4], double ti[3], double qi[4]) {
    qi[0] = q[0]; qi[1] = -q[1]; qi[2] = -q[2]; qi[3] = -q[3];
    double r[3];
    quat_rotate(qi, t, r);
    ti[0] = -r[0]; ti[1] = -r[1]; ti[2] = -r[2];
}
// a * b
APEX_HD void se3_mul(const double ta[3], const double qa[4], const double tb[3], const double qb[4], double t[3], double q[4]) {
    double r[3];
    quat_mul(qa, qb, q);
    quat_rotate(qa, tb, r);
    t[0] = r[0] + ta[0]; t[1] = r[1] + ta[1]; t[2] = r[2] + ta[2];
}

// SO3::log (so3.rs:313-357): atan2 form, mirrored for w < 0
APEX_HD void so3_log(const double q[4], double th[3]) {
    const double s2 = q[1] * q[1] + q[2] * q[2] + q[3] * q[3];
    double coeff = 2.0;
    if (s2 > kSmallAngle2) {
        const double s = sqrt(s2), c = q[0];
        const double two = 2.0 * (c < 0.0 ? atan2(-s, -c) : atan2(s, c));
        coeff = two / s;
    }
    th[0] = q[1] * coeff; th[1] = q[2] * coeff; th[2] = q[3] * coeff;
}

// Jl^-1(theta) = I - 1/2 K + (1/a - (1+cos t)/(2 t sin t)) K^2 (so3.rs:628-646)
APEX_HD void so3_left_jacobian_inv(const double th[3], double D[9]) {
    const double a = th[0] * th[0] + th[1] * th[1] + th[2] * th[2];
    double K[9], K2[9];
    hat3(th, K);
    m3_mul(K, K, K2);
    double c2 = 0.0;
    if (a > kSmallAngle2) {
        const double t = sqrt(a);
        c2 = 1.0 / a - (1.0 + cos(t)) / (2.0 * t * sin(t));
    }
#pragma unroll
    for (int i = 0; i < 9; ++i) D[i] = -0.5 * K[i] + c2 * K2[i];
    D[0] += 1.0; D[4] += 1.0; D[8] += 1.0;
}

// Q(rho, theta) exactly as the reference codes it (se3.rs:520-558), d coefficient included
APEX_HD void se3_q_block(const double rho[3], const double th[3], double Q[9]) {
    double Rk[9], Tk[9];
    hat3(rho, Rk);
    hat3(th, Tk);
    const double t2 = th[0] * th[0] + th[1] * th[1] + th[2] * th[2];
    const double a = 0.5;
    double b = 1.0 / 6.0 + 1.0 / 120.0 * t2, c = -1.0 / 24.0 + 1.0 / 720.0 * t2, d = -1.0 / 60.0;
    if (t2 > kSmallAngle2) {
        const double tn = sqrt(t2), tn3 = tn * t2, tn4 = t2 * t2, tn5 = tn3 * t2;
        const double s = sin(tn), co = cos(tn);
        b = (tn - s) / tn3;
        c = (1.0 - t2 / 2.0 - co) / tn4;
        d = (c - 3.0) * (tn - s - tn3 / 6.0) / tn5;
    }
    double tr[9], rt[9], trt[9], rtt[9], trtt[9];
    m3_mul(Tk, Rk, tr);
    m3_mul(Rk, Tk, rt);
    m3_mul(tr, Tk, trt);
    m3_mul(rt, Tk, rtt);
    m3_mul(trt, Tk, trtt);
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
        for (int j = 0; j < 3; ++j) {
            const int ij = 3 * i + j, ji = 3 * j + i;
            Q[ij] = Rk[ij] * a + (tr[ij] + rt[ij] + trt[ij]) * b - (rtt[ij] - rtt[ji] - trt[ij] * 3.0) * c - trtt[ij] * d;
        }
}

// residual only: r = Log((k1^-1 k0) * meas); poses are prepared (unit quaternions)
APEX_HD void between_residual(const double* __restrict__ k0, const double* __restrict__ k1, const double* __restrict__ m,
                              double r[6], double tA[3], double qA[4], double D[9]) {
    double t1i[3], q1i[4], tD[3], qD[4];
    se3_inv(k1, k1 + 3, t1i, q1i);
    se3_mul(t1i, q1i, k0, k0 + 3, tA, qA);
    se3_mul(tA, qA, m, m + 3, tD, qD);
    so3_log(qD, r + 3);
    so3_left_jacobian_inv(r + 3, D);
#pragma unroll
    for (int i = 0; i < 3; ++i) r[i] = D[3 * i] * tD[0] + D[3 * i + 1] * tD[1] + D[3 * i + 2] * tD[2];
}

// residual + both Jacobians
APEX_HD void between_linearize(const double* __restrict__ k0, const double* __restrict__ k1, const double* __restrict__ m,
                               double r[6], Jac6& J0, Jac6& J1) {
    double tA[3], qA[4], D[9];
    between_residual(k0, k1, m, r, tA, qA, D);
    // Jr^-1(r) = [D, B; 0, D],  B = -D Q(-rho,-theta) D
    double B[9];
    {
        const double nrho[3] = {-r[0], -r[1], -r[2]}, nth[3] = {-r[3], -r[4], -r[5]};
        double Q[9], T[9];
        se3_q_block(nrho, nth, Q);
        m3_mul(D, Q, T);
        m3_mul(T, D, B);
#pragma unroll
        for (int i = 0; i < 9; ++i) B[i] = -B[i];
    }
    // Adj(meas^-1) = [Rm, Tm; 0, Rm]
    double Rm[9], Tm[9];
    {
        double tmi[3], qmi[4];
        se3_inv(m, m + 3, tmi, qmi);
        quat_to_rot(qmi, Rm);
        hat_mul(tmi, Rm, Tm);
    }
    // dr/dk0 = Jr^-1 Adj(meas^-1)
    m3_mul(D, Rm, J0.P);
    {
        double X[9], Y[9];
        m3_mul(D, Tm, X);
        m3_mul(B, Rm, Y);
#pragma unroll
        for (int i = 0; i < 9; ++i) J0.T[i] = X[i] + Y[i];
    }
    // Adj(A^-1) = [Ra, Ta; 0, Ra];  d1 = Adj(meas^-1) (-Adj(A^-1)) = -[Rm Ra, Rm Ta + Tm Ra; 0, Rm Ra]
    double M[9], N[9];
    {
        double tAi[3], qAi[4], Ra[9], Ta[9], X[9], Y[9];
        se3_inv(tA, qA, tAi, qAi);
        quat_to_rot(qAi, Ra);
        hat_mul(tAi, Ra, Ta);
        m3_mul(Rm, Ra, M);
        m3_mul(Rm, Ta, X);
        m3_mul(Tm, Ra, Y);
#pragma unroll
        for (int i = 0; i < 9; ++i) { M[i] = -M[i]; N[i] = -(X[i] + Y[i]); }
    }
    // dr/dk1 = Jr^-1 d1
    m3_mul(D, M, J1.P);
    {
        double X[9], Y[9];
        m3_mul(D, N, X);
        m3_mul(B, M, Y);
#pragma unroll
        for (int i = 0; i < 9; ++i) J1.T[i] = X[i] + Y[i];
    }
}

// sqrt(rho') of HuberLoss for squared norm s (loss_functions.rs:364-380); delta <= 0: no loss
APEX_HD double pg_huber_scale(double delta, double s) {
    if (delta > 0.0 && s > delta * delta) return sqrt(delta / sqrt(s));
    return 1.0;
}

// H_ab = J_a^T J_b (6x6 row-major) for J = [P T; 0 P]
APEX_HD void jtj(const Jac6& A, const Jac6& B, double H[36]) {
    double pp[9], pt[9], tp[9], tt[9];
    m3_tmul(A.P, B.P, pp);
    m3_tmul(A.P, B.T, pt);
    m3_tmul(A.T, B.P, tp);
    m3_tmul(A.T, B.T, tt);
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
        for (int j = 0; j < 3; ++j) {
            H[6 * i + j] = pp[3 * i + j];
            H[6 * i + 3 + j] = pt[3 * i + j];
            H[6 * (i + 3) + j] = tp[3 * i + j];
            H[6 * (i + 3) + 3 + j] = tt[3 * i + j] + pp[3 * i + j];
        }
}
// g_a = J_a^T r
APEX_HD void jtr(const Jac6& A, const double r[6], double g[6]) {
#pragma unroll
    for (int i = 0; i < 3; ++i) {
        g[i] = A.P[i] * r[0] + A.P[3 + i] * r[1] + A.P[6 + i] * r[2];
        g[3 + i] = (A.T[i] * r[0] + A.T[3 + i] * r[1] + A.T[6 + i] * r[2]) + (A.P[i] * r[3] + A.P[3 + i] * r[4] + A.P[6 + i] * r[5]);
    }
}

// ---- the general loss (pg_loss.hpp) ---------------------------------------------------------------------------------
// The compile-time loss policy is the type of the loss parameter: a double is the Huber delta of set_structure and selects
// the code above and below exactly as it was; a PgLoss selects the general corrector.  A kernel is instantiated once per
// policy and its launcher picks (pg_kernels.hip).
struct LossLegacy  { using Param = double; static constexpr bool kGeneral = false; };
struct LossGeneral { using Param = PgLoss; static constexpr bool kGeneral = true; };

// One SE3 edge under the general corrector, in the form the assembly uses.  J~ = sqrt(rho') (J - a r r^T J) is never formed:
// it would lose the [P T; 0 P] shape.  With w_v = J_v^T r (J and r uncorrected, s = |r|^2, a = alpha_sq_norm):
//     J~_a^T J~_b = rho' (J_a^T J_b - a (2 - a s) w_a w_b^T)
//     J~_v^T r~   = sqrt(rho') residual_scaling (1 - a s) w_v
//     J~ x        = sqrt(rho') (J x - a r (w . x))
// In the first arm a = 0 and this is rho' J^T J, rho' w, sqrt(rho') J x.
struct EdgeNormal6 {
    PgCorrector c;
    double s;             // |r|^2
    double w0[6], w1[6];  // J0^T r, J1^T r
    double rho1, kap, gsc;   // sqrt_rho1^2, a (2 - a s), sqrt_rho1 residual_scaling (1 - a s)

    // H = J_a^T J_b (jtj) -> J~_a^T J~_b
    APEX_HD void correct(double H[36], const double wa[6], const double wb[6]) const {
#pragma unroll
        for (int i = 0; i < 6; ++i)
#pragma unroll
            for (int j = 0; j < 6; ++j) H[6 * i + j] = rho1 * (H[6 * i + j] - kap * wa[i] * wb[j]);
    }
    APEX_HD void grad(const double w[6], double g[6]) const {
#pragma unroll
        for (int i = 0; i < 6; ++i) g[i] = gsc * w[i];
    }
};

// The uncorrected linearisation, then the corrector and what EdgeNormal6 needs.  false: rho' = 0, the edge contributes nothing.
// (between_linearize is called whole, exactly as the huber_delta path calls it: splitting it into a residual and a Jacobian
// half so that the loss could run in between changed the instructions of the huber_delta kernels as well.)
APEX_HD bool between_linearize_general(const double* __restrict__ k0, const double* __restrict__ k1, const double* __restrict__ m,
                                       const PgLoss& loss, double r[6], Jac6& J0, Jac6& J1, EdgeNormal6& n) {
    between_linearize(k0, k1, m, r, J0, J1);
    n.s = r[0] * r[0] + r[1] * r[1] + r[2] * r[2] + r[3] * r[3] + r[4] * r[4] + r[5] * r[5];
    n.c = pg_loss_corrector(loss, n.s);
    if (n.c.sqrt_rho1 == 0.0) return false;
    const double as = n.c.alpha_sq_norm * n.s;
    n.rho1 = n.c.sqrt_rho1 * n.c.sqrt_rho1;
    n.kap = n.c.alpha_sq_norm * (2.0 - as);
    n.gsc = n.c.sqrt_rho1 * n.c.residual_scaling * (1.0 - as);
    jtr(J0, r, n.w0);
    jtr(J1, r, n.w1);
    return true;
}

// ---- edge information matrices ------------------------------------------------------------------------
// Edge e may carry a symmetric positive-definite D x D matrix Omega = U^T U in the tangent order of the residual.  The block
// is the reference's block whitened, r_w = U r, J_w = U J, and the loss acts on (r_w, J_w, s = r^T Omega r) through the same
// corrector.  The third loss policy: the general corrector plus Omega.  Its instantiations are the only code that reads
// PGView::info; no loss, L2 and Huber run through it too (as a PgLoss of that kind) when information is set.
struct LossWeighted { using Param = PgLoss; static constexpr bool kGeneral = true; };

// Omega travels packed (InfoPack<D>, info_pack.h: the layout, beside the host code that checks and packs the matrices)
template <int D>
APEX_HD void info_unpack(const double* __restrict__ p, double* __restrict__ W) {   // -> full, row-major
    int k = 0;
#pragma unroll
    for (int i = 0; i < D; ++i)
#pragma unroll
        for (int j = i; j < D; ++j) { W[D * i + j] = p[k]; W[D * j + i] = p[k]; ++k; }
}
// y = Omega x
template <int D>
APEX_HD void info_mv(const double* __restrict__ W, const double* __restrict__ x, double* __restrict__ y) {
#pragma unroll
    for (int i = 0; i < D; ++i) {
        double acc = W[D * i] * x[0];
#pragma unroll
        for (int j = 1; j < D; ++j) acc += W[D * i + j] * x[j];
        y[i] = acc;
    }
}
template <int D>
APEX_HD double dotn(const double* __restrict__ x, const double* __restrict__ y) {
    double acc = x[0] * y[0];
#pragma unroll
    for (int i = 1; i < D; ++i) acc += x[i] * y[i];
    return acc;
}
// s = r^T Omega r (never negative: a rounding residue below zero would send sqrt(s) of a loss to NaN)
template <int D>
APEX_HD double info_sqnorm(const double* __restrict__ W, const double* __restrict__ r) {
    double Wr[D];
    info_mv<D>(W, r, Wr);
    return fmax(dotn<D>(r, Wr), 0.0);
}
// U upper-triangular with Omega = U^T U (the transpose of the Cholesky factor); Omega is positive definite (the host checks)
template <int D>
APEX_HD void info_chol_upper(const double* __restrict__ W, double* __restrict__ U) {
    for (int i = 0; i < D * D; ++i) U[i] = 0.0;
    for (int i = 0; i < D; ++i)
        for (int j = i; j < D; ++j) {
            double acc = W[D * i + j];
            for (int k = 0; k < i; ++k) acc -= U[D * k + i] * U[D * k + j];
            U[D * i + j] = i == j ? sqrt(acc) : acc / U[D * i + i];
        }
}
// The literal whitened and corrected block of one edge, for the exports (not hot): r~ = residual_scaling U r,
// J~ = sqrt(rho') U (J - a r (Omega r)^T J); r [D], J [D][2 D] uncorrected.  An edge with rho' = 0 is written as zeros.
template <int D>
APEX_HD void info_export_block(const double* __restrict__ W, const PgLoss& loss, const double* __restrict__ r, const double* __restrict__ J,
                               double* __restrict__ r_out, double* __restrict__ j_out) {
    double Wr[D], w[2 * D], U[D * D];
    info_mv<D>(W, r, Wr);
    const double s = fmax(dotn<D>(r, Wr), 0.0);
    const PgCorrector c = pg_loss_corrector(loss, s);
    if (c.sqrt_rho1 == 0.0) {
        if (r_out) for (int i = 0; i < D; ++i) r_out[i] = 0.0;
        if (j_out) for (int i = 0; i < 2 * D * D; ++i) j_out[i] = 0.0;
        return;
    }
    info_chol_upper<D>(W, U);
    if (r_out)
        for (int i = 0; i < D; ++i) {
            double acc = 0.0;
            for (int k = i; k < D; ++k) acc += U[D * i + k] * r[k];
            r_out[i] = c.residual_scaling * acc;
        }
    if (!j_out) return;
    for (int j = 0; j < 2 * D; ++j) {
        double acc = 0.0;
        for (int k = 0; k < D; ++k) acc += Wr[k] * J[2 * D * k + j];
        w[j] = c.alpha_sq_norm * acc;   // a (Omega r)^T J
    }
    for (int i = 0; i < D; ++i)
        for (int j = 0; j < 2 * D; ++j) {
            double acc = 0.0;
            for (int k = i; k < D; ++k) acc += U[D * i + k] * (J[2 * D * k + j] - r[k] * w[j]);
            j_out[2 * D * i + j] = c.sqrt_rho1 * acc;
        }
}

// M = Omega J for J = [P T; 0 P]: dense 6 x 6, formed once per Jacobian and used by every block that has it on the right
APEX_HD void info_mul_jac(const double* __restrict__ W, const Jac6& J, double* __restrict__ M) {
#pragma unroll
    for (int i = 0; i < 6; ++i)
#pragma unroll
        for (int j = 0; j < 3; ++j) {
            M[6 * i + j] = W[6 * i] * J.P[j] + W[6 * i + 1] * J.P[3 + j] + W[6 * i + 2] * J.P[6 + j];
            M[6 * i + 3 + j] = (W[6 * i] * J.T[j] + W[6 * i + 1] * J.T[3 + j] + W[6 * i + 2] * J.T[6 + j]) +
                               (W[6 * i + 3] * J.P[j] + W[6 * i + 4] * J.P[3 + j] + W[6 * i + 5] * J.P[6 + j]);
        }
}
// G = A^T M for A = [P T; 0 P]: with M = Omega J_b this is G_ab = J_a^T Omega J_b.  Not symmetric in (a, b) unless Omega is
// a multiple of I: the block of row vertex a and column vertex b is G_ab, the transposed one is G_ba.
APEX_HD void jt_mul(const Jac6& A, const double* __restrict__ M, double* __restrict__ G) {
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
        for (int j = 0; j < 6; ++j) {
            G[6 * i + j] = A.P[i] * M[j] + A.P[3 + i] * M[6 + j] + A.P[6 + i] * M[12 + j];
            G[6 * (i + 3) + j] = (A.T[i] * M[j] + A.T[3 + i] * M[6 + j] + A.T[6 + i] * M[12 + j]) +
                                 (A.P[i] * M[18 + j] + A.P[3 + i] * M[24 + j] + A.P[6 + i] * M[30 + j]);
        }
}

// between_linearize_general with Omega: s = r^T Omega r and w_v = J_v^T (Omega r).  With those, EdgeNormal6 corrects
// G_ab = J_a^T Omega J_b exactly as it corrects J_a^T J_b:
//     J~_a^T J~_b = rho' (G_ab - a (2 - a s) w_a w_b^T),   J~_v^T r~ = sqrt(rho') residual_scaling (1 - a s) w_v,
//     (J~ x).(J~ y) = rho' z_x^T Omega z_y with z_x = J x - a r (w . x)
// so the hot kernels need Omega only, never U.
APEX_HD bool between_linearize_weighted(const double* __restrict__ k0, const double* __restrict__ k1, const double* __restrict__ m,
                                        const PgLoss& loss, const double* __restrict__ W, double r[6], Jac6& J0, Jac6& J1, EdgeNormal6& n) {
    between_linearize(k0, k1, m, r, J0, J1);
    double Wr[6];
    info_mv<6>(W, r, Wr);
    n.s = fmax(dotn<6>(r, Wr), 0.0);
    n.c = pg_loss_corrector(loss, n.s);
    if (n.c.sqrt_rho1 == 0.0) return false;
    const double as = n.c.alpha_sq_norm * n.s;
    n.rho1 = n.c.sqrt_rho1 * n.c.sqrt_rho1;
    n.kap = n.c.alpha_sq_norm * (2.0 - as);
    n.gsc = n.c.sqrt_rho1 * n.c.residual_scaling * (1.0 - as);
    jtr(J0, Wr, n.w0);
    jtr(J1, Wr, n.w1);
    return true;
}

// PriorFactor on an SE3 variable (prior_factor.rs:96-108): r = to_vector(x) - data over the 7 stored doubles of the prepared
// pose (SE3::from(DVector).to_vector(), unit quaternion), J = the first six columns of I7; returns sqrt(rho') of the
// block's Huber loss
APEX_HD double prior_eval(const double* __restrict__ x7, const double* __restrict__ data7, double delta, double r[7]) {
    double s = 0.0;
#pragma unroll
    for (int a = 0; a < 7; ++a) { r[a] = x7[a] - data7[a]; s += r[a] * r[a]; }
    const double sc = pg_huber_scale(delta, s);
#pragma unroll
    for (int a = 0; a < 7; ++a) r[a] *= sc;
    return sc;
}

// What the manifold-generic kernels of pg_kernels.hip know about a vertex type: three sizes and forwarders to the math
// above.  Se2Manifold (pg2_device.hpp) and So3Manifold (pg_so3_device.hpp) are the others.  Each manifold keeps its own order of operations behind these
// names -- where the Huber factor is applied, how a prior's squares are added -- because the bits depend on it.
struct Se3Manifold {
    static constexpr int kDof = 6;      // tangent columns per vertex
    static constexpr int kAmb = 7;      // stored doubles per vertex / measurement / prior: t(3) q(4)
    static constexpr int kStride = 8;   // doubles per prepared pose / measurement: t(3) q(4) pad
    static constexpr int kPriorStride = kStride;   // doubles per prior block: data (kAmb) | the block's Huber delta
    static constexpr bool kPriorOnPrepared = true;   // the prior sees the normalised pose

    static APEX_HD void prepare(const double* __restrict__ v, double* __restrict__ o) { pose_normalise(v, o); }
    static APEX_HD void plus(const double* x, const double* d, double* o) { se3_plus(x, d, o); }
    static APEX_HD void residual(const double* __restrict__ k0, const double* __restrict__ k1, const double* __restrict__ m, double r[6]) {
        double tA[3], qA[4], D[9];
        between_residual(k0, k1, m, r, tA, qA, D);
    }
    static APEX_HD double prior_residual(const double* __restrict__ x, const double* __restrict__ data, double delta, double r[7]) {
        return prior_eval(x, data, delta, r);
    }
    static APEX_HD double cost_add_prior(double acc, const double r[7]) {   // one chain through the accumulator
#pragma unroll
        for (int a = 0; a < 7; ++a) acc += r[a] * r[a];
        return acc;
    }
    // u = J~0 a0 + J~1 a1, w = J~0 b0 + J~1 b1 for the corrected Jacobians J~ = sqrt(rho') [dr/dk0 | dr/dk1] of one edge
    // (the linearisation of k_pg_edges; a0 / b0: the six tangent entries of k0's vertex, a1 / b1 of k1's).  J = [P T; 0 P]:
    // J x = (P x_t + T x_r, P x_r).  sqrt(rho') multiplies the 12 products, not the 36 Jacobian entries.
    static APEX_HD void edge_jv(const double* __restrict__ k0, const double* __restrict__ k1, const double* __restrict__ m, double huber_delta,
                                const double a0[6], const double a1[6], const double b0[6], const double b1[6], double u[6], double w[6]) {
        double r[6];
        Jac6 J0, J1;
        between_linearize(k0, k1, m, r, J0, J1);
        const double sc = pg_huber_scale(huber_delta, r[0] * r[0] + r[1] * r[1] + r[2] * r[2] + r[3] * r[3] + r[4] * r[4] + r[5] * r[5]);
#pragma unroll
        for (int i = 0; i < 3; ++i) {
            double ut = 0.0, ur = 0.0, wt = 0.0, wr = 0.0;
#pragma unroll
            for (int j = 0; j < 3; ++j) {
                const double p0 = J0.P[3 * i + j], t0 = J0.T[3 * i + j], p1 = J1.P[3 * i + j], t1 = J1.T[3 * i + j];
                ut += (p0 * a0[j] + t0 * a0[3 + j]) + (p1 * a1[j] + t1 * a1[3 + j]);
                ur += p0 * a0[3 + j] + p1 * a1[3 + j];
                wt += (p0 * b0[j] + t0 * b0[3 + j]) + (p1 * b1[j] + t1 * b1[3 + j]);
                wr += p0 * b0[3 + j] + p1 * b1[3 + j];
            }
            u[i] = sc * ut; u[3 + i] = sc * ur; w[i] = sc * wt; w[3 + i] = sc * wr;
        }
    }
    // the same under the general loss: J~ x = sqrt(rho') (J x - a r (w . x)), w . x = w0 . x0 + w1 . x1 (EdgeNormal6)
    static APEX_HD void edge_jv(const double* __restrict__ k0, const double* __restrict__ k1, const double* __restrict__ m, const PgLoss& loss,
                                const double a0[6], const double a1[6], const double b0[6], const double b1[6], double u[6], double w[6]) {
        double r[6];
        Jac6 J0, J1;
        EdgeNormal6 n;
        if (!between_linearize_general(k0, k1, m, loss, r, J0, J1, n)) {
#pragma unroll
            for (int i = 0; i < 6; ++i) { u[i] = 0.0; w[i] = 0.0; }
            return;
        }
        double wa = 0.0, wb = 0.0;
#pragma unroll
        for (int i = 0; i < 6; ++i) { wa += n.w0[i] * a0[i] + n.w1[i] * a1[i]; wb += n.w0[i] * b0[i] + n.w1[i] * b1[i]; }
        const double sc = n.c.sqrt_rho1;
        wa *= n.c.alpha_sq_norm; wb *= n.c.alpha_sq_norm;
#pragma unroll
        for (int i = 0; i < 3; ++i) {
            double ut = 0.0, ur = 0.0, wt = 0.0, wr = 0.0;
#pragma unroll
            for (int j = 0; j < 3; ++j) {
                const double p0 = J0.P[3 * i + j], t0 = J0.T[3 * i + j], p1 = J1.P[3 * i + j], t1 = J1.T[3 * i + j];
                ut += (p0 * a0[j] + t0 * a0[3 + j]) + (p1 * a1[j] + t1 * a1[3 + j]);
                ur += p0 * a0[3 + j] + p1 * a1[3 + j];
                wt += (p0 * b0[j] + t0 * b0[3 + j]) + (p1 * b1[j] + t1 * b1[3 + j]);
                wr += p0 * b0[3 + j] + p1 * b1[3 + j];
            }
            u[i] = sc * (ut - r[i] * wa); u[3 + i] = sc * (ur - r[3 + i] * wa);
            w[i] = sc * (wt - r[i] * wb); w[3 + i] = sc * (wr - r[3 + i] * wb);
        }
    }
    // corrected residual [6] and Jacobian [6][12] = [dr/dk0 | dr/dk1] of one edge (either may be null) under the general
    // loss.  First arm: the legacy stores with sqrt(rho') (Huber through this path gives Huber's bits).  Second arm: the
    // literal J~ = sqrt(rho') (J - a r r^T J) (corrector.rs:241-253), dense -- this kernel is not hot.
    static APEX_HD void export_edge(const double* __restrict__ k0, const double* __restrict__ k1, const double* __restrict__ m,
                                    const PgLoss& loss, double* __restrict__ r_out, double* __restrict__ j_out) {
        double r[6];
        Jac6 J[2];
        between_linearize(k0, k1, m, r, J[0], J[1]);
        const double s = r[0] * r[0] + r[1] * r[1] + r[2] * r[2] + r[3] * r[3] + r[4] * r[4] + r[5] * r[5];
        const PgCorrector c = pg_loss_corrector(loss, s);
        const double sc = c.sqrt_rho1;
        if (r_out)
            for (int i = 0; i < 6; ++i) r_out[i] = c.residual_scaling * r[i];
        if (!j_out) return;
        double rtj[12];
        jtr(J[0], r, rtj);
        jtr(J[1], r, rtj + 6);
        for (int w = 0; w < 2; ++w)
            for (int i = 0; i < 3; ++i)
                for (int j = 0; j < 3; ++j) {
                    double* o = j_out + 6 * w;
                    if (c.alpha_sq_norm == 0.0) {
                        o[12 * i + j] = sc * J[w].P[3 * i + j];
                        o[12 * i + 3 + j] = sc * J[w].T[3 * i + j];
                        o[12 * (i + 3) + j] = 0.0;
                        o[12 * (i + 3) + 3 + j] = sc * J[w].P[3 * i + j];
                    } else {
                        const double a = c.alpha_sq_norm, wl = rtj[6 * w + j], wh = rtj[6 * w + 3 + j];
                        o[12 * i + j] = sc * (J[w].P[3 * i + j] - a * r[i] * wl);
                        o[12 * i + 3 + j] = sc * (J[w].T[3 * i + j] - a * r[i] * wh);
                        o[12 * (i + 3) + j] = sc * (0.0 - a * r[3 + i] * wl);
                        o[12 * (i + 3) + 3 + j] = sc * (J[w].P[3 * i + j] - a * r[3 + i] * wh);
                    }
                }
    }
    // With Omega (LossWeighted): u = sqrt(rho') z_a, w = sqrt(rho') z_b, z_x = J x - a r (w . x) -- corrected, not whitened; the
    // caller closes the products with Omega: (J~ a).(J~ b) = u^T Omega w.
    static APEX_HD void edge_jv_info(const double* __restrict__ k0, const double* __restrict__ k1, const double* __restrict__ m, const PgLoss& loss,
                                     const double* __restrict__ W, const double a0[6], const double a1[6], const double b0[6], const double b1[6],
                                     double u[6], double w[6]) {
        double r[6];
        Jac6 J0, J1;
        EdgeNormal6 n;
        if (!between_linearize_weighted(k0, k1, m, loss, W, r, J0, J1, n)) {
#pragma unroll
            for (int i = 0; i < 6; ++i) { u[i] = 0.0; w[i] = 0.0; }
            return;
        }
        double wa = 0.0, wb = 0.0;
#pragma unroll
        for (int i = 0; i < 6; ++i) { wa += n.w0[i] * a0[i] + n.w1[i] * a1[i]; wb += n.w0[i] * b0[i] + n.w1[i] * b1[i]; }
        const double sc = n.c.sqrt_rho1;
        wa *= n.c.alpha_sq_norm; wb *= n.c.alpha_sq_norm;
#pragma unroll
        for (int i = 0; i < 3; ++i) {
            double ut = 0.0, ur = 0.0, wt = 0.0, wr = 0.0;
#pragma unroll
            for (int j = 0; j < 3; ++j) {
                const double p0 = J0.P[3 * i + j], t0 = J0.T[3 * i + j], p1 = J1.P[3 * i + j], t1 = J1.T[3 * i + j];
                ut += (p0 * a0[j] + t0 * a0[3 + j]) + (p1 * a1[j] + t1 * a1[3 + j]);
                ur += p0 * a0[3 + j] + p1 * a1[3 + j];
                wt += (p0 * b0[j] + t0 * b0[3 + j]) + (p1 * b1[j] + t1 * b1[3 + j]);
                wr += p0 * b0[3 + j] + p1 * b1[3 + j];
            }
            u[i] = sc * (ut - r[i] * wa); u[3 + i] = sc * (ur - r[3 + i] * wa);
            w[i] = sc * (wt - r[i] * wb); w[3 + i] = sc * (wr - r[3 + i] * wb);
        }
    }
    // the literal whitened, corrected residual [6] and Jacobian [6][12] of one edge (info_export_block: factors Omega here)
    static APEX_HD void export_edge_info(const double* __restrict__ k0, const double* __restrict__ k1, const double* __restrict__ m,
                                         const PgLoss& loss, const double* __restrict__ W, double* __restrict__ r_out, double* __restrict__ j_out) {
        double r[6], Jd[72];
        Jac6 J[2];
        between_linearize(k0, k1, m, r, J[0], J[1]);
        for (int w = 0; w < 2; ++w)
            for (int i = 0; i < 3; ++i)
                for (int j = 0; j < 3; ++j) {
                    double* o = Jd + 6 * w;
                    o[12 * i + j] = J[w].P[3 * i + j];
                    o[12 * i + 3 + j] = J[w].T[3 * i + j];
                    o[12 * (i + 3) + j] = 0.0;
                    o[12 * (i + 3) + 3 + j] = J[w].P[3 * i + j];
                }
        info_export_block<6>(W, loss, r, Jd, r_out, j_out);
    }
    // corrected residual [6] and Jacobian [6][12] = [dr/dk0 | dr/dk1] of one edge (either may be null); sqrt(rho') is
    // applied at the store
    static APEX_HD void export_edge(const double* __restrict__ k0, const double* __restrict__ k1, const double* __restrict__ m,
                                    double huber_delta, double* __restrict__ r_out, double* __restrict__ j_out) {
        double r[6];
        Jac6 J[2];
        between_linearize(k0, k1, m, r, J[0], J[1]);
        const double sc = pg_huber_scale(huber_delta, r[0] * r[0] + r[1] * r[1] + r[2] * r[2] + r[3] * r[3] + r[4] * r[4] + r[5] * r[5]);
        if (r_out)
            for (int i = 0; i < 6; ++i) r_out[i] = sc * r[i];
        if (j_out)
            for (int w = 0; w < 2; ++w)
                for (int i = 0; i < 3; ++i)
                    for (int j = 0; j < 3; ++j) {
                        double* o = j_out + 6 * w;
                        o[12 * i + j] = sc * J[w].P[3 * i + j];
                        o[12 * i + 3 + j] = sc * J[w].T[3 * i + j];
                        o[12 * (i + 3) + j] = 0.0;
                        o[12 * (i + 3) + 3 + j] = sc * J[w].P[3 * i + j];
                    }
    }
};

// ---- the row-owned SE3 assembly (apexgpu_pg_set_option "row_owned_assembly") ---------------------------------
// One block-row of H and of g, owned by vertex v: the loop of k_pg6_assemble, host-compilable so that
// tests/host_harness_se3_row.cpp replays it.  The 6-DOF sibling of pg_row_assemble<M> (pg2_device.hpp) over the same lists
// (pg2_lists.h: CSR of the edges incident to each vertex, ascending edge index, a self-loop listed once).  Every edge of the
// list is re-linearised; H_vv and g_v accumulate in registers in list order; for an other endpoint u < v the full block of
// (v, u) goes to add_off(u, B) -- row v of the lower triangle has one writer, so a plain read-add-write there has no race and
// parallel edges sum in list order.
// Every product is formed by the operations of k_pg_edges / pg_edge_weighted (pg_kernels.hip) under the same policy LP --
// between_linearize scaled by pg_huber_scale, jtj and jtr | between_linearize_general, jtj, EdgeNormal6 |
// between_linearize_weighted, info_mul_jac, jt_mul, EdgeNormal6 -- and only the order in which the products of different edges
// are summed differs from the atomic scatter.  Hvv is filled in full; a caller that reads its lower triangle only lets the
// compiler drop the rest.  info: the packed Omega of every edge (InfoPack<6>), read by LossWeighted only.
template <class LP, typename AddOff>
APEX_HD void pg_row_assemble6(uint32_t v, const double* __restrict__ posep, const double* __restrict__ meas,
                              const uint32_t* __restrict__ e_from, const uint32_t* __restrict__ e_to,
                              const int* __restrict__ inc_ptr, const uint32_t* __restrict__ inc_edge,
                              const double* __restrict__ info, const typename LP::Param& loss, double Hvv[36], double gv[6],
                              AddOff add_off) {
    constexpr bool weighted = std::is_same<LP, LossWeighted>::value;
#pragma unroll
    for (int i = 0; i < 36; ++i) Hvv[i] = 0.0;
#pragma unroll
    for (int i = 0; i < 6; ++i) gv[i] = 0.0;
    for (int k = inc_ptr[v]; k < inc_ptr[v + 1]; ++k) {
        const uint32_t e = inc_edge[k], a = e_from[e], b = e_to[e];
        const double* k0 = posep + 8 * (size_t)a;
        const double* k1 = posep + 8 * (size_t)b;
        const double* m = meas + 8 * (size_t)e;
        double r[6];
        Jac6 J0, J1;
        [[maybe_unused]] EdgeNormal6 nf;
        [[maybe_unused]] double W[36];
        if constexpr (weighted) {
            info_unpack<6>(info + InfoPack<6>::kStride * (size_t)e, W);
            if (!between_linearize_weighted(k0, k1, m, loss, W, r, J0, J1, nf)) continue;   // (rho' = 0: nothing)
        } else if constexpr (LP::kGeneral) {
            if (!between_linearize_general(k0, k1, m, loss, r, J0, J1, nf)) continue;
        } else {
            between_linearize(k0, k1, m, r, J0, J1);
            const double sc = pg_huber_scale(loss, r[0] * r[0] + r[1] * r[1] + r[2] * r[2] + r[3] * r[3] + r[4] * r[4] + r[5] * r[5]);
            if (sc != 1.0) {
#pragma unroll
                for (int i = 0; i < 6; ++i) r[i] *= sc;
#pragma unroll
                for (int i = 0; i < 9; ++i) { J0.P[i] *= sc; J0.T[i] *= sc; J1.P[i] *= sc; J1.T[i] *= sc; }
            }
        }
        // G = A^T B (A^T Omega B under LossWeighted), corrected: the block of row A's vertex and column B's vertex
        const auto block = [&](const Jac6& A, const double* wa, const Jac6& B, const double* wb, double G[36]) {
            if constexpr (weighted) {
                double M[36];
                info_mul_jac(W, B, M);
                jt_mul(A, M, G);
            } else {
                jtj(A, B, G);
            }
            if constexpr (LP::kGeneral) nf.correct(G, wa, wb);
        };
        const auto gradient = [&](const Jac6& A, const double* wa, double gt[6]) {
            if constexpr (LP::kGeneral) nf.grad(wa, gt);
            else jtr(A, r, gt);
        };
        double G[36], gt[6];
        if (a == b) {   // self-loop: G_00 + G_11 + G_01 + G_01^T on the diagonal block, both gradient segments on g_v
            block(J0, nf.w0, J0, nf.w0, G);
#pragma unroll
            for (int i = 0; i < 36; ++i) Hvv[i] += G[i];
            block(J1, nf.w1, J1, nf.w1, G);
#pragma unroll
            for (int i = 0; i < 36; ++i) Hvv[i] += G[i];
            block(J0, nf.w0, J1, nf.w1, G);
#pragma unroll
            for (int i = 0; i < 6; ++i)
#pragma unroll
                for (int j = 0; j < 6; ++j) Hvv[6 * i + j] += G[6 * i + j] + G[6 * j + i];
            gradient(J0, nf.w0, gt);
#pragma unroll
            for (int i = 0; i < 6; ++i) gv[i] += gt[i];
            gradient(J1, nf.w1, gt);
#pragma unroll
            for (int i = 0; i < 6; ++i) gv[i] += gt[i];
            continue;
        }
        const bool first = a == v;   // (selects, not pointers into the register arrays: no scratch)
        const uint32_t u = first ? b : a;
        Jac6 Jv, Ju;
#pragma unroll
        for (int i = 0; i < 9; ++i) {
            Jv.P[i] = first ? J0.P[i] : J1.P[i]; Jv.T[i] = first ? J0.T[i] : J1.T[i];
            Ju.P[i] = first ? J1.P[i] : J0.P[i]; Ju.T[i] = first ? J1.T[i] : J0.T[i];
        }
        [[maybe_unused]] double wv[6], wu[6];
        if constexpr (LP::kGeneral) {
#pragma unroll
            for (int i = 0; i < 6; ++i) { wv[i] = first ? nf.w0[i] : nf.w1[i]; wu[i] = first ? nf.w1[i] : nf.w0[i]; }
        }
        block(Jv, wv, Jv, wv, G);
#pragma unroll
        for (int i = 0; i < 36; ++i) Hvv[i] += G[i];
        gradient(Jv, wv, gt);
#pragma unroll
        for (int i = 0; i < 6; ++i) gv[i] += gt[i];
        if (u < v) {   // row v, column u: J_v^T (Omega) J_u -- the transposed Jacobian is the row vertex's
            block(Jv, wv, Ju, wu, G);
            add_off(u, G);
        }
    }
}

}  // namespace apex
