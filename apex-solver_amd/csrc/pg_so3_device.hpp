// pg_so3_device.hpp -- per-edge SO3 pose-graph math (rotation averaging) behind the kernels of pg_kernels.hip, and
// So3Manifold, the trait through which the manifold-generic kernels and the row-owned assembly (pg2_device.hpp) reach it.
//
// APEX_HD (host+device) like pg2_device.hpp, so tests/host_harness_so3.cpp runs the same code on the CPU.
//
// Reference semantics (file:line under the apex-solver tree):
//   SO3 = unit quaternion, vector form [qw, qx, qy, qz]           crates/apex-manifolds/src/so3.rs:210-213, 225-229
//   inverse / compose and their Jacobians (Adj(R) = R)            so3.rs:254-299
//   log: sin^2 against SMALL_ANGLE_THRESHOLD, the cos < 0 arm     so3.rs:313-357, crates/apex-manifolds/src/lib.rs:61
//   exp: from_scaled_axis | (1, theta / 2) normalised             so3.rs:558-577
//   right_jacobian_inv = left_jacobian_inv^T                      so3.rs:618-644
//   LieGroup::between, right plus                                 lib.rs:401-419, 269-283
//   BetweenFactor<SO3>::linearize                                 src/factors/between_factor.rs:268-322
//       r = Log((k1^-1 k0) * meas),  dr/dk0 = Jr^-1(r) Adj(meas^-1),
//       dr/dk1 = Jr^-1(r) (Adj(meas^-1) (-Adj((k1^-1 k0)^-1)))
//   PriorFactor on an SO3 variable (4 rows over 3 columns)        src/factors/prior_factor.rs:96-108,
//                                                                 src/linearizer/cpu/sparse.rs:201-204
//
// A vertex, a measurement and a prior datum are the four doubles [qw, qx, qy, qz]; a prepared one is the same quaternion
// normalised with the operations of SE3's pose_normalise (quat_normalise_twice), so an SE3 pose and an SO3 vertex with the
// same quaternion prepare to the same bits.  Tangents are [theta_x, theta_y, theta_z]; Jacobians are dense row-major 3 x 3.
// so3_log, so3_left_jacobian_inv and the quaternion helpers are those of SE3's rotational block (pg_device.hpp,
// ba_device.hpp); the loss and information corrections are block3_correct / block3_weight of pg2_device.hpp.
#pragma once
#include "pg2_device.hpp"

namespace apex {

constexpr int kRot3Stride = 4;        // doubles per prepared SO3 vertex / measurement: 32 bytes, two 16-byte loads
constexpr int kRot3PriorStride = 6;   // doubles per prior block: the datum (4) | the block's Huber delta | pad to 16 bytes

APEX_HD void quat_conj(const double q[4], double o[4]) { o[0] = q[0]; o[1] = -q[1]; o[2] = -q[2]; o[3] = -q[3]; }

// residual only: r = Log((k1^-1 k0) * meas) on prepared (unit) quaternions; A = k1^-1 k0 is handed back for the Jacobians.
// The quaternion products are those of SE3's between_residual (se3_inv / se3_mul on the rotational part).
APEX_HD void between_so3_residual(const double* __restrict__ k0, const double* __restrict__ k1, const double* __restrict__ m,
                                  double r[3], double A[4]) {
    double k1i[4], D[4];
    quat_conj(k1, k1i);
    quat_mul(k1i, k0, A);
    quat_mul(A, m, D);
    so3_log(D, r);
}

// residual + both Jacobians (row-major 3 x 3), the chain J_log * J_compose * J_between as the factor multiplies it.
// Adj of a rotation is its matrix: Adj(meas^-1) = R(meas)^T = R(conj meas).
APEX_HD void between_so3_linearize(const double* __restrict__ k0, const double* __restrict__ k1, const double* __restrict__ m,
                                   double r[3], double J0[9], double J1[9]) {
    double A[4], qi[4], Jl[9], Jr[9], Rm[9], Ra[9], C[9];
    between_so3_residual(k0, k1, m, r, A);
    so3_left_jacobian_inv(r, Jl);   // Jr^-1 = (Jl^-1)^T; below the threshold I - 1/2 [r]x, transposed I + 1/2 [r]x
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
        for (int j = 0; j < 3; ++j) Jr[3 * i + j] = Jl[3 * j + i];
    quat_conj(m, qi);
    quat_to_rot(qi, Rm);            // d(A m)/dA
    quat_conj(A, qi);
    quat_to_rot(qi, Ra);            // dA/dk1 = -Adj(A^-1), dA/dk0 = I
#pragma unroll
    for (int i = 0; i < 9; ++i) Ra[i] = -Ra[i];
    m3_mul(Rm, Ra, C);
    m3_mul(Jr, Rm, J0);
    m3_mul(Jr, C, J1);
}

// PriorFactor on an SO3 variable: r = coeffs(x) - data over the four stored doubles of the prepared quaternion, J = the first
// three columns of I4 (the scatter view truncates the 4 x 4 identity, as it truncates SE3's 7 x 7); returns sqrt(rho') of the
// block's Huber loss.  The counterpart of prior_eval.
APEX_HD double prior_so3_eval(const double* __restrict__ x4, const double* __restrict__ data4, double delta, double r[4]) {
    double s = 0.0;
#pragma unroll
    for (int a = 0; a < 4; ++a) { r[a] = x4[a] - data4[a]; s += r[a] * r[a]; }
    const double sc = pg_huber_scale(delta, s);
#pragma unroll
    for (int a = 0; a < 4; ++a) r[a] *= sc;
    return sc;
}

// x (+) d = x * Exp(d) on the stored quaternion as it is, stored as the product gives it (not re-normalised: se3_plus keeps its
// quaternion the same way).  x (+) 0 = x: a vertex that does not move keeps its bits (all three DOF fixed).
APEX_HD void so3_plus(const double* __restrict__ q4, const double d[3], double* __restrict__ o4) {
    if (d[0] == 0.0 && d[1] == 0.0 && d[2] == 0.0) { o4[0] = q4[0]; o4[1] = q4[1]; o4[2] = q4[2]; o4[3] = q4[3]; return; }
    double e[4];
    so3_exp(d, e);
    quat_mul(q4, e, o4);
}

// The SO3 side of the trait pg_device.hpp describes at Se3Manifold.  kStride is the vertex itself (4 doubles): a prior block
// needs a fifth double for its Huber delta, so it has a stride of its own instead of widening every pose and measurement to 6
// (96 instead of 144 bytes read per edge linearisation).
struct So3Manifold : Dof3EdgeOps<So3Manifold> {
    static constexpr int kDof = 3;                        // tangent columns per vertex
    static constexpr int kAmb = 4;                        // stored doubles per vertex / measurement / prior: qw qx qy qz
    static constexpr int kStride = kRot3Stride;           // doubles per prepared vertex / measurement
    static constexpr int kPriorStride = kRot3PriorStride; // doubles per prior block: data (kAmb) | the block's Huber delta | pad
    static constexpr bool kPriorOnPrepared = true;        // the prior sees the normalised quaternion

    static APEX_HD void prepare(const double* __restrict__ v, double* __restrict__ o) { quat_normalise_twice(v, o); }
    static APEX_HD void plus(const double* x, const double* d, double* o) { so3_plus(x, d, o); }
    static APEX_HD void residual(const double* __restrict__ k0, const double* __restrict__ k1, const double* __restrict__ m, double r[3]) {
        double A[4];
        between_so3_residual(k0, k1, m, r, A);
    }
    static APEX_HD void linearize(const double* __restrict__ k0, const double* __restrict__ k1, const double* __restrict__ m,
                                  double r[3], double J0[9], double J1[9]) {
        between_so3_linearize(k0, k1, m, r, J0, J1);
    }
    static APEX_HD double prior_residual(const double* __restrict__ x, const double* __restrict__ data, double delta, double r[4]) {
        return prior_so3_eval(x, data, delta, r);
    }
    static APEX_HD double cost_add_prior(double acc, const double r[4]) {   // all four rows, one chain through the accumulator (as SE3's seven)
#pragma unroll
        for (int a = 0; a < 4; ++a) acc += r[a] * r[a];
        return acc;
    }
};

}  // namespace apex
