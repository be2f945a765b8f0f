// pg_kernels.h -- launchers of the pose-graph kernels (pg_kernels.hip; BASELINE.json configs[1]).  Every launcher that
// depends on what a vertex is takes the manifold and picks the instantiation (Se3Manifold | Se2Manifold | So3Manifold) itself.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "ba_kernels.h"
#include "pg_loss.hpp"

namespace apex {

enum PgManifold { kManifoldSE3 = 0, kManifoldSE2 = 1, kManifoldSO3 = 2 };
// The 3-DOF manifolds (48 vertices per tile) are always assembled row-owned over the incident-edge lists of pg2_lists.h, with
// their prior blocks sorted by vertex; SE3 is assembled edge-major with atomics unless its handle was given the option
// "row_owned_assembly" (PoseGraphSolver::row_owned_: the property of the handle that the lists, the views, the prior order
// and launch_pg_assemble follow -- this function answers for the manifold alone).
inline bool pg_row_owned(int manifold) { return manifold == kManifoldSE2 || manifold == kManifoldSO3; }

// Read-only view of one parameter set + the edge list (internal vertex numbering).  Sizes per manifold (SE3 | SE2 | SO3):
// amb = 7 | 3 | 4 stored doubles per vertex, stride = 8 | 4 | 4 doubles per prepared pose and measurement, prior stride =
// 8 | 4 | 6 doubles per prior block.
struct PGView {
    int64_t n_v, n_e;
    const double* posep;     // [n_v][stride] prepared poses: t, unit quaternion, pad | x y cos sin | unit quaternion
    const uint32_t* e_from;  // [n_e] k0 of BetweenFactor
    const uint32_t* e_to;    // [n_e] k1
    const double* meas;      // [n_e][stride] prepared measurements
    double huber_delta;      // <= 0: no loss function
    // PriorFactor blocks (prior_factor.rs:96-108): r = to_vector(x_v) - data, amb rows.  SE3: the caller's order (row-owned
    // handle: sorted by vertex, stable), x_v the prepared pose, J = the first six columns of I7.  SE2: sorted by vertex (stable), x_v = [x, y, theta], J = I3.  SO3: sorted
    // by vertex (stable), x_v the prepared quaternion, J = the first three columns of I4.
    int n_prior = 0;
    const uint32_t* prior_v = nullptr;    // [n_prior] vertex (device order)
    const double* prior_data = nullptr;   // [n_prior][prior stride]: data (amb) | the block's Huber delta (<= 0: none)
    // row-owned handles only (null on an SE3 handle without the option "row_owned_assembly")
    const double* poses = nullptr;        // [n_v][amb] the stored vertices (what an SE2 prior sees: x y theta)
    const int* inc_ptr = nullptr;         // [n_v + 1] incident-edge CSR of the row-owned assembly (pg2_lists.h)
    const uint32_t* inc_edge = nullptr;
    const int* prior_slot = nullptr;      // [n_prior] the caller's index of the block (export order)
    // Edge information matrices (apexgpu_pg_set_information): [n_e][InfoPack<dof>::kStride] the packed upper
    // triangle of every edge's Omega, the caller's edge order; null: none.  Non-null selects the LossWeighted instantiations,
    // which read the loss from `loss` below whatever its kind (PoseGraphSolver::view puts no loss, L2 and Huber there as well).
    // (Ahead of `loss`: the struct's tail keeps its layout against the kernel arguments behind it, and the instruction stream
    // of the other instantiations differs from what it was in kernel-argument offsets only.)
    const double* info = nullptr;
    // The loss of every BetweenFactor block when apexgpu_pg_set_loss gave one that huber_delta cannot express
    // (kind != kLossNone): the launchers below then run the general-loss instantiation of every per-edge kernel and
    // huber_delta is not read for the edges.  kLossNone: the instantiations that know huber_delta only -- the code and the
    // bits of a handle that never heard of a loss (PoseGraphSolver::view sends no loss, L2 and Huber there too).
    PgLoss loss;
};

// Every launcher below that linearises edges (assemble, cost, export, jv_gram) also picks the loss policy (pg_device.hpp):
// LossWeighted when v.info is set, else LossLegacy | LossGeneral from v.loss.kind.
void launch_pg_prepare(int manifold, int64_t n, const double* poses, double* posep, hipStream_t s);
// H (tiles, lower triangle) += J^T J, g += J^T r over the edges, then the prior blocks' J^T J (sc^2 on the diagonal entries
// of the vertex) and J^T r; tiles and g zeroed by the caller.  Two launches, and two algorithms:
//   row_owned false (SE3 only)  k_pg_edges + k_pg_priors   edge-major, fp64 atomics, priors in the caller's order
//   row_owned true   SE2, SO3   k_pg2_assemble + k_pg2_priors   no atomics, a fixed order of summation per destination
//                    SE3        k_pg6_assemble + k_pg2_priors   the same over 6 x 6 blocks
// row_owned is the handle's property: the view must carry inc_ptr / inc_edge and priors sorted by vertex when it is true.
void launch_pg_assemble(int manifold, bool row_owned, const PGView& v, const TileMap& tm, double* g, hipStream_t s);
// corrected prior residuals [n_prior][amb], the caller's order
void launch_pg_prior_export(int manifold, const PGView& v, double* r_out, hipStream_t s);
void launch_pg_cost(int manifold, const PGView& v, double* partial, int n_partial, double* out_sumsq, hipStream_t s);
void launch_pg_retract(int manifold, int64_t n_v, const double* poses, const double* d, double sign, const uint8_t* fix,
                       double* poses_out, hipStream_t s);
void launch_pg_negate(int64_t n, const double* x, double* y, hipStream_t s);
// corrected residuals [n_e][dof] and Jacobians [n_e][dof][2 dof] = [dr/dk0 | dr/dk1] in the kernel's edge order
void launch_pg_export(int manifold, const PGView& v, double* r_out, double* j_out, hipStream_t s);
// Dog-Leg's products with H = J^T J (dog_leg.rs:776-803, 948-960): partial[n_partial * 3], fixed order.
// out3 = {|J a|^2, (J a).(J b), |J b|^2} over the edges and priors of v; a, b [dof n_v] in internal column order
void launch_pg_jv_gram(int manifold, const PGView& v, const double* a, const double* b, double* partial, int n_partial,
                       double* out3, hipStream_t s);

}  // namespace apex
