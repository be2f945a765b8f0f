// pg2_kernels.h -- launchers of the SE2 pose-graph kernels (pg2_kernels.hip).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "ba_kernels.h"

namespace apex {

constexpr int kVertsPerTile2 = kNB / 3;   // 48 vertices per 144-row tile

// Read-only view of one parameter set + the edge list (internal vertex numbering).
struct PG2View {
    int64_t n_v, n_e;
    const double* poses;     // [n_v][3] x y theta (what the prior sees)
    const double* posep;     // [n_v][4] prepared poses: x y cos sin
    const uint32_t* e_from;  // [n_e] k0 of BetweenFactor
    const uint32_t* e_to;    // [n_e] k1
    const double* meas;      // [n_e][4] prepared measurements
    double huber_delta;      // <= 0: no loss function
    const int* inc_ptr;      // [n_v + 1] incident-edge CSR (pg2_lists.h)
    const uint32_t* inc_edge;
    // PriorFactor blocks, sorted by vertex (stable): r = [x, y, theta] - data, J = I3
    int n_prior = 0;
    const uint32_t* prior_v = nullptr;    // [n_prior] vertex (device order), ascending
    const double* prior_data = nullptr;   // [n_prior][4]: data (3) | the block's Huber delta (<= 0: none)
    const int* prior_slot = nullptr;      // [n_prior] the caller's index of the block (export order)
};

void launch_pg2_prepare(int64_t n, const double* poses3, double* posep, hipStream_t s);
// H (tiles, lower triangle) += J^T J, g = J^T r, row-owned: no atomics, a fixed order of summation per destination
void launch_pg2_assemble(const PG2View& v, const TileMap& tm, double* g, hipStream_t s);
// the prior blocks' J^T J (sc^2 on the three diagonal entries of the vertex) and J^T r; after launch_pg2_assemble
void launch_pg2_priors(const PG2View& v, const TileMap& tm, double* g, hipStream_t s);
void launch_pg2_prior_export(const PG2View& v, double* r3_out, hipStream_t s);
void launch_pg2_cost(const PG2View& v, double* partial, int n_partial, double* out_sumsq, hipStream_t s);
void launch_pg2_retract(int64_t n_v, const double* poses, const double* d, double sign, const uint8_t* fix,
                        double* poses_out, hipStream_t s);
// corrected residuals [n_e][3] and Jacobians [n_e][3][6] = [dr/dk0 | dr/dk1] in edge order
void launch_pg2_export(const PG2View& v, double* r_out, double* j_out, hipStream_t s);

}  // namespace apex
