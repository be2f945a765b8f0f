// pg2_kernels.hip -- SE2 pose-graph kernels: BetweenFactor<SE2> linearisation fused with a row-owned block-sparse
// J^T J / J^T r assembly, trial cost, retraction.
//
//   k_pg2_prepare       vertex-major  x y cos sin of a parameter set (SE2::from(DVector))
//   k_pg2_assemble      vertex-major  lane v walks the edges incident to v (pg2_assemble_row): H_vv and g_v in registers,
//                                     blocks (v, u), u < v, by plain read-add-write -- row v of the lower triangle has
//                                     one writer, so there are no atomics and every sum has a fixed order: two
//                                     assemblies of one state are bit-identical.  An edge is linearised by both of its
//                                     endpoints (a few dozen flops) instead of scattering 24-byte segments atomically.
//   k_pg2_priors        one lane per run of prior blocks on one vertex (the blocks arrive sorted by vertex)
//   k_pg2_cost_partial  edge-major    1/2 |r~|^2 at a (trial) parameter set, the reduction tree of k_pg_cost_partial
//   k_pg2_retract       vertex-major  x (+) d with the fixed-DOF mask (src/core/problem.rs:185-197)
//   k_pg2_export        edge-major    parity exports
#include <hip/hip_runtime.h>

#include "pg2_device.hpp"
#include "pg2_kernels.h"

namespace apex {

__device__ __forceinline__ double pg2_block_sum_256(double v, double* scratch) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off, 64);
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    if (lane == 0) scratch[w] = v;
    __syncthreads();
    double r = 0.0;
    if (threadIdx.x == 0) r = (scratch[0] + scratch[1]) + (scratch[2] + scratch[3]);
    __syncthreads();
    return r;
}

__global__ __launch_bounds__(256) void k_pg2_prepare(int64_t n, const double* __restrict__ poses3, double* __restrict__ posep) {
    const int64_t v = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (v >= n) return;
    const double p[3] = {poses3[3 * v], poses3[3 * v + 1], poses3[3 * v + 2]};
    double o[4];
    se2_prepare(p, o);
    double2* q = reinterpret_cast<double2*>(posep + kPose2Stride * v);
    q[0] = make_double2(o[0], o[1]);
    q[1] = make_double2(o[2], o[3]);
}

// 3x3 block (row vertex vr, column vertex vc, vr >= vc) of the lower-triangular tile matrix
__device__ __forceinline__ double* h2_block_ptr(const TileMap& tm, uint32_t vr, uint32_t vc) {
    const uint32_t I = vr / kVertsPerTile2, J = vc / kVertsPerTile2;
    const int slot = tm.slot[(size_t)I * tm.nt + J];
    return tm.tiles + (size_t)slot * (kNB * kNB) + (size_t)((vr % kVertsPerTile2) * 3) * kNB + (vc % kVertsPerTile2) * 3;
}

__global__ __launch_bounds__(256) void k_pg2_assemble(PG2View v, TileMap tm, double* __restrict__ g) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= v.n_v) return;
    const uint32_t row = (uint32_t)i;
    double H[9], gv[3];
    pg2_assemble_row(row, v.posep, v.meas, v.e_from, v.e_to, v.inc_ptr, v.inc_edge, v.huber_delta, H, gv,
                     [&](uint32_t u, const double* B) {
                         double* blk = h2_block_ptr(tm, row, u);
#pragma unroll
                         for (int a = 0; a < 3; ++a)
#pragma unroll
                             for (int b = 0; b < 3; ++b) blk[a * kNB + b] += B[3 * a + b];
                     });
    double* blk = h2_block_ptr(tm, row, row);   // (on top of the damping add_diag has put there)
#pragma unroll
    for (int a = 0; a < 3; ++a)
#pragma unroll
        for (int b = 0; b <= a; ++b) blk[a * kNB + b] += H[3 * a + b];
#pragma unroll
    for (int a = 0; a < 3; ++a) g[3 * (size_t)row + a] = gv[a];
}

__device__ __forceinline__ double prior2_at(const PG2View& v, int k, double r[3]) {
    const uint32_t a = v.prior_v[k];
    const double x[3] = {v.poses[3 * (size_t)a], v.poses[3 * (size_t)a + 1], v.poses[3 * (size_t)a + 2]};
    const double* d = v.prior_data + kPose2Stride * (size_t)k;
    const double dd[3] = {d[0], d[1], d[2]};
    return prior2_eval(x, dd, d[3], r);
}
__global__ __launch_bounds__(64) void k_pg2_priors(PG2View v, TileMap tm, double* __restrict__ g) {
    const int k = blockIdx.x * 64 + threadIdx.x;
    if (k >= v.n_prior) return;
    const uint32_t a = v.prior_v[k];
    if (k > 0 && v.prior_v[k - 1] == a) return;   // the first block of a vertex sums the whole run, in order
    double h = 0.0, gv[3] = {0.0, 0.0, 0.0};
    for (int j = k; j < v.n_prior && v.prior_v[j] == a; ++j) {
        double r[3];
        const double sc = prior2_at(v, j, r);     // J~ = sc I3: J~^T J~ = sc^2 I3, J~^T r~ = sc r~
        h += sc * sc;
#pragma unroll
        for (int i = 0; i < 3; ++i) gv[i] += sc * r[i];
    }
    double* blk = h2_block_ptr(tm, a, a);
#pragma unroll
    for (int i = 0; i < 3; ++i) {
        blk[i * kNB + i] += h;
        g[3 * (size_t)a + i] += gv[i];
    }
}
__global__ __launch_bounds__(64) void k_pg2_prior_export(PG2View v, double* __restrict__ r3_out) {
    const int k = blockIdx.x * 64 + threadIdx.x;
    if (k >= v.n_prior) return;
    double r[3];
    (void)prior2_at(v, k, r);
    const int o = v.prior_slot[k];
    for (int a = 0; a < 3; ++a) r3_out[3 * o + a] = r[a];
}

__device__ __forceinline__ void load_pose4(const double* __restrict__ base, int64_t i, double p[4]) {
    const double2* q = reinterpret_cast<const double2*>(base + kPose2Stride * i);
    const double2 a = q[0], b = q[1];
    p[0] = a.x; p[1] = a.y; p[2] = b.x; p[3] = b.y;
}

__global__ __launch_bounds__(256) void k_pg2_cost_partial(PG2View v, double* __restrict__ partial) {
    __shared__ double scratch[4];
    double acc = 0.0;
    if (blockIdx.x == 0)
        for (int k = threadIdx.x; k < v.n_prior; k += 256) {
            double r[3];
            (void)prior2_at(v, k, r);
            acc += r[0] * r[0] + r[1] * r[1] + r[2] * r[2];
        }
    for (int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x; e < v.n_e; e += (int64_t)gridDim.x * 256) {
        double k0[4], k1[4], m[4], r[3], A[4];
        load_pose4(v.posep, v.e_from[e], k0);
        load_pose4(v.posep, v.e_to[e], k1);
        load_pose4(v.meas, e, m);
        between2_residual(k0, k1, m, r, A);
        const double s = r[0] * r[0] + r[1] * r[1] + r[2] * r[2];
        const double sc = pg_huber_scale(v.huber_delta, s);
        acc += (sc * sc) * s;
    }
    acc = pg2_block_sum_256(acc, scratch);
    if (threadIdx.x == 0) partial[blockIdx.x] = acc;
}

__global__ __launch_bounds__(256) void k_pg2_retract(int64_t n_v, const double* __restrict__ poses,
                                                       const double* __restrict__ d, double sign,
                                                       const uint8_t* __restrict__ fix, double* __restrict__ poses_out) {
    const int64_t v = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (v >= n_v) return;
    double dd[3], p[3], o[3];
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        dd[a] = fix[3 * v + a] ? 0.0 : sign * d[3 * v + a];
        p[a] = poses[3 * v + a];
    }
    se2_plus(p, dd, o);
#pragma unroll
    for (int a = 0; a < 3; ++a) poses_out[3 * v + a] = o[a];
}

__global__ __launch_bounds__(256) void k_pg2_export(PG2View v, double* __restrict__ r_out, double* __restrict__ j_out) {
    const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (e >= v.n_e) return;
    double k0[4], k1[4], m[4], r[3], J0[9], J1[9];
    load_pose4(v.posep, v.e_from[e], k0);
    load_pose4(v.posep, v.e_to[e], k1);
    load_pose4(v.meas, e, m);
    between2_corrected(k0, k1, m, v.huber_delta, r, J0, J1);
    if (r_out)
        for (int i = 0; i < 3; ++i) r_out[3 * e + i] = r[i];
    if (j_out)
        for (int i = 0; i < 3; ++i)
            for (int j = 0; j < 3; ++j) {
                j_out[18 * e + 6 * i + j] = J0[3 * i + j];
                j_out[18 * e + 6 * i + 3 + j] = J1[3 * i + j];
            }
}

static inline int grid256(int64_t n) { return (int)((n + 255) / 256); }

void launch_pg2_prepare(int64_t n, const double* poses3, double* posep, hipStream_t s) {
    if (n > 0) hipLaunchKernelGGL(k_pg2_prepare, dim3(grid256(n)), dim3(256), 0, s, n, poses3, posep);
}
void launch_pg2_assemble(const PG2View& v, const TileMap& tm, double* g, hipStream_t s) {
    if (v.n_v > 0) hipLaunchKernelGGL(k_pg2_assemble, dim3(grid256(v.n_v)), dim3(256), 0, s, v, tm, g);
}
void launch_pg2_priors(const PG2View& v, const TileMap& tm, double* g, hipStream_t s) {
    if (v.n_prior > 0) hipLaunchKernelGGL(k_pg2_priors, dim3((v.n_prior + 63) / 64), dim3(64), 0, s, v, tm, g);
}
void launch_pg2_prior_export(const PG2View& v, double* r3_out, hipStream_t s) {
    if (v.n_prior > 0) hipLaunchKernelGGL(k_pg2_prior_export, dim3((v.n_prior + 63) / 64), dim3(64), 0, s, v, r3_out);
}
void launch_pg2_cost(const PG2View& v, double* partial, int n_partial, double* out_sumsq, hipStream_t s) {
    hipLaunchKernelGGL(k_pg2_cost_partial, dim3(n_partial), dim3(256), 0, s, v, partial);
    launch_sum_partials(partial, n_partial, 1, out_sumsq, s);
}
void launch_pg2_retract(int64_t n_v, const double* poses, const double* d, double sign, const uint8_t* fix,
                        double* poses_out, hipStream_t s) {
    if (n_v > 0) hipLaunchKernelGGL(k_pg2_retract, dim3(grid256(n_v)), dim3(256), 0, s, n_v, poses, d, sign, fix, poses_out);
}
void launch_pg2_export(const PG2View& v, double* r_out, double* j_out, hipStream_t s) {
    if (v.n_e > 0) hipLaunchKernelGGL(k_pg2_export, dim3(grid256(v.n_e)), dim3(256), 0, s, v, r_out, j_out);
}

}  // namespace apex
