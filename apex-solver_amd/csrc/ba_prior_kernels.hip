// ba_prior_kernels.hip -- PriorFactor blocks on camera poses and intrinsics (ba_prior_kernels.h).
//
//   k_ba_prior_eval        one lane per camera: its runs of pose and intrinsics blocks summed in list order
//   k_ba_prior_add_system  explicit S: tile diagonal, g_c += , g_red -=    (behind k_cam_reduce)
//   k_ba_prior_add_blocks  matrix-free: Schur-Jacobi blocks, g_c, g_red     (behind k_extract_diag_blocks)
//   k_ba_prior_matvec      y += P x                                         (behind k_implicit_matvec)
//   k_ba_prior_cost_add    the priors' partial slot of the cost             (behind k_cost_partial + k_sum_partials)
//   k_ba_prior_gram_add    Dog-Leg's three sums                             (behind k_ba_jv_gram)
//   k_ba_prior_export      corrected residuals, the caller's order
//
// The factor (src/factors/prior_factor.rs:93-105): r = to_vector(x) - data, J = I; the linearizer keeps the variable's tangent
// columns (sparse.rs:201-204), so a pose block is seven rows over six columns and its seventh row counts in the cost only.  The
// weight w (an addition: the reference's factor has unit information) scales r and J, then the block's Huber corrector scales
// both by sqrt(rho') with s = |w r|^2 over all rows: the corrected Jacobian is (sqrt(rho') w) [I; 0].
#include "ba_prior_kernels.h"

#include "ba_device.hpp"
#include "ba_dispatch.h"
#include "device_reduce.hpp"
#include "pg_device.hpp"

namespace apex {

// r~ of pose block k on the camera record q (BAView::camq: unit quaternion, t, f k1 k2); returns sqrt(rho') w
__device__ __forceinline__ double pose_prior_at(const double* __restrict__ q, const double* __restrict__ d, double r[7]) {
    const double w = d[8];
    const double x[7] = {q[4], q[5], q[6], q[0], q[1], q[2], q[3]};   // to_vector order: t, qw qx qy qz
    double s = 0.0;
#pragma unroll
    for (int a = 0; a < 7; ++a) { r[a] = w * (x[a] - d[a]); s += r[a] * r[a]; }
    const double sc = pg_huber_scale(d[7], s);
#pragma unroll
    for (int a = 0; a < 7; ++a) r[a] *= sc;
    return sc * w;
}

__device__ __forceinline__ double intr_prior_at(const double* __restrict__ q, const double* __restrict__ d, double r[3]) {
    const double w = d[4];
    double s = 0.0;
#pragma unroll
    for (int a = 0; a < 3; ++a) { r[a] = w * (q[7 + a] - d[a]); s += r[a] * r[a]; }
    const double sc = pg_huber_scale(d[3], s);
#pragma unroll
    for (int a = 0; a < 3; ++a) r[a] *= sc;
    return sc * w;
}

template <int DC>
__global__ __launch_bounds__(64) void k_ba_prior_eval(int64_t n_cam, const double* __restrict__ camq, BaPriorView pv,
                                                        double* __restrict__ pdiag, double* __restrict__ pg, double* __restrict__ pcost) {
    const int64_t c = (int64_t)blockIdx.x * 64 + threadIdx.x;
    if (c >= n_cam) return;
    const double* q = camq + (size_t)kCamQStride * c;
    double h[2] = {0.0, 0.0}, g[9] = {}, cost = 0.0;
    if (pv.n_pose > 0)
        for (int k = pv.pose_ptr[c]; k < pv.pose_ptr[c + 1]; ++k) {
            double r[7];
            const double j = pose_prior_at(q, pv.pose_data + (size_t)kPosePriorStride * k, r);
            h[0] += j * j;
#pragma unroll
            for (int a = 0; a < 6; ++a) g[a] += j * r[a];
#pragma unroll
            for (int a = 0; a < 7; ++a) cost += r[a] * r[a];
        }
    if (DC == 9 && pv.n_intr > 0)
        for (int k = pv.intr_ptr[c]; k < pv.intr_ptr[c + 1]; ++k) {
            double r[3];
            const double j = intr_prior_at(q, pv.intr_data + (size_t)kIntrPriorStride * k, r);
            h[1] += j * j;
#pragma unroll
            for (int a = 0; a < 3; ++a) { g[6 + a] += j * r[a]; cost += r[a] * r[a]; }
        }
    pcost[c] = cost;
    if (!pdiag) return;
#pragma unroll
    for (int a = 0; a < DC; ++a) {
        pdiag[(size_t)DC * c + a] = h[a < 6 ? 0 : 1];
        pg[(size_t)DC * c + a] = g[a];
    }
}

__global__ __launch_bounds__(256) void k_ba_prior_add_system(int64_t n_c, const double* __restrict__ pdiag, const double* __restrict__ pg,
                                                               TileMap tm, double* __restrict__ g_c, double* __restrict__ g_red) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n_c) return;
    const double p = pdiag[i];
    if (p == 0.0) return;   // (a camera without blocks: its entries keep their bits)
    const int I = (int)(i / kNB), r = (int)(i - (int64_t)I * kNB);
    tm.tiles[(size_t)tm.slot[(size_t)I * tm.nt + I] * (kNB * kNB) + (size_t)r * kNB + r] += p;
    const double g = pg[i];
    g_c[i] += g;
    g_red[i] -= g;   // (k_cam_reduce leaves the right-hand side: g_red = -(g_c - H_cl H_ll^-1 g_l))
}

template <int DC>
__global__ __launch_bounds__(256) void k_ba_prior_add_blocks(int64_t n_c, const double* __restrict__ pdiag, const double* __restrict__ pg,
                                                               double* __restrict__ sd, double* __restrict__ g_c, double* __restrict__ g_red) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n_c) return;
    const double p = pdiag[i];
    if (p == 0.0) return;
    const int64_t c = i / DC;
    const int a = (int)(i - c * DC);
    sd[(size_t)c * DC * DC + a * DC + a] += p;
    const double g = pg[i];
    g_c[i] += g;
    g_red[i] -= g;   // (k_cam_reduce leaves the right-hand side: g_red = -(g_c - H_cl H_ll^-1 g_l))
}

__global__ __launch_bounds__(256) void k_ba_prior_matvec(int64_t n_c, const double* __restrict__ pdiag, const double* __restrict__ x,
                                                           double* __restrict__ y) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n_c) return;
    const double p = pdiag[i];
    if (p != 0.0) y[i] += p * x[i];
}

__global__ __launch_bounds__(256) void k_ba_prior_cost_add(int64_t n_cam, const double* __restrict__ pcost, double* __restrict__ out) {
    __shared__ double scratch[4];
    double s = 0.0;
    for (int64_t c = threadIdx.x; c < n_cam; c += 256) s += pcost[c];
    s = block_sum_256(s, scratch);
    if (threadIdx.x == 0) out[0] += s;
}

__global__ __launch_bounds__(256) void k_ba_prior_gram_add(int64_t n_c, const double* __restrict__ pdiag, const double* __restrict__ a,
                                                             const double* __restrict__ b, double* __restrict__ out3) {
    __shared__ double scratch[4];
    double aa = 0.0, ab = 0.0, bb = 0.0;
    for (int64_t i = threadIdx.x; i < n_c; i += 256) {
        const double p = pdiag[i], ai = a[i], bi = b[i];
        aa += p * ai * ai; ab += p * ai * bi; bb += p * bi * bi;
    }
    aa = block_sum_256(aa, scratch);
    ab = block_sum_256(ab, scratch);
    bb = block_sum_256(bb, scratch);
    if (threadIdx.x == 0) { out3[0] += aa; out3[1] += ab; out3[2] += bb; }
}

// block k of either set (pose blocks first) to the caller's slot
__global__ __launch_bounds__(64) void k_ba_prior_export(const double* __restrict__ camq, BaPriorView pv, double* __restrict__ pose_out,
                                                          double* __restrict__ intr_out) {
    const int k = blockIdx.x * 64 + threadIdx.x;
    if (k < pv.n_pose) {
        if (!pose_out) return;
        double r[7];
        (void)pose_prior_at(camq + (size_t)kCamQStride * pv.pose_cam[k], pv.pose_data + (size_t)kPosePriorStride * k, r);
        double* o = pose_out + 7 * (size_t)pv.pose_slot[k];
#pragma unroll
        for (int a = 0; a < 7; ++a) o[a] = r[a];
    } else if (k < pv.n_pose + pv.n_intr) {
        if (!intr_out) return;
        const int j = k - pv.n_pose;
        double r[3];
        (void)intr_prior_at(camq + (size_t)kCamQStride * pv.intr_cam[j], pv.intr_data + (size_t)kIntrPriorStride * j, r);
        double* o = intr_out + 3 * (size_t)pv.intr_slot[j];
#pragma unroll
        for (int a = 0; a < 3; ++a) o[a] = r[a];
    }
}

static unsigned grid_of(int64_t n, int block) { return (unsigned)((n + block - 1) / block); }

void launch_ba_prior_eval(int dc, int64_t n_cam, const double* camq, const BaPriorView& pv, double* pdiag, double* pg, double* pcost, hipStream_t s) {
    with_dc(dc, [&](auto DC) {
        hipLaunchKernelGGL(k_ba_prior_eval<DC()>, dim3(grid_of(n_cam, 64)), dim3(64), 0, s, n_cam, camq, pv, pdiag, pg, pcost);
    });
}
void launch_ba_prior_add_system(int64_t n_c, const double* pdiag, const double* pg, const TileMap& tm, double* g_c, double* g_red, hipStream_t s) {
    hipLaunchKernelGGL(k_ba_prior_add_system, dim3(grid_of(n_c, 256)), dim3(256), 0, s, n_c, pdiag, pg, tm, g_c, g_red);
}
void launch_ba_prior_add_blocks(int dc, int64_t n_cam, const double* pdiag, const double* pg, double* sd, double* g_c, double* g_red, hipStream_t s) {
    const int64_t n_c = n_cam * dc;
    with_dc(dc, [&](auto DC) {
        hipLaunchKernelGGL(k_ba_prior_add_blocks<DC()>, dim3(grid_of(n_c, 256)), dim3(256), 0, s, n_c, pdiag, pg, sd, g_c, g_red);
    });
}
void launch_ba_prior_matvec(int64_t n_c, const double* pdiag, const double* x, double* y, hipStream_t s) {
    hipLaunchKernelGGL(k_ba_prior_matvec, dim3(grid_of(n_c, 256)), dim3(256), 0, s, n_c, pdiag, x, y);
}
void launch_ba_prior_cost_add(int64_t n_cam, const double* pcost, double* out, hipStream_t s) {
    hipLaunchKernelGGL(k_ba_prior_cost_add, dim3(1), dim3(256), 0, s, n_cam, pcost, out);
}
void launch_ba_prior_gram_add(int64_t n_c, const double* pdiag, const double* a, const double* b, double* out3, hipStream_t s) {
    hipLaunchKernelGGL(k_ba_prior_gram_add, dim3(1), dim3(256), 0, s, n_c, pdiag, a, b, out3);
}
void launch_ba_prior_export(const double* camq, const BaPriorView& pv, double* pose_out, double* intr_out, hipStream_t s) {
    const int n = pv.n_pose + pv.n_intr;
    if (n > 0) hipLaunchKernelGGL(k_ba_prior_export, dim3(grid_of(n, 64)), dim3(64), 0, s, camq, pv, pose_out, intr_out);
}

}  // namespace apex
