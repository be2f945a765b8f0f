// cov_kernels.hip -- marginal landmark covariances from the selected inverse of S.
//
// With V_l^-1 the (damped, gated, scaled) 3 x 3 inverse the Schur complement used, W_i = Jc_i^T Jl_i the camera-landmark
// block of observation i, and Z = S^-1 on the tile pattern of the factor (SelectedInverse::blocks / ensure, tile_sinv.h), the
// landmark block of the inverse of the factorised matrix is
//     Sigma_ll = D_l^-1 (Hinv_l + sum_{i,j in obs(l)} U_i^T Z_{c(i) c(j)} U_j) D_l^-1,     U_i = D_c W_i Hinv_l
// where Hinv_l = D_l V_l^-1 D_l is the landmark record (ba_kernels.h) and D the Jacobi scaling (identity when off).  This is the
// adjoint of the Schur pair kernel: it reads camera-pair blocks and writes one 3 x 3 per landmark.  Z_{c(i) c(j)} is the
// stored block when c(j) <= c(i) in the internal camera order; otherwise the pair is taken as (j, i), whose term is the
// transpose -- the sum is formed as X + X^T with X = sum_{i<j} P_ij + 1/2 sum_i P_ii, so the orientation of a term does not
// matter and the result is symmetric bit for bit.
//
// A group of G lanes handles one landmark: the lanes linearise the landmark's observations at the factorised point (the
// cameras of the parameter set the factor was linearised at, the point of the landmark record) and park U_i in LDS, then
// deal the observation pairs out round-robin (lane t: pairs t, t + G, ...) and reduce over the group with a fixed butterfly.
// No atomics, a fixed summation order: two calls give the same bits.  Small landmarks (k <= kLcSmallK observations) take
// 8-lane groups, one chunk; larger ones a whole 64-lane workgroup each, in chunks of kLcChunk observations (chunk pairs
// a <= b, two LDS slots), so a landmark seen by hundreds of cameras is spread over a wave instead of a lane.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "ba_device.hpp"
#include "ba_dispatch.h"
#include "ba_kernels.h"

namespace apex {

namespace {

// Hll^-1 (row-major, expanded from the six stored entries) and the point of a landmark record
__device__ __forceinline__ void load_hinv_point(const double* __restrict__ rec, int64_t l, double H[9], double pw[3]) {
    const double2* q = reinterpret_cast<const double2*>(rec + kLmStride * l);
    const double2 a0 = q[0], a1 = q[1], a2 = q[2], a3 = q[3], a4 = q[4];
    H[0] = a0.x; H[1] = a0.y; H[2] = a1.x;
    H[3] = a0.y; H[4] = a1.y; H[5] = a2.x;
    H[6] = a1.x; H[7] = a2.x; H[8] = a2.y;
    pw[0] = a3.x; pw[1] = a3.y; pw[2] = a4.x;
}

// U = D_c (Jc^T Jl) Hinv of observation i (DC x 3, row-major) and its camera
template <int DC, class LOSS>
__device__ __forceinline__ uint32_t obs_u(const BAView& v, LOSS loss, int64_t i, const double H[9], const double pw[3], double* __restrict__ U) {
    const uint32_t c = v.o_cam[i];
    Cam cam;
    load_cam_q(v.camq + kCamQStride * (size_t)c, v.mask_code, cam);
    const double2 uv = v.o_uv[i];
    double r[2], Jc[2][DC], Jl[2][3];
    linearize_obs<DC>(cam, pw, uv.x, uv.y, loss, r, Jc, Jl);
#pragma unroll
    for (int a = 0; a < DC; ++a) {
        const double s = v.cam_scale ? v.cam_scale[(size_t)c * DC + a] : 1.0;
        double w[3];
#pragma unroll
        for (int q = 0; q < 3; ++q) w[q] = s * (Jc[0][a] * Jl[0][q] + Jc[1][a] * Jl[1][q]);
#pragma unroll
        for (int q = 0; q < 3; ++q) U[a * 3 + q] = w[0] * H[q] + w[1] * H[3 + q] + w[2] * H[6 + q];
    }
    return c;
}

// X += wgt * Ui^T Z(ci, cj) Uj for ci >= cj (a block of Z's lower tile pattern)
template <int DC>
__device__ __forceinline__ void pair_term(const TileMap& z, const double* Ui, uint32_t ci, const double* Uj, uint32_t cj, double wgt,
                                          double X[9], int* __restrict__ err) {
    constexpr int CPT = kNB / DC;
    const int slot = z.slot[(size_t)(ci / CPT) * z.nt + cj / CPT];
    if (slot < 0) { *err = 1; return; }   // (cannot happen: a covisible pair is a block of S; refuse rather than read off the map)
    const double* B = z.tiles + (size_t)slot * (kNB * kNB) + (size_t)((ci % CPT) * DC) * kNB + (cj % CPT) * DC;
    double T[3][3] = {{0, 0, 0}, {0, 0, 0}, {0, 0, 0}};   // T = Ui^T B (3 x DC) folded with Uj row by row
#pragma unroll
    for (int a = 0; a < DC; ++a) {
        double y[3] = {0.0, 0.0, 0.0};   // row a of B Uj
#pragma unroll
        for (int b = 0; b < DC; ++b) {
            const double zab = B[(size_t)a * kNB + b];
#pragma unroll
            for (int q = 0; q < 3; ++q) y[q] += zab * Uj[b * 3 + q];
        }
#pragma unroll
        for (int p = 0; p < 3; ++p)
#pragma unroll
            for (int q = 0; q < 3; ++q) T[p][q] += Ui[a * 3 + p] * y[q];
    }
#pragma unroll
    for (int p = 0; p < 3; ++p)
#pragma unroll
        for (int q = 0; q < 3; ++q) X[3 * p + q] += wgt * T[p][q];
}

// G lanes per landmark, NT threads per workgroup; chunks of CH observations.  G == NT when CH chunks may repeat (k > CH): the
// chunk loop then runs uniformly over the workgroup and may synchronise.
// LOSS: empty (v.huber_delta) or PgLoss, a kernel argument of its own, as in ba_kernels.hip (ba_device.hpp, loss_arg)
template <int DC, int G, int NT, int CH, class... LOSS>
__global__ __launch_bounds__(NT) void k_landmark_cov(BAView v, LOSS... loss, const double* __restrict__ hinv, TileMap z, const int* __restrict__ list,
                                                     int n_list, double* __restrict__ out, int* __restrict__ err) {
    static_assert(NT % G == 0 && G <= 64, "groups inside a wave");
    constexpr int NGRP = NT / G, US = 3 * DC;
    constexpr bool MULTI = (G == NT);   // several chunks per landmark: two LDS slots
    constexpr int SLOTS = MULTI ? 2 : 1;
    __shared__ double sU[NGRP][SLOTS][CH * US];
    __shared__ uint32_t sC[NGRP][SLOTS][CH];
    const int grp = threadIdx.x / G, t = threadIdx.x % G;
    const int64_t li = (int64_t)blockIdx.x * NGRP + grp;
    const bool active = li < n_list;
    const int64_t l = active ? list[li] : 0;
    double H[9], pw[3];
    load_hinv_point(hinv, l, H, pw);
    const int b = v.pt_ptr[l], k = active ? v.pt_ptr[l + 1] - b : 0;
    const int nch = MULTI ? (k + CH - 1) / CH : 1;   // (!MULTI: the host puts only landmarks with k <= CH here)
    double X[9];
#pragma unroll
    for (int q = 0; q < 9; ++q) X[q] = 0.0;
    for (int ca = 0; ca < nch; ++ca) {
        for (int cb = ca; cb < nch; ++cb) {
            const int two = (MULTI && cb != ca) ? 2 : 1;
            if (MULTI) __syncthreads();   // (the previous chunk pair's reads are done)
            for (int q = t; q < two * CH; q += G) {
                const int s = q / CH, o = q - s * CH, idx = (s == 0 ? ca : cb) * CH + o;
                if (idx < k) sC[grp][s][o] = obs_u<DC>(v, loss_arg(v, loss...), b + idx, H, pw, &sU[grp][s][o * US]);
            }
            __syncthreads();
            const int na = min(CH, k - ca * CH), nb = min(CH, k - cb * CH);
            const int npairs = (two == 1) ? na * (na + 1) / 2 : na * nb;
            const int sb = two - 1;
            for (int p = t; p < npairs; p += G) {
                int i, j;
                if (two == 1) {   // p = j (j + 1) / 2 + i, i <= j
                    j = (int)((sqrt(8.0 * p + 1.0) - 1.0) * 0.5);
                    while (j * (j + 1) / 2 > p) --j;
                    while ((j + 1) * (j + 2) / 2 <= p) ++j;
                    i = p - j * (j + 1) / 2;
                } else {
                    i = p / nb; j = p - i * nb;
                }
                const double* Ui = &sU[grp][0][i * US];
                const double* Uj = &sU[grp][sb][j * US];
                const uint32_t ci = sC[grp][0][i], cj = sC[grp][sb][j];
                const double wgt = (two == 1 && i == j) ? 0.5 : 1.0;
                if (ci >= cj) pair_term<DC>(z, Ui, ci, Uj, cj, wgt, X, err);
                else pair_term<DC>(z, Uj, cj, Ui, ci, wgt, X, err);
            }
        }
    }
#pragma unroll
    for (int m = 1; m < G; m <<= 1)
#pragma unroll
        for (int q = 0; q < 9; ++q) X[q] += __shfl_xor(X[q], m, G);
    if (active && t == 0) {
        double d[3] = {1.0, 1.0, 1.0};
        if (v.pt_scale) { d[0] = v.pt_scale[3 * l]; d[1] = v.pt_scale[3 * l + 1]; d[2] = v.pt_scale[3 * l + 2]; }
        double* o = out + 9 * l;
#pragma unroll
        for (int p = 0; p < 3; ++p)
#pragma unroll
            for (int q = p; q < 3; ++q) {
                const double s = (H[3 * p + q] + (X[3 * p + q] + X[3 * q + p])) / (d[p] * d[q]);
                o[3 * p + q] = s;
                o[3 * q + p] = s;
            }
    }
}

}  // namespace

void launch_landmark_cov(int dc, const BAView& v, const double* hinv, const TileMap& z, const int* small_list, int n_small,
                         const int* large_list, int n_large, double* out, int* err, hipStream_t s, const PgLoss* loss) {
    constexpr int NT = 128, G = 8;
    static_assert(kLcSmallK <= G, "a small landmark is one chunk of its group");
    with_dc(dc, [&](auto DC) {
        with_ba_loss(loss, [&](auto... l) {
            if (n_large > 0)   // first: the long ones start early and the short ones fill in behind them
                hipLaunchKernelGGL((k_landmark_cov<DC(), 64, 64, kLcChunk, decltype(l)...>), dim3(n_large), dim3(64), 0, s, v, l..., hinv, z, large_list, n_large, out, err);
            if (n_small > 0)
                hipLaunchKernelGGL((k_landmark_cov<DC(), G, NT, kLcSmallK, decltype(l)...>), dim3((n_small + NT / G - 1) / (NT / G)), dim3(NT), 0, s, v, l..., hinv, z,
                                   small_list, n_small, out, err);
        });
    });
}

}  // namespace apex
