// ba_prior_kernels.h -- PriorFactor blocks on the cameras of a bundle-adjustment problem: the launchers of
// ba_prior_kernels.hip.  The priors are block-diagonal in H_cc, so they are small add-ons BEHIND the kernels of ba_kernels.hip,
// which never see them: one evaluation per linearisation leaves diag(P) = sum rho' w^2 per camera column, P's gradient and
// the cost per camera, and every consumer adds those vectors where its kernel left off.  No atomics anywhere: one lane owns one
// camera's run of blocks and sums it in list order.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "ba_kernels.h"
#include "prior_lists.h"   // kPosePriorStride, kIntrPriorStride: the block layouts, where the host packs them

namespace apex {

// Both sets as the device holds them: sorted by internal camera (stable), with a CSR over the cameras.  An empty set: n = 0.
struct BaPriorView {
    int n_pose = 0, n_intr = 0;
    const int* pose_ptr = nullptr;      // [n_cam + 1] run of camera c: [pose_ptr[c], pose_ptr[c + 1])
    const double* pose_data = nullptr;  // [n_pose][kPosePriorStride]
    const int* pose_slot = nullptr;     // [n_pose] the caller's index of the block (export order)
    const int* pose_cam = nullptr;      // [n_pose] the block's internal camera
    const int* intr_ptr = nullptr;
    const double* intr_data = nullptr;  // [n_intr][kIntrPriorStride]
    const int* intr_slot = nullptr;
    const int* intr_cam = nullptr;
};

// One lane per camera over camq (BAView::camq: the normalised pose and the intrinsics of one parameter set): pdiag / pg
// [n_cam][dc] (may both be NULL: the cost alone) := sum of (sqrt(rho') w)^2 on the block's columns | J~^T r~; pcost[n_cam] :=
// the camera's sum of squared corrected rows (all seven of a pose block).
void launch_ba_prior_eval(int dc, int64_t n_cam, const double* camq, const BaPriorView& pv, double* pdiag, double* pg, double* pcost, hipStream_t s);
// explicit S: the diagonal of the tiles += pdiag, g_c += pg, g_red -= pg (the right-hand side's sign) over the n_c camera columns
void launch_ba_prior_add_system(int64_t n_c, const double* pdiag, const double* pg, const TileMap& tm, double* g_c, double* g_red, hipStream_t s);
// matrix-free: the diagonal of the Schur-Jacobi blocks sd[n_cam][dc][dc] += pdiag, g_c += pg, g_red -= pg
void launch_ba_prior_add_blocks(int dc, int64_t n_cam, const double* pdiag, const double* pg, double* sd, double* g_c, double* g_red, hipStream_t s);
void launch_ba_prior_matvec(int64_t n_c, const double* pdiag, const double* x, double* y, hipStream_t s);   // y += P x
// out[0] += sum_c pcost[c]: one block, a fixed tree -- the priors' own partial slot behind launch_cost's sum
void launch_ba_prior_cost_add(int64_t n_cam, const double* pcost, double* out, hipStream_t s);
// out3 += { sum p a^2, sum p a b, sum p b^2 } over the n_c camera columns (a prior row has one entry): one block, a fixed tree
void launch_ba_prior_gram_add(int64_t n_c, const double* pdiag, const double* a, const double* b, double* out3, hipStream_t s);
// corrected residuals in the caller's order: pose_out [n_pose][7], intr_out [n_intr][3] (either may be NULL)
void launch_ba_prior_export(const double* camq, const BaPriorView& pv, double* pose_out, double* intr_out, hipStream_t s);

}  // namespace apex
