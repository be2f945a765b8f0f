// hessian_csc.h -- the host assembly behind Solver::get_hessian_csc (explicit_schur.rs:1236-1238): H = J^T J of a bundle
// adjustment problem, undamped, full symmetric, CSC in the caller's global column order, from the per-factor Jacobian blocks the
// device linearises.  An observer / Dog-Leg export, not the hot path.  Plain host C++: tests/host_harness_hessian_csc.cpp.
#pragma once
#include <stdint.h>

#include <vector>

#include "column_map.h"

namespace apex {

struct HessianCscInput {
    int64_t n_cam = 0, n_pt = 0, n_obs = 0;
    int dc = 9;                            // columns per camera: 9 | 6
    const uint32_t* cam_idx = nullptr;     // [n_obs] the caller's factor list: camera and
    const uint32_t* pt_idx = nullptr;      // [n_obs] landmark of factor i, the caller's numbering
    const double* jc = nullptr;            // [n_obs][2][dc] camera blocks, [n_obs][2][3] landmark blocks (get_jacobian_blocks);
    const double* jl = nullptr;            //   both NULL: the count alone
    const std::vector<double>* prior_diag = nullptr;   // diag(P) of the camera priors [n_cam * dc], INTERNAL order; NULL or empty: none
    const std::vector<int>* cmap = nullptr;            // the caller's camera -> internal camera (read with prior_diag only)
    const ColumnMap* cam_map = nullptr;    // the caller's columns of the camera side and
    const ColumnMap* pt_map = nullptr;     //   of the landmarks
};

// Returns nnz: 2 * dc * 3 per distinct (camera, landmark) coupling, dc * dc per camera that a factor or a non-zero prior
// diagonal touches, 9 per observed landmark.  Structural entries of every factor are kept even when a block is zero (a point
// behind its camera), as the reference's sparse product keeps them; duplicated (camera, landmark) factors are merged.  With jc
// and jl: colptr [total + 1], rowidx [nnz], values [nnz] are filled (total = 9 n_cam + 3 n_pt), row indices ascending inside a
// column; -1 if the entries written do not add up to nnz (never, for lists in range).
int64_t hessian_csc(const HessianCscInput& in, int64_t* colptr, int64_t* rowidx, double* values);

}  // namespace apex
