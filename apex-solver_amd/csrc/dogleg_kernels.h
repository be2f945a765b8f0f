// dogleg_kernels.h -- launchers of the Dog-Leg vector kernels (dogleg_kernels.hip): what a Dog-Leg step is beside the solve and
// the Gram pass, on plain vectors -- nothing here knows a pose, a camera or a manifold (dog_leg.rs:776-803, 818-902, 948-960;
// dogleg_combine.hpp).  The products with H = J^T J stay with the problem's own kernels (launch_pg_jv_gram, launch_ba_jv_gram).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace apex {

struct ColumnMap;

// One contiguous piece of the Dog-Leg vectors: the pose graph has one (all of g_ / d_), bundle adjustment two (the camera and the
// landmark half).  What the kernels read: n, g the gradient, d the step (read by the dots, written by the blend), scale (may be
// NULL: 1), a = scale^2 g (written by the dots; may be NULL), h the cached Gauss-Newton step (written by the dots, read by the
// blend).  What TileBackend reads (tile_backend.h): n_alloc, the length a and h are allocated with, and map, the caller's columns
// of the piece.  A solver fills everything but a and h, which are TileBackend's.
struct DlSegment {
    int64_t n; const double* g; double* d; const double* scale; double* a; double* h;
    int64_t n_alloc; const ColumnMap* map;
};

// All reductions: no atomics, a fixed order.  Segment k of n_seg (1 | 2) takes per = n_partial / n_seg blocks and writes its
// partials from partial + stride * k * per (n_partial >= n_seg; partial holds 3 n_partial doubles for the dots, n_partial for the
// blend; an odd n_partial leaves its last slot unused with two segments); then ONE sum of the n_seg * per entries in index order
// -- first segment first.
// out3 = {g_s.g_s, y.y, g_s.y} for g_s = scale g, y = d / scale; a = scale^2 g, h = d on the way
void launch_dl_dots(const DlSegment* segs, int n_seg, double* partial, int n_partial, double* out3, hipStream_t s);
// out7 = {alpha, beta, c_g, c_h, |step_s|, predicted reduction, type} from sums6 = {g.g, h.h, g.h, g.Hg, g.Hh, h.Hh} (device) and the radius
void launch_dl_combine(const double* sums6, double delta, double* out7, hipStream_t s);
// d = coef[1] h - coef[0] scale^2 g (coef on the device), out_sumsq = |d|^2
void launch_dl_blend(const DlSegment* segs, int n_seg, const double* coef, double* partial, int n_partial, double* out_sumsq,
                     hipStream_t s);

}  // namespace apex
