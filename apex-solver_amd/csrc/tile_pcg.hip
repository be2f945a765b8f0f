// tile_pcg.hip -- see tile_pcg.h
#include "tile_pcg.h"

#include <math.h>

#include <algorithm>

#include "chol_kernels.h"
#include "pcg_loop.h"

namespace apex {

hipError_t TilePcg::setup(const PcgPlanView& v, const PlanLists& lists, int64_t n_slots) {
    v_ = v;
    hipError_t e = sym_part_.alloc_zero((size_t)n_slots * 2 * kNB);
    if (e == hipSuccess) e = row_dot_.alloc_zero((size_t)v.nt);
    if (e == hipSuccess) e = blk_part_.alloc_zero(2 * (size_t)((v.n_pad + 255) / 256));
    if (e == hipSuccess) e = scal_.alloc_zero(8);
    if (e == hipSuccess) e = sym_row_ptr_.upload(lists.sym_row_ptr);
    if (e == hipSuccess) e = sym_entries_.upload(lists.sym_entries);
    return e;
}

void TilePcg::release() {
    sym_row_ptr_.reset(); sym_entries_.reset();
    sym_part_.reset(); row_dot_.reset(); blk_part_.reset(); scal_.reset();
    readback_.release();
}

void TilePcg::matvec(const double* x, double* y) {
    launch_sym_tile_products(v_.sym_tiles, v_.n_sym_tiles, v_.tiles, x, sym_part_, v_.stream);
    launch_sym_tile_gather(v_.nt, sym_row_ptr_, sym_entries_, sym_part_, x, y, row_dot_, v_.stream);
}

// Per iteration: one pass over the non-zero tiles (k_sym_tile_products + k_sym_tile_gather, which also yields p.Ap), two fused
// vector kernels that keep alpha/beta on the device, and ONE host read-back of {p.Ap, r.r, r.z, frozen} for the reference's three
// termination tests, one iteration behind (pcg_loop.h); k_pcg_close_iteration makes the same tests on the device.
hipError_t TilePcg::solve(const double* rhs, double* x, double* work, int max_iter, double tol, int* iters) {
    const hipStream_t stream = v_.stream;
    const int n = (int)v_.n_pad;
    double *dg = work, *pre = work + n, *r = work + 2 * (size_t)n, *z = work + 3 * (size_t)n, *p = work + 4 * (size_t)n,
           *ap = work + 5 * (size_t)n;
    double* sc = scal_;  // ExplicitPcgScalars
    hipError_t e;
    if ((e = readback_.ensure()) != hipSuccess) return e;
    launch_tile_diag(v_.tiles, v_.diag_slot, v_.nt, dg, stream);
    launch_pcg_init(n, dg, rhs, pre, x, r, z, p, stream);
    if ((e = hipMemsetAsync(sc, 0, 8 * sizeof(double), stream)) != hipSuccess) return e;
    launch_dot(n, r, z, sc, stream);
    launch_dot(n, r, r, sc + 2, stream);
    if ((e = hipMemcpyAsync(&readback_.host(0), sc, 4 * sizeof(double), hipMemcpyDeviceToHost, stream)) != hipSuccess) return e;
    if ((e = hipStreamSynchronize(stream)) != hipSuccess) return e;
    const double abs_tol = tol * std::max(sqrt(readback_.host(0).rr), 1.0);
    const PcgLoopResult res = pcg_loop_one_behind(
        max_iter,
        [&](int slot) -> int {
            matvec(p, ap);
            launch_pcg_step1(n, v_.nt, sc, row_dot_, p, ap, pre, x, r, blk_part_, sc + 1, stream);
            launch_pcg_step2(n, sc, blk_part_, pre, r, p, sc + 2, abs_tol, stream);
            return readback_.post(slot, sc, 5, stream);
        },
        [&](int slot) -> int { return readback_.wait(slot); },
        [&](int slot) {   // the device's verdict (frozen, k_pcg_close_iteration) decides -- the speculative iteration obeys the same word
            const ExplicitPcgScalars& h = readback_.host(slot);
            if (fabs(h.p_ap) < 1e-30) return PcgVerdict::kStopUncounted;               // p.Ap (:703-705); x was left untouched
            return h.frozen != 0.0 ? PcgVerdict::kStopCounted : PcgVerdict::kGoOn;   // |r| < tol (:726-728) or rz_old ~ 0 (:741-743)
        });
    if (res.status != 0) return (hipError_t)res.status;
    *iters = res.iterations;
    return hipStreamSynchronize(stream);   // (the speculative iteration, if any, has drained: x is final)
}

}  // namespace apex
