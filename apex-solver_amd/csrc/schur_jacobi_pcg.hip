// schur_jacobi_pcg.hip -- see schur_jacobi_pcg.h
#include "schur_jacobi_pcg.h"

#include <string.h>

#include <algorithm>

#include "ba_kernels.h"

namespace apex {

hipError_t SchurJacobiPcg::setup(int64_t n_blocks, int dc, int64_t n, int64_t n_pad, hipStream_t stream, double* partial, int n_partial) {
    n_blocks_ = n_blocks; dc_ = dc; n_ = n; n_pad_ = n_pad;
    stream_ = stream; partial_ = partial; n_partial_ = n_partial;
    hipError_t e = diag_.alloc_zero((size_t)n_blocks * dc * dc);
    if (e == hipSuccess) e = minv_.alloc_zero((size_t)n_blocks * dc * dc);
    for (DeviceBuffer<double>* v : {&r_, &z_, &p_, &ap_})
        if (e == hipSuccess) e = v->alloc_zero((size_t)n_pad);
    if (e == hipSuccess) e = scal_.alloc_zero(sizeof(ImplicitPcgScalars) / sizeof(double));
    return e;
}

void SchurJacobiPcg::build_preconditioner(const double* scale_or_null) {
    if (scale_or_null) launch_scale_diag_blocks(dc_, n_blocks_, scale_or_null, diag_, stream_);
    launch_precond_blocks(dc_, n_blocks_, diag_, minv_, stream_);
}

hipError_t SchurJacobiPcg::begin(const double* rhs, double* x, double tol, double* abs_tol) {
    double* sc = scal_;
    hipError_t e;
    if ((e = readback_.ensure()) != hipSuccess) return e;
    if ((e = hipMemsetAsync(x, 0, n_pad_ * sizeof(double), stream_)) != hipSuccess) return e;
    if ((e = hipMemcpyAsync(r_, rhs, n_pad_ * sizeof(double), hipMemcpyDeviceToDevice, stream_)) != hipSuccess) return e;
    launch_precond_apply(dc_, n_blocks_, minv_, r_, z_, stream_);
    if ((e = hipMemcpyAsync(p_, z_, n_pad_ * sizeof(double), hipMemcpyDeviceToDevice, stream_)) != hipSuccess) return e;
    launch_dot2((int)n_, r_, z_, r_, r_, partial_, n_partial_, sc, stream_);
    launch_pcg_implicit_begin(sc, stream_);   // rz_old := r.z, not frozen
    if ((e = hipMemcpyAsync(&readback_.host(0), sc, sizeof(ImplicitPcgStart), hipMemcpyDeviceToHost, stream_)) != hipSuccess) return e;
    if ((e = hipStreamSynchronize(stream_)) != hipSuccess) return e;
    ImplicitPcgStart start;
    memcpy(&start, &readback_.host(0), sizeof start);
    *abs_tol = tol * std::max(sqrt(start.rr), 1.0);
    return hipSuccess;
}

// Every scalar of the iteration stays on the device (alpha, beta, the reference's three termination tests:
// k_pcg_implicit_close), and the host reads {r.r, r.z, p.Ap, frozen} one iteration behind (pcg_loop.h).  (Sharded: every rank
// reads the same scalars and enqueues the same iterations.)
hipError_t SchurJacobiPcg::close_iteration(int slot, double* x, double abs_tol) {
    const int n = (int)n_;
    double* sc = scal_;
    launch_dot2(n, p_, ap_, p_, ap_, partial_, n_partial_, sc + offsetof(ImplicitPcgScalars, p_ap) / sizeof(double), stream_);
    launch_pcg_update_xr_sc(n, sc, p_, ap_, x, r_, stream_);      // alpha = rz_old / p.Ap; nothing when |p.Ap| < 1e-20 (:610-613)
    launch_precond_apply(dc_, n_blocks_, minv_, r_, z_, stream_);
    launch_dot2(n, r_, r_, r_, z_, partial_, n_partial_, sc, stream_);
    launch_pcg_implicit_close(sc, abs_tol, stream_);               // :634-641, :652-654, else beta and rz_old
    launch_pcg_update_p_sc(n, sc, z_, p_, stream_);
    return readback_.post(slot, sc, 6, stream_);
}

}  // namespace apex
