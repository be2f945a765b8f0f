// schur_jacobi_pcg.h -- block-Jacobi-preconditioned CG over an ABSTRACT operator (solve_pcg_block, implicit_schur.rs:577-679; the
// kernels: pcg_kernels.hip and the per-block launchers of the camera kernels; the host loop: pcg_loop.h).  Every scalar of an iteration
// stays on the device and the host reads them one iteration behind.  SchurJacobiPcg owns everything that is PCG -- the diagonal
// blocks and their inverses, the work vectors r, z, p, Ap, the eight device scalars and their read-back -- and borrows the
// reduction scratch of its owner.  It knows nothing of what the operator is: solve() takes y = A p as a callable, and whoever
// assembles the operator fills diag_blocks() with its diagonal (the matrix-free Schur complement: Solver, solver.hip).
#pragma once
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include <string>

#include "device_buffer.h"
#include "lm_loop.h"
#include "pcg_kernels.h"
#include "pcg_loop.h"
#include "pcg_readback.h"

namespace apex {

class SchurJacobiPcg {
   public:
    // Once per structure: n_blocks diagonal blocks of dc x dc over n = n_blocks * dc unknowns in vectors of n_pad; `partial`
    // (n_partial blocks' worth, two sums each) is the owner's reduction scratch, used between this class's own launches only.
    // Everything is allocated and cleared on the NULL stream; a second setup() replaces the first, the destructor frees.
    hipError_t setup(int64_t n_blocks, int dc, int64_t n, int64_t n_pad, hipStream_t stream, double* partial, int n_partial);
    double* diag_blocks() { return diag_; }   // [n_blocks][dc][dc]: the operator's diagonal, summed over the ranks by its assembler
    // diag_blocks() is complete: D A D's blocks in place when a scaling is given (n entries, else NULL), then their inverses
    void build_preconditioner(const double* scale_or_null);
    // x = A^-1 rhs from x = 0.  matvec(p, ap) -> status enqueues ap = A p on the stream; a status other than kOk ends the loop
    // and is returned as it is (its text is the callable's business).  A HIP failure of the loop itself: kDeviceError, the text
    // in *err.  *iters as the reference counts them; x is final on return (the stream has drained).
    template <typename Matvec>
    int solve(const double* rhs, double* x, int max_iter, double tol, Matvec&& matvec, int* iters, std::string* err) {
        double abs_tol = 0.0;
        int rc = check(begin(rhs, x, tol, &abs_tol), "the PCG's first sums", err);
        if (rc != kOk) return rc;
        const PcgLoopResult res = pcg_loop_one_behind(
            max_iter,
            [&](int slot) -> int {
                const int mrc = matvec(static_cast<const double*>(p_), ap_.get());
                return mrc != kOk ? mrc : check(close_iteration(slot, x, abs_tol), "a PCG iteration", err);
            },
            [&](int slot) -> int { return check(readback_.wait(slot), "the PCG read-back's wait", err); },
            [&](int slot) {
                const ImplicitPcgScalars& h = readback_.host(slot);
                if (fabs(h.p_ap) < 1e-20) return PcgVerdict::kStopUncounted;               // :610-613 (x, r untouched)
                return h.frozen != 0.0 ? PcgVerdict::kStopCounted : PcgVerdict::kGoOn;   // the device's verdict: |r| < tol (:634-641) or rz_old ~ 0 (:652-654)
            });
        if (res.status != kOk) return res.status;
        rc = check(hipStreamSynchronize(stream_), "the PCG's last wait", err);   // (the speculative iteration, if any, has drained)
        if (rc == kOk) *iters = res.iterations;
        return rc;
    }

   private:
    // x = 0, r = rhs, z = M^-1 r, p = z, the first sums; waits once for |rhs|: *abs_tol = tol * max(|rhs|, 1)
    hipError_t begin(const double* rhs, double* x, double tol, double* abs_tol);
    // behind ap_ = A p_: alpha, x, r, z, the three termination tests, beta, p -- and the scalars posted to `slot`
    hipError_t close_iteration(int slot, double* x, double abs_tol);
    static int check(hipError_t e, const char* what, std::string* err) {
        if (e != hipSuccess) *err = std::string("HIP error in ") + what + ": " + hipGetErrorString(e);
        return e == hipSuccess ? kOk : kDeviceError;
    }

    int64_t n_blocks_ = 0, n_ = 0, n_pad_ = 0;
    int dc_ = 0, n_partial_ = 0;
    hipStream_t stream_ = nullptr;
    double* partial_ = nullptr;   // borrowed
    DeviceBuffer<double> diag_, minv_;
    DeviceBuffer<double> r_, z_, p_, ap_;
    DeviceBuffer<double> scal_;   // ImplicitPcgScalars
    PcgReadback<ImplicitPcgScalars> readback_;
};

}  // namespace apex
