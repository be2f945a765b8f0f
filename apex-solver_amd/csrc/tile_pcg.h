// tile_pcg.h -- Jacobi-preconditioned CG on a TilePlan's UNFACTORED tiles (solve_with_pcg, explicit_schur.rs:639-756; the
// kernels: pcg_kernels.hip; the host loop: pcg_loop.h).  TilePcg owns everything that is PCG -- the gather lists and partials of
// the symmetric tile product, the reduction scratch, the device scalars and their read-back -- and reads the plan through a view
// the plan fills in.  It writes nothing of the plan.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "device_buffer.h"
#include "pcg_kernels.h"
#include "pcg_readback.h"
#include "plan_lists.h"

namespace apex {

// What the PCG reads of its plan.  TilePlan::upload() fills it in once: every field is written by build() alone and void after
// release(), which are also the two calls that run setup() and release() here.
struct PcgPlanView {
    const double* tiles = nullptr;       // device, by slot
    const int* diag_slot = nullptr;      // device
    const SymTile* sym_tiles = nullptr;  // device: the tiles non-zero before fill (the plan's: scale_sym reads them too)
    int n_sym_tiles = 0;
    int nt = 0;
    int64_t n_pad = 0;
    hipStream_t stream = nullptr;
};

class TilePcg {
   public:
    // the device step of the plan's build(): the gather lists uploaded, the work arrays allocated and cleared (NULL stream)
    hipError_t setup(const PcgPlanView& v, const PlanLists& lists, int64_t n_slots);
    void release();
    // y = A x (deterministic two-pass symmetric product), no sync
    void matvec(const double* x, double* y);
    // work: 6*n_pad doubles; syncs once per iteration
    hipError_t solve(const double* rhs, double* x, double* work, int max_iter, double tol, int* iters);
    const double* scalars() const { return scal_; }   // device: ExplicitPcgScalars as the last solve() left them (tests)

   private:
    PcgPlanView v_;
    DeviceBuffer<int> sym_row_ptr_;
    DeviceBuffer<SymEntry> sym_entries_;
    DeviceBuffer<double> sym_part_, row_dot_, blk_part_, scal_;
    PcgReadback<ExplicitPcgScalars> readback_;
};

}  // namespace apex
