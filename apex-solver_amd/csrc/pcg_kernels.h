// pcg_kernels.h -- the device scalars and the launchers of the two Jacobi-PCG loops (pcg_kernels.hip): the explicit one on a
// plan's unfactored tiles (TilePcg, tile_pcg.h) and the one over an abstract operator (SchurJacobiPcg, schur_jacobi_pcg.h).
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>

#include "tile_tasks.h"

namespace apex {

// The scalars of an iteration as the kernels index them: eight doubles on the device, copied to a pinned slot (PcgReadback,
// pcg_readback.h) that the host reads through the same struct.
struct ExplicitPcgScalars { double rz_old, p_ap, rr, rz, frozen, pad[3]; };        // k_pcg_step1 / step2 / close_iteration
struct ImplicitPcgScalars { double rr, rz, p_ap, pad0, rz_old, frozen, beta, pad1; };   // k_pcg_implicit_* / update_*_sc
// ... and what the matrix-free loop's first dot2 leaves in sc[0..1] until the first iteration's dot2: k_pcg_implicit_begin reads rz
struct ImplicitPcgStart { double rz, rr; };
static_assert(sizeof(ExplicitPcgScalars) == 64 && offsetof(ExplicitPcgScalars, p_ap) == 8 && offsetof(ExplicitPcgScalars, rr) == 16 &&
              offsetof(ExplicitPcgScalars, rz) == 24 && offsetof(ExplicitPcgScalars, frozen) == 32, "the kernels index scal[0..4]");
static_assert(sizeof(ImplicitPcgScalars) == 64 && offsetof(ImplicitPcgScalars, rz) == 8 && offsetof(ImplicitPcgScalars, p_ap) == 16 &&
              offsetof(ImplicitPcgScalars, rz_old) == 32 && offsetof(ImplicitPcgScalars, frozen) == 40 && offsetof(ImplicitPcgScalars, beta) == 48,
              "the kernels index sc[0..6]");

void launch_sym_tile_products(const SymTile* list, int n, const double* tiles, const double* x, double* part, hipStream_t s);
void launch_sym_tile_gather(int nt, const int* row_ptr, const SymEntry* entries, const double* part, const double* p,
                            double* y, double* row_dot, hipStream_t s);
void launch_pcg_step1(int n, int nt, const double* scal, const double* row_dot, const double* p, const double* ap,
                      const double* pre, double* x, double* r, double* blk_part, double* out_pap, hipStream_t s);
void launch_pcg_step2(int n, double* scal, const double* blk_part, const double* pre, const double* r, double* p,
                      double* out2, double abs_tol, hipStream_t s);
void launch_pcg_init(int n, const double* diag, const double* b, double* pre, double* x, double* r, double* z, double* p,
                     hipStream_t s);
void launch_dot(int n, const double* a, const double* b, double* out, hipStream_t s);
// the matrix-free PCG's scalars stay on the device (sc: ImplicitPcgScalars): see k_pcg_implicit_close
void launch_pcg_implicit_begin(double* sc, hipStream_t s);
void launch_pcg_update_xr_sc(int n, const double* sc, const double* p, const double* ap, double* x, double* r, hipStream_t s);
void launch_pcg_implicit_close(double* sc, double abs_tol, hipStream_t s);
void launch_pcg_update_p_sc(int n, const double* sc, const double* z, double* p, hipStream_t s);

}  // namespace apex
