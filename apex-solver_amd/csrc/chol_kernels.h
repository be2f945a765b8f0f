// chol_kernels.h -- launchers of the tile Cholesky / triangular-solve kernels and of the small operations on a plan's tiles.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "ba_kernels.h"
#include "tile_tasks.h"

namespace apex {

void launch_potrf_inv(const PotrfTask* tasks, int n, int* fail, hipStream_t s, int* arrived = nullptr);
void launch_gate(const int* arrived, int expected, int max_micros, hipStream_t s);
// the dataflow factorisation: one workgroup per unit, dispatched in list order; ver[] must be zero; err: error word (time-out)
void launch_factor_flow(const FactorUnit* units, int n_units, int* ver, int* fail, int* err, hipStream_t s,
                        unsigned long long* trace = nullptr, bool diag_lower = false);
// batches of <= 56 tasks use the latency kernels, larger ones the four-wave strip kernel (three workgroups per tile)
// tri_b: every B is a lower-triangular inverse written by launch_potrf_inv (zero 16 x 16 blocks right of the diagonal): the
// large-batch kernel then skips the 36 of 81 block products that multiply by them.
// diag_lower (the updates, beta != 0): a task with A == B targets a diagonal tile, of which only the lower triangle is read again;
// its three 48 x 48 blocks right of the diagonal ones are not computed (in k_factor_flow likewise)
void launch_tile_gemm_nt(const GemmTask* tasks, int n, double alpha, double beta, hipStream_t s, bool tri_b = false, bool diag_lower = false);
void launch_clear_i32(int* p, int64_t n, hipStream_t s);                   // a small clear as ONE kernel (chol_kernels.hip)
void launch_post_word(int* word, int* host_word_dev, hipStream_t s);       // *host = *word, *word = 0 when *word != 0
// poison_block >= 0 (tests only): that block's counter is made unreachable after the flags are cleared, so the task that
// waits for it runs into the spin limit -- the time-out path (error word raised, wrong result) on demand
void launch_tri_flow(bool backward, const FlowTask* tasks, int n_tasks, const double* in, double* out, double* part, int* flags,
                     int nt, hipStream_t s, const double* fold_b, double* fold_out, int poison_block = -1, bool keep_flags = false);   // keep_flags: the second part of a sweep launched in two (the counters of the first part stand)
// tests only: n workgroups that each take a whole CU's LDS (nothing else that needs LDS fits beside them) and spin for
// `micros`; *started (host-visible) counts the workgroups that are resident
void launch_occupy_cus(int n, int micros, int* started, hipStream_t s);
void launch_tri_step(bool trans, const TriTask* tasks, int n, double* vwork, double* vout, hipStream_t s);
void launch_tile_diag(const double* tiles, const int* diag_slot, int nt, double* diag, hipStream_t s);
void launch_tile_add_diag(double* tiles, const int* diag_slot, int n_valid, int n_total, double add_valid,
                          double set_pad, hipStream_t s);
// distributed triangular solves: per-tile class masks (bit 1 << cls[tile]); in must not alias out for select
void launch_vec_select(int n, const double* in, const int* cls, int mask, double* out, hipStream_t s);
void launch_vec_merge(int n, const double* src, const int* cls, int mask, double* dst, hipStream_t s);
void launch_tile_scale_sym(const SymTile* list, int n, double* tiles, const double* scale /* n_pad */, hipStream_t s);

}  // namespace apex
