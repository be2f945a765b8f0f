// pcg_kernels.hip -- the kernels of the two Jacobi-preconditioned conjugate-gradient loops (pcg_kernels.h): the symmetric tile
// product of the explicit loop (TilePcg, tile_pcg.h), its fused vector updates, and the vector updates of the matrix-free loop
// (SchurJacobiPcg, schur_jacobi_pcg.h).  Every scalar of an iteration stays on the device; the layouts are pcg_kernels.h's.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "pcg_kernels.h"
#include "device_reduce.hpp"
#include "tile_kernel_defs.h"

namespace apex {

// ------------------------------------------------------------------------------------------
// Symmetric tile matvec for the PCG variant, two deterministic passes (no atomics):
//   k_sym_tile_products: one workgroup per STRUCTURALLY NON-ZERO tile (I,J) of S reads the tile ONCE
//       (straight into registers, see below) and writes u = A x_J and, off the diagonal, v = A^T x_I
//       (diagonal tiles: u = sym(A) x_I from the lower triangle) to part[slot][0..143 | 144..287];
//   k_sym_tile_gather: one workgroup per block row adds its partials in list order and also emits
//       the block's share of p.Ap.
// ------------------------------------------------------------------------------------------
// (round 4: the tile no longer goes through LDS.  The first version staged two 72-row halves in 84 KB of LDS -- one workgroup
// per CU, 144 of its 256 threads doing 72-step dot products out of LDS between two barriers: 198 us for the 710 MB of
// final-13682's touched tiles, 3.6 TB/s.  Now a wave streams 36 rows straight into registers, a lane owning the column pair
// (2 l, 2 l + 1) and, lanes 0..7, (128 + 2 l, 129 + 2 l): v = A^T x_I accumulates in the lane, u = A x_J is one DPP wave
// reduction per row; 4.7 KB of LDS for the vectors and the four waves' column sums, eight workgroups per CU.)
template <int CTRL, int ROW_MASK>
__device__ __forceinline__ double sym_dpp_add(double x) {   // x + (x moved by CTRL); lanes outside the row mask, and lanes the move has nothing for, add 0
    const int lo = __builtin_amdgcn_update_dpp(0, __double2loint(x), CTRL, ROW_MASK, 0xF, true);
    const int hi = __builtin_amdgcn_update_dpp(0, __double2hiint(x), CTRL, ROW_MASK, 0xF, true);
    return x + __hiloint2double(hi, lo);
}
__device__ __forceinline__ double sym_wave_sum(double x) {   // the sum over the 64 lanes, valid in lane 63
    x = sym_dpp_add<0x118, 0xF>(x);   // row_shr:8
    x = sym_dpp_add<0x114, 0xF>(x);   // row_shr:4
    x = sym_dpp_add<0x112, 0xF>(x);   // row_shr:2
    x = sym_dpp_add<0x111, 0xF>(x);   // row_shr:1   -> lane 15 of every row of 16 holds the row's sum
    x = sym_dpp_add<0x142, 0xA>(x);   // row_bcast:15 into rows 1 and 3
    x = sym_dpp_add<0x143, 0xC>(x);   // row_bcast:31 into rows 2 and 3
    return x;
}
__global__ __launch_bounds__(256) void k_sym_tile_products(const SymTile* __restrict__ list,
                                                             const double* __restrict__ tiles,
                                                             const double* __restrict__ x, double* __restrict__ part) {
    constexpr int RW = NB / 4;   // 36 rows per wave
    constexpr int RB = 6;        // rows in flight per wave (12 loads of 16 bytes per lane)
    __shared__ double sxI[NB], su[NB], sv[4][NB];
    const SymTile st = list[blockIdx.x];
    const double* __restrict__ M = tiles + (size_t)st.slot * (NB * NB);
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    const bool diag = (st.I == st.J);
    if (tid < NB) sxI[tid] = x[(size_t)st.I * NB + tid];
    const bool ext = lane < 8;   // the lanes that also own columns 128 + 2 l, 129 + 2 l
    const int c0 = 2 * lane, c1 = 128 + 2 * lane;
    const double2 xj = *reinterpret_cast<const double2*>(x + (size_t)st.J * NB + c0);
    const double2 xje = ext ? *reinterpret_cast<const double2*>(x + (size_t)st.J * NB + c1) : make_double2(0.0, 0.0);
    double v0 = 0.0, v1 = 0.0, ve0 = 0.0, ve1 = 0.0;
    __syncthreads();
    for (int rb = 0; rb < RW; rb += RB) {
        double2 m[RB], me[RB];
#pragma unroll
        for (int k = 0; k < RB; ++k) {
            const double* row = M + (size_t)(RW * w + rb + k) * NB;
            m[k] = *reinterpret_cast<const double2*>(row + c0);
            me[k] = ext ? *reinterpret_cast<const double2*>(row + c1) : make_double2(0.0, 0.0);
        }
#pragma unroll
        for (int k = 0; k < RB; ++k) {
            const int r = RW * w + rb + k;
            double a0 = m[k].x, a1 = m[k].y, b0 = me[k].x, b1 = me[k].y;
            if (diag) {   // only the lower triangle of a diagonal tile is valid: u takes it with the diagonal ...
                if (c0 > r) a0 = 0.0;
                if (c0 + 1 > r) a1 = 0.0;
                if (c1 > r) b0 = 0.0;
                if (c1 + 1 > r) b1 = 0.0;
            }
            const double pr = fma(a0, xj.x, fma(a1, xj.y, fma(b0, xje.x, b1 * xje.y)));
            const double tot = sym_wave_sum(pr);
            if (lane == 63) su[r] = tot;
            if (diag) {   // ... and v = (strictly lower part)^T x_I completes sym(A) x
                if (c0 == r) a0 = 0.0;
                if (c0 + 1 == r) a1 = 0.0;
                if (c1 == r) b0 = 0.0;
                if (c1 + 1 == r) b1 = 0.0;
            }
            const double xi = sxI[r];
            v0 = fma(a0, xi, v0); v1 = fma(a1, xi, v1); ve0 = fma(b0, xi, ve0); ve1 = fma(b1, xi, ve1);
        }
    }
    sv[w][c0] = v0; sv[w][c0 + 1] = v1;
    if (ext) { sv[w][c1] = ve0; sv[w][c1 + 1] = ve1; }
    __syncthreads();
    double* pu = part + (size_t)st.slot * (2 * NB);
    if (tid < NB) {
        pu[tid] = su[tid];
        pu[NB + tid] = (sv[0][tid] + sv[1][tid]) + (sv[2][tid] + sv[3][tid]);
    }
}

__global__ __launch_bounds__(256) void k_sym_tile_gather(const int* __restrict__ row_ptr,
                                                           const SymEntry* __restrict__ entries,
                                                           const double* __restrict__ part,
                                                           const double* __restrict__ p, double* __restrict__ y,
                                                           double* __restrict__ row_dot) {
    __shared__ double sc[4];
    const int I = blockIdx.x, tid = threadIdx.x;
    double acc = 0.0;
    if (tid < NB) {
        for (int e = row_ptr[I]; e < row_ptr[I + 1]; ++e) {
            const SymEntry en = entries[e];
            const double* pu = part + (size_t)en.slot * (2 * NB);
            if (en.kind == 0) acc += pu[tid];                 // tile (I, other): u
            else if (en.kind == 1) acc += pu[NB + tid];       // tile (other, I): v
            else acc += pu[tid] + pu[NB + tid];               // diagonal: lower part + mirrored upper part
        }
        y[(size_t)I * NB + tid] = acc;
    }
    double d = (tid < NB) ? acc * p[(size_t)I * NB + tid] : 0.0;
    d = wave_sum(d);
    if ((tid & 63) == 0) sc[tid >> 6] = d;
    __syncthreads();
    if (tid == 0) row_dot[I] = (sc[0] + sc[1]) + (sc[2] + sc[3]);
}

// PCG state update, part 1:  alpha = rz_old / pAp ; x += alpha p ; r -= alpha Ap ; per-block
// partial sums of r.r and r.(pre r).   scal[0] = rz_old, row_dot[0..nt) = shares of p.Ap.
__global__ __launch_bounds__(256) void k_pcg_step1(int n, int nt, const double* __restrict__ scal,
                                                     const double* __restrict__ row_dot, const double* __restrict__ p,
                                                     const double* __restrict__ ap, const double* __restrict__ pre,
                                                     double* __restrict__ x, double* __restrict__ r,
                                                     double* __restrict__ blk_part, double* __restrict__ out_pap) {
    __shared__ double sc[4];
    __shared__ double s_alpha;
    const int tid = threadIdx.x;
    double pap = 0.0;
    for (int i = tid; i < nt; i += 256) pap += row_dot[i];
    pap = wave_sum(pap);
    if ((tid & 63) == 0) sc[tid >> 6] = pap;
    __syncthreads();
    if (tid == 0) {
        const double tot = (sc[0] + sc[1]) + (sc[2] + sc[3]);
        // scal[4] != 0: the iteration BEFORE this one met a termination test (k_pcg_close_iteration) -- the host, which reads the
        // scalars one iteration behind (TilePcg::solve), has enqueued this one on speculation: it changes nothing
        const bool frozen = scal[4] != 0.0;
        s_alpha = (frozen || fabs(tot) < 1e-30) ? 0.0 : scal[0] / tot;   // |pAp| < 1e-30: the host breaks (:703-705)
        if (blockIdx.x == 0 && !frozen) out_pap[0] = tot;
    }
    __syncthreads();
    const double alpha = s_alpha;
    const int i = blockIdx.x * 256 + tid;
    double rr = 0.0, rz = 0.0;
    if (i < n) {
        x[i] += alpha * p[i];
        const double ri = r[i] - alpha * ap[i];
        r[i] = ri;
        rr = ri * ri; rz = ri * (pre[i] * ri);
    }
    rr = wave_sum(rr); rz = wave_sum(rz);
    __syncthreads();
    if ((tid & 63) == 0) { sc[tid >> 6] = rr; }
    __syncthreads();
    const double rr_b = (sc[0] + sc[1]) + (sc[2] + sc[3]);
    __syncthreads();
    if ((tid & 63) == 0) { sc[tid >> 6] = rz; }
    __syncthreads();
    if (tid == 0) { blk_part[2 * blockIdx.x] = rr_b; blk_part[2 * blockIdx.x + 1] = (sc[0] + sc[1]) + (sc[2] + sc[3]); }
}

// part 2: totals of r.r and r.z ; beta = rz_new / rz_old ; z = pre r ; p = z + beta p ;
// scal[0] <- rz_new (block 0 publishes {rr, rz_new} for the host's convergence test)
__global__ __launch_bounds__(256) void k_pcg_step2(int n, int n_blk, double* __restrict__ scal,
                                                     const double* __restrict__ blk_part, const double* __restrict__ pre,
                                                     const double* __restrict__ r, double* __restrict__ p,
                                                     double* __restrict__ out2) {
    __shared__ double sc[4];
    __shared__ double s_beta;
    const int tid = threadIdx.x;
    double rr = 0.0, rz = 0.0;
    for (int i = tid; i < n_blk; i += 256) { rr += blk_part[2 * i]; rz += blk_part[2 * i + 1]; }
    rr = wave_sum(rr); rz = wave_sum(rz);
    if ((tid & 63) == 0) sc[tid >> 6] = rr;
    __syncthreads();
    const double rr_t = (sc[0] + sc[1]) + (sc[2] + sc[3]);
    __syncthreads();
    if ((tid & 63) == 0) sc[tid >> 6] = rz;
    __syncthreads();
    const double rz_t = (sc[0] + sc[1]) + (sc[2] + sc[3]);
    __shared__ int s_frozen;
    __shared__ int s_stop;
    if (tid == 0) {
        s_beta = rz_t / scal[0]; s_frozen = scal[4] != 0.0;
        // p.Ap ~ 0 or rz_old ~ 0 (a zero right-hand side: no camera columns, a converged start): the reference breaks before
        // it forms beta (:703-705, :741-743).  k_pcg_close_iteration freezes behind this kernel; beta = 0 / 0 must not reach p,
        // or the speculative iteration's x += 0 * p turns the untouched x into NaN
        s_stop = fabs(scal[1]) < 1e-30 || fabs(scal[0]) < 1e-30;
    }
    __syncthreads();
    if (s_frozen) return;   // (a speculative iteration behind a met termination test: p and the scalars stay)
    const double beta = s_beta;
    const int i = blockIdx.x * 256 + tid;
    if (i < n && !s_stop) p[i] = pre[i] * r[i] + beta * p[i];
    if (blockIdx.x == 0 && tid == 0) { out2[0] = rr_t; out2[1] = rz_t; }
}
// The end of a PCG iteration on the device (one thread): the reference's three termination tests on this iteration's scalars
// (explicit_schur.rs:703-705, 726-728, 741-743) -- met: scal[4] = 1, everything later is frozen; else rz_old := r.z.
// scal: ExplicitPcgScalars (pcg_kernels.h)
__global__ void k_pcg_close_iteration(double* __restrict__ scal, double abs_tol) {
    if (scal[4] != 0.0) return;
    if (fabs(scal[1]) < 1e-30 || sqrt(scal[2]) < abs_tol || fabs(scal[0]) < 1e-30) { scal[4] = 1.0; return; }
    scal[0] = scal[3];
}

// ---- small vector kernels for PCG (explicit_schur.rs:639-756) -----------------------------------
__global__ __launch_bounds__(256) void k_pcg_init(int n, const double* __restrict__ diag, const double* __restrict__ b,
                                                    double* __restrict__ pre, double* __restrict__ x,
                                                    double* __restrict__ r, double* __restrict__ z,
                                                    double* __restrict__ p) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const double d = diag[i];
    const double m = (fabs(d) > 1e-12) ? 1.0 / d : 1.0;
    pre[i] = m; x[i] = 0.0; r[i] = b[i];
    const double zi = m * b[i];
    z[i] = zi; p[i] = zi;
}

// out[0] = a.b  (single block, fixed order)
__global__ __launch_bounds__(256) void k_dot(int n, const double* __restrict__ a, const double* __restrict__ b,
                                               double* __restrict__ out) {
    __shared__ double sc[4];
    double s = 0.0;
    for (int i = threadIdx.x; i < n; i += 256) s += a[i] * b[i];
    s = wave_sum(s);
    if ((threadIdx.x & 63) == 0) sc[threadIdx.x >> 6] = s;
    __syncthreads();
    if (threadIdx.x == 0) out[0] = (sc[0] + sc[1]) + (sc[2] + sc[3]);
}

// ---- the matrix-free PCG with its scalars on the device (SchurJacobiPcg::solve reads them one iteration behind) ----------
// sc: ImplicitPcgScalars (pcg_kernels.h)
__global__ void k_pcg_implicit_begin(double* __restrict__ sc) { sc[4] = sc[0]; sc[5] = 0.0; sc[6] = 0.0; }   // (sc[0] = r.z of the start)
__global__ __launch_bounds__(256) void k_pcg_update_xr_sc(int n, const double* __restrict__ sc, const double* __restrict__ p,
                                                            const double* __restrict__ ap, double* __restrict__ x, double* __restrict__ r) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    const double pap = sc[2];
    if (i >= n || sc[5] != 0.0 || fabs(pap) < 1e-20) return;   // frozen, or the reference's break before the update (:610-613)
    const double alpha = sc[4] / pap;
    x[i] += alpha * p[i];
    r[i] -= alpha * ap[i];
}
// the reference's tests at the end of an iteration (implicit_schur.rs:610-613, 634-641, 652-654), else beta and the new rz_old
__global__ void k_pcg_implicit_close(double* __restrict__ sc, double abs_tol) {
    if (sc[5] != 0.0) return;
    if (fabs(sc[2]) < 1e-20 || sqrt(sc[0]) < abs_tol || fabs(sc[4]) < 1e-30) { sc[5] = 1.0; return; }
    sc[6] = sc[1] / sc[4];
    sc[4] = sc[1];
}
__global__ __launch_bounds__(256) void k_pcg_update_p_sc(int n, const double* __restrict__ sc, const double* __restrict__ z, double* __restrict__ p) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i < n && sc[5] == 0.0) p[i] = z[i] + sc[6] * p[i];
}

void launch_sym_tile_products(const SymTile* list, int n, const double* tiles, const double* x, double* part, hipStream_t s) {
    if (n > 0) hipLaunchKernelGGL(k_sym_tile_products, dim3(n), dim3(256), 0, s, list, tiles, x, part);
}
void launch_sym_tile_gather(int nt, const int* row_ptr, const SymEntry* entries, const double* part, const double* p,
                            double* y, double* row_dot, hipStream_t s) {
    hipLaunchKernelGGL(k_sym_tile_gather, dim3(nt), dim3(256), 0, s, row_ptr, entries, part, p, y, row_dot);
}
void launch_pcg_step1(int n, int nt, const double* scal, const double* row_dot, const double* p, const double* ap,
                      const double* pre, double* x, double* r, double* blk_part, double* out_pap, hipStream_t s) {
    hipLaunchKernelGGL(k_pcg_step1, dim3((n + 255) / 256), dim3(256), 0, s, n, nt, scal, row_dot, p, ap, pre, x, r, blk_part, out_pap);
}
void launch_pcg_step2(int n, double* scal, const double* blk_part, const double* pre, const double* r, double* p,
                      double* out2, double abs_tol, hipStream_t s) {
    const int nb = (n + 255) / 256;
    hipLaunchKernelGGL(k_pcg_step2, dim3(nb), dim3(256), 0, s, n, nb, scal, blk_part, pre, r, p, out2);
    hipLaunchKernelGGL(k_pcg_close_iteration, dim3(1), dim3(1), 0, s, scal, abs_tol);
}
void launch_pcg_init(int n, const double* diag, const double* b, double* pre, double* x, double* r, double* z, double* p,
                     hipStream_t s) {
    hipLaunchKernelGGL(k_pcg_init, dim3((n + 255) / 256), dim3(256), 0, s, n, diag, b, pre, x, r, z, p);
}
void launch_dot(int n, const double* a, const double* b, double* out, hipStream_t s) {
    hipLaunchKernelGGL(k_dot, dim3(1), dim3(256), 0, s, n, a, b, out);
}
void launch_pcg_implicit_begin(double* sc, hipStream_t s) { hipLaunchKernelGGL(k_pcg_implicit_begin, dim3(1), dim3(1), 0, s, sc); }
void launch_pcg_update_xr_sc(int n, const double* sc, const double* p, const double* ap, double* x, double* r, hipStream_t s) {
    hipLaunchKernelGGL(k_pcg_update_xr_sc, dim3((n + 255) / 256), dim3(256), 0, s, n, sc, p, ap, x, r);
}
void launch_pcg_implicit_close(double* sc, double abs_tol, hipStream_t s) { hipLaunchKernelGGL(k_pcg_implicit_close, dim3(1), dim3(1), 0, s, sc, abs_tol); }
void launch_pcg_update_p_sc(int n, const double* sc, const double* z, double* p, hipStream_t s) {
    hipLaunchKernelGGL(k_pcg_update_p_sc, dim3((n + 255) / 256), dim3(256), 0, s, n, sc, z, p);
}

// (set-up: Solver::set_structure loads this translation unit's code object on its background thread, as warm_chol_kernels does)
__global__ void k_warm_pcg_kernels() {}
void warm_pcg_kernels(hipStream_t s) { hipLaunchKernelGGL(k_warm_pcg_kernels, dim3(1), dim3(64), 0, s); }

}  // namespace apex
