// sinv_kernels.hip -- the two kernels of the selected inversion (tile_sinv.h) and their launchers.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "tile_kernel_defs.h"
#include "tile_sinv.h"

namespace apex {

// ------------------------------------------------------------------------------------------
// Selected inversion (SelectedInverse, tile_sinv.h): batched tile products with a transpose option on either operand,
// summed over a list into one output tile.  The layout of k_tile_gemm_nt_small (chol_kernels.hip): NINE workgroups per output tile, one per
// 48 x 48 block, three waves each (wave w: rows 16 w.., three 16-wide column blocks), K in 48-wide chunks staged through
// LDS.  The staging absorbs the transposes: the LDS images are always sA[i][k] = op(A)[i][k] and sB[j][k] = op(B)[k][j],
// so the MFMA loop is the NT loop of the factorisation.  An operand whose LDS row is a row of its tile is copied
// straight ("direct"), otherwise each double2 of a tile row lands in two LDS rows.  The products of a task are summed in
// list order, each one chunk by chunk, four k per instruction: every element has one fixed summation order, so a
// repeated call is bitwise identical.  The C tile is only written.
// ------------------------------------------------------------------------------------------
__global__ __launch_bounds__(192) void k_sinv_gemm(const SinvTask* __restrict__ tasks, int n_units, const SinvProd* __restrict__ prods) {
    __shared__ double sA[48 * PS];
    __shared__ double sB[48 * PS];
    const int unit = blockIdx.x;
    if (unit >= n_units) return;
    const SinvTask tk = tasks[unit / 9];
    const int blk = unit % 9, bi = blk / 3, bj = blk % 3;
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    const int lr = lane & 15, lk = lane >> 4;
    constexpr int C2 = KS / 2, NR = 48 * C2 / 192;   // a 48 x 48 chunk of either operand: six double2 per thread
    double4_t acc[3];
#pragma unroll
    for (int j = 0; j < 3; ++j) acc[j] = (double4_t){0.0, 0.0, 0.0, 0.0};
    f64x2_t ra[NR], rb[NR];
    int op_ld = 0;
    // step s: product s / 3, K chunk s % 3.  direct A: rows 48 bi.. of A, columns k0..; transposed: rows k0.., columns 48 bi..
    // direct B (op(B) = B^T): rows 48 bj.. of B, columns k0..; otherwise rows k0.., columns 48 bj..
    auto gload = [&](int step) {
        const SinvProd p = prods[tk.first + step / 3];
        const int k0 = (step % 3) * KS;
        op_ld = p.op;
        const bool da = (p.op & kSinvTransA) == 0, db = (p.op & kSinvTransB) != 0;
        GlobalCF64 Ag = (GlobalCF64)p.A + (da ? (size_t)(48 * bi) * NB + k0 : (size_t)k0 * NB + 48 * bi);
        GlobalCF64 Bg = (GlobalCF64)p.B + (db ? (size_t)(48 * bj) * NB + k0 : (size_t)k0 * NB + 48 * bj);
#pragma unroll
        for (int i = 0; i < NR; ++i) {
            const int idx = tid + 192 * i, row = idx / C2, c2 = idx % C2;
            ra[i] = *reinterpret_cast<GlobalCF64x2>(Ag + (size_t)row * NB + 2 * c2);
            rb[i] = *reinterpret_cast<GlobalCF64x2>(Bg + (size_t)row * NB + 2 * c2);
        }
    };
    auto stage = [&](double* s, const f64x2_t* r, bool direct) {
#pragma unroll
        for (int i = 0; i < NR; ++i) {
            const int idx = tid + 192 * i, row = idx / C2, c2 = idx % C2;
            if (direct) { s[row * PS + 2 * c2] = r[i].x; s[row * PS + 2 * c2 + 1] = r[i].y; }
            else { s[(2 * c2) * PS + row] = r[i].x; s[(2 * c2 + 1) * PS + row] = r[i].y; }
        }
    };
    const int n_steps = 3 * tk.count;
    if (n_steps > 0) gload(0);
    for (int step = 0; step < n_steps; ++step) {
        const int op = op_ld;
        __syncthreads();
        stage(sA, ra, (op & kSinvTransA) == 0);
        stage(sB, rb, (op & kSinvTransB) != 0);
        __syncthreads();
        if (step + 1 < n_steps) gload(step + 1);
        const double sgn = (op & kSinvNeg) ? -1.0 : 1.0;
#pragma unroll
        for (int kk = 0; kk < KS; kk += 4) {
            const double a = sgn * sA[(16 * w + lr) * PS + kk + lk];
#pragma unroll
            for (int j = 0; j < 3; ++j) {
                const double b = sB[(16 * j + lr) * PS + kk + lk];
                acc[j] = __builtin_amdgcn_mfma_f64_16x16x4f64(a, b, acc[j], 0, 0, 0);
            }
        }
    }
    GlobalF64 C = (GlobalF64)tk.C + (size_t)bi * 48 * NB + bj * 48;
#pragma unroll
    for (int j = 0; j < 3; ++j)
#pragma unroll
        for (int r = 0; r < 4; ++r) C[(size_t)(16 * w + lk + 4 * r) * NB + 16 * j + lr] = acc[j][r];
}

__global__ void k_sinv_diag_blocks(const double* __restrict__ z, const int* __restrict__ diag_slot, const int64_t* __restrict__ pos,
                                   int64_t n_var, int d, double* __restrict__ out) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int64_t dd = (int64_t)d * d;
    if (i >= n_var * dd) return;
    const int64_t v = i / dd;
    const int a = (int)((i - v * dd) / d), b = (int)(i - v * dd - (int64_t)a * d);
    const int64_t p = pos[v];
    const int t = (int)(p / NB), o = (int)(p - (int64_t)t * NB);
    const double* Z = z + (size_t)diag_slot[t] * NB * NB;
    out[i] = 0.5 * (Z[(size_t)(o + a) * NB + o + b] + Z[(size_t)(o + b) * NB + o + a]);
}

void launch_sinv_gemm(const SinvTask* tasks, int n_tasks, const SinvProd* prods, hipStream_t s) {
    if (n_tasks > 0) hipLaunchKernelGGL(k_sinv_gemm, dim3(9 * n_tasks), dim3(192), 0, s, tasks, 9 * n_tasks, prods);
}
void launch_sinv_diag_blocks(const double* z, const int* diag_slot, const int64_t* pos, int64_t n_var, int d, double* out, hipStream_t s) {
    const int64_t n = n_var * d * d;
    if (n > 0) hipLaunchKernelGGL(k_sinv_diag_blocks, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, z, diag_slot, pos, n_var, d, out);
}

}  // namespace apex
