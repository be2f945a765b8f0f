// pg_kernels.hip -- pose-graph kernels: BetweenFactor linearisation fused with the block-sparse J^T J / J^T r assembly,
// trial cost, retraction, parity exports.
//
// Generic over the manifold M (Se3Manifold of pg_device.hpp | Se2Manifold of pg2_device.hpp | So3Manifold of pg_so3_device.hpp):
//   k_pg_prepare<M>       vertex-major  prepared poses of a parameter set (SE3::from(DVector) | SE2::from(DVector))
//   k_pg_cost_partial<M>  edge-major    1/2 |r~|^2 at a (trial) parameter set
//   k_pg_retract<M>       vertex-major  x (+) d with the fixed-DOF mask (src/core/problem.rs:185-197)
//   k_pg_prior_export<M>, k_pg_export<M>  parity exports
//   k_pg_jv_gram<M>       edge-major    |J a|^2, (J a).(J b), |J b|^2 matrix-free: the products with H = J^T J the Dog-Leg step needs
//                                       (dog_leg.rs:776-803, 948-960) once the tiles hold L instead of H; the rest of a Dog-Leg
//                                       step runs on plain vectors and lives in dogleg_kernels.hip
// Two assemblies.  The 3-DOF manifolds SE2 and SO3 are always row-owned; SE3 (6 x 6) is edge-major by default and row-owned
// on a handle given the option "row_owned_assembly" (launch_pg_assemble takes the handle's flag):
//   k_pg_edges      SE3  edge-major    r, dr/dk0, dr/dk1 per edge in registers (never written to memory), loss correction,
//                                      then H_aa += Ja^T Ja, H_bb += Jb^T Jb, H_(hi,lo) += J_hi^T J_lo, g_a += Ja^T r,
//                                      g_b += Jb^T r with fp64 atomics (SparseCholeskySolver's J^T J and J^T r,
//                                      src/linalg/sparse/cholesky.rs:166-181)
//   k_pg_priors     SE3  one lane per prior block, atomics
//   k_pg2_assemble<M>  SE2, SO3  vertex-major  lane v walks the edges incident to v (pg_row_assemble<M>): H_vv and g_v in registers,
//                                      blocks (v, u), u < v, by plain read-add-write -- row v of the lower triangle has
//                                      one writer, so there are no atomics and every sum has a fixed order: two
//                                      assemblies of one state are bit-identical.  An edge is linearised by both of its
//                                      endpoints (a few dozen flops) instead of scattering 24-byte segments atomically.
//   k_pg6_assemble<LP> SE3 under the option  vertex-major  the same over 6 x 6 blocks (pg_row_assemble6): every product formed as
//                                      k_pg_edges forms it, summed in list order instead of by atomics
//   k_pg2_priors<M>    every row-owned handle  one lane per run of prior blocks on one vertex (the blocks arrive sorted by vertex)
// Every kernel that linearises edges is instantiated per loss policy (pg_device.hpp): LossLegacy (huber_delta), LossGeneral
// (PgLoss), LossWeighted (PgLoss and the edge information matrices of PGView::info).
//
// HBM-bound and tiny next to the factorisation: per SE3 edge 2 x 64 B poses + 64 B measurement in,
// 3 x 288 B + 2 x 48 B of atomics out.
#include <hip/hip_runtime.h>

#include "device_reduce.hpp"
#include "pg2_device.hpp"
#include "pg_device.hpp"
#include "pg_kernels.h"
#include "pg_so3_device.hpp"

namespace apex {

// block i of N doubles (N even) by 16-byte loads
template <int N>
__device__ __forceinline__ void load_block(const double* __restrict__ base, int64_t i, double p[N]) {
    static_assert(N % 2 == 0, "16-byte loads");
    const double2* q = reinterpret_cast<const double2*>(base + N * i);
#pragma unroll
    for (int a = 0; a < N / 2; ++a) {
        const double2 t = q[a];
        p[2 * a] = t.x; p[2 * a + 1] = t.y;
    }
}
// one prepared pose / measurement: M::kStride doubles
template <class M>
__device__ __forceinline__ void load_pose(const double* __restrict__ base, int64_t i, double p[M::kStride]) {
    load_block<M::kStride>(base, i, p);
}

// DOF x DOF block (row vertex vr, column vertex vc, vr >= vc) of the lower-triangular tile matrix
template <int DOF>
__device__ __forceinline__ double* h_block_ptr(const TileMap& tm, uint32_t vr, uint32_t vc) {
    constexpr uint32_t vpt = kNB / DOF;   // vertices per 144-row tile: 24 | 48
    const uint32_t I = vr / vpt, J = vc / vpt;
    const int slot = tm.slot[(size_t)I * tm.nt + J];
    return tm.tiles + (size_t)slot * (kNB * kNB) + (size_t)((vr % vpt) * DOF) * kNB + (vc % vpt) * DOF;
}

// what the per-edge math of policy LP takes as its loss: the Huber delta | the PgLoss
template <class LP>
__device__ __forceinline__ const typename LP::Param& loss_param(const PGView& v) {
    if constexpr (LP::kGeneral) return v.loss;
    else return v.huber_delta;
}

// r0^2 + r1^2 + ... left to right, as the one expression it used to be spelled as
template <int N>
__device__ __forceinline__ double sumsq(const double r[N]) {
    double s = r[0] * r[0];
#pragma unroll
    for (int a = 1; a < N; ++a) s += r[a] * r[a];
    return s;
}

// LossWeighted: the instantiation that reads v.info
template <class LP>
constexpr bool kWeighted = std::is_same<LP, LossWeighted>::value;

// edge e's Omega, unpacked to full row-major D x D: InfoPack<D>::kStride doubles by 16-byte loads
template <int D>
__device__ __forceinline__ void load_info(const double* __restrict__ base, int64_t e, double W[D * D]) {
    constexpr int S = InfoPack<D>::kStride;
    double p[S];
    const double2* q = reinterpret_cast<const double2*>(base + S * e);
#pragma unroll
    for (int a = 0; a < S / 2; ++a) {
        const double2 t = q[a];
        p[2 * a] = t.x; p[2 * a + 1] = t.y;
    }
    info_unpack<D>(p, W);
}

// One prior block: the corrected residual (M::kAmb rows); returns sqrt(rho')
template <class M>
__device__ __forceinline__ double prior_at(const PGView& v, int k, double r[M::kAmb]) {
    const uint32_t a = v.prior_v[k];
    static_assert(M::kPriorStride > M::kAmb, "a prior block holds its Huber delta behind the datum");
    double x[M::kStride], d[M::kPriorStride];
    if constexpr (M::kPriorOnPrepared) {
        load_pose<M>(v.posep, a, x);
    } else {
#pragma unroll
        for (int i = 0; i < M::kAmb; ++i) x[i] = v.poses[M::kAmb * (size_t)a + i];
    }
    load_block<M::kPriorStride>(v.prior_data, k, d);   // data (kAmb) | the block's Huber delta
    return M::prior_residual(x, d, d[M::kAmb], r);
}

template <class M>
__global__ __launch_bounds__(256) void k_pg_prepare(int64_t n, const double* __restrict__ poses, double* __restrict__ posep) {
    const int64_t v = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (v >= n) return;
    double p[M::kAmb], o[M::kStride] = {};   // (the pad of an SE3 pose stays 0)
#pragma unroll
    for (int a = 0; a < M::kAmb; ++a) p[a] = poses[M::kAmb * v + a];
    M::prepare(p, o);
    double2* q = reinterpret_cast<double2*>(posep + M::kStride * v);
#pragma unroll
    for (int a = 0; a < M::kStride / 2; ++a) q[a] = make_double2(o[2 * a], o[2 * a + 1]);
}

// ---- SE3 assembly: edge-major, fp64 atomics ------------------------------------------------------------------------
__device__ __forceinline__ void atomic_add_lower6(double* blk, const double H[36]) {
#pragma unroll
    for (int i = 0; i < 6; ++i)
#pragma unroll
        for (int j = 0; j <= i; ++j) unsafeAtomicAdd(blk + i * kNB + j, H[6 * i + j]);
}
__device__ __forceinline__ void atomic_add_full6(double* blk, const double H[36]) {
#pragma unroll
    for (int i = 0; i < 6; ++i)
#pragma unroll
        for (int j = 0; j < 6; ++j) unsafeAtomicAdd(blk + i * kNB + j, H[6 * i + j]);
}

// The body of k_pg_edges<LossWeighted>: every block is G_ab = J_a^T Omega J_b under EdgeNormal6's correction.  Omega J_b is
// formed once per Jacobian (M) and serves the diagonal block and the cross block that has J_b on the right; the cross block
// of row vertex hi and column vertex lo is J_hi^T Omega J_lo -- G_ab is not symmetric in (a, b), so which Jacobian is
// transposed is decided by the vertex order, not by the edge's direction.
__device__ __forceinline__ void pg_edge_weighted(const PGView& v, const TileMap& tm, double* __restrict__ g, int64_t e, uint32_t a,
                                                 uint32_t b, const double k0[8], const double k1[8], const double m[8]) {
    double W[36], r[6];
    load_info<6>(v.info, e, W);
    Jac6 J0, J1;
    EdgeNormal6 nf;
    if (!between_linearize_weighted(k0, k1, m, v.loss, W, r, J0, J1, nf)) return;
    double M[36], H[36], gv[6];
    info_mul_jac(W, J0, M);   // Omega J0
    jt_mul(J0, M, H);
    nf.correct(H, nf.w0, nf.w0);
    atomic_add_lower6(h_block_ptr<6>(tm, a, a), H);
    if (a < b) {   // row b, column a: J1^T Omega J0
        jt_mul(J1, M, H);
        nf.correct(H, nf.w1, nf.w0);
        atomic_add_full6(h_block_ptr<6>(tm, b, a), H);
    }
    info_mul_jac(W, J1, M);   // Omega J1
    jt_mul(J1, M, H);
    nf.correct(H, nf.w1, nf.w1);
    atomic_add_lower6(h_block_ptr<6>(tm, b, b), H);
    if (a > b) {   // row a, column b: J0^T Omega J1
        jt_mul(J0, M, H);
        nf.correct(H, nf.w0, nf.w1);
        atomic_add_full6(h_block_ptr<6>(tm, a, b), H);
    } else if (a == b) {   // self-loop: the two cross terms G_01 + G_10 = G_01 + G_01^T land on the diagonal block
        jt_mul(J0, M, H);
        nf.correct(H, nf.w0, nf.w1);
        double* blk = h_block_ptr<6>(tm, a, a);
#pragma unroll
        for (int i = 0; i < 6; ++i)
#pragma unroll
            for (int j = 0; j <= i; ++j) unsafeAtomicAdd(blk + i * kNB + j, H[6 * i + j] + H[6 * j + i]);
    }
    nf.grad(nf.w0, gv);
#pragma unroll
    for (int i = 0; i < 6; ++i) unsafeAtomicAdd(g + (size_t)a * 6 + i, gv[i]);
    nf.grad(nf.w1, gv);
#pragma unroll
    for (int i = 0; i < 6; ++i) unsafeAtomicAdd(g + (size_t)b * 6 + i, gv[i]);
}

// LP = LossGeneral: J0, J1, r stay uncorrected and every block and gradient segment is corrected as it is formed
// (EdgeNormal6, pg_device.hpp); an edge whose rho' is 0 leaves before any block is formed.
template <class LP>
__global__ __launch_bounds__(256) void k_pg_edges(PGView v, TileMap tm, double* __restrict__ g) {
    const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (e >= v.n_e) return;
    const uint32_t a = v.e_from[e], b = v.e_to[e];
    double k0[8], k1[8], m[8], r[6];
    load_pose<Se3Manifold>(v.posep, a, k0);
    load_pose<Se3Manifold>(v.posep, b, k1);
    load_pose<Se3Manifold>(v.meas, e, m);
    if constexpr (kWeighted<LP>) { pg_edge_weighted(v, tm, g, e, a, b, k0, k1, m); return; }
    Jac6 J0, J1;
    [[maybe_unused]] EdgeNormal6 nf;
    if constexpr (LP::kGeneral) {
        if (!between_linearize_general(k0, k1, m, v.loss, r, J0, J1, nf)) return;
    } else {
        between_linearize(k0, k1, m, r, J0, J1);
        // loss correction: r and J scale by sqrt(rho') (corrector.rs:143-181; rho'' <= 0 for Huber)
        const double sc = pg_huber_scale(v.huber_delta, sumsq<6>(r));
        if (sc != 1.0) {
#pragma unroll
            for (int i = 0; i < 6; ++i) r[i] *= sc;
#pragma unroll
            for (int i = 0; i < 9; ++i) { J0.P[i] *= sc; J0.T[i] *= sc; J1.P[i] *= sc; J1.T[i] *= sc; }
        }
    }
    double H[36], gv[6];
    jtj(J0, J0, H);
    if constexpr (LP::kGeneral) nf.correct(H, nf.w0, nf.w0);
    {
        double* blk = h_block_ptr<6>(tm, a, a);
#pragma unroll
        for (int i = 0; i < 6; ++i)
#pragma unroll
            for (int j = 0; j <= i; ++j) unsafeAtomicAdd(blk + i * kNB + j, H[6 * i + j]);
    }
    jtj(J1, J1, H);
    if constexpr (LP::kGeneral) nf.correct(H, nf.w1, nf.w1);
    {
        double* blk = h_block_ptr<6>(tm, b, b);
#pragma unroll
        for (int i = 0; i < 6; ++i)
#pragma unroll
            for (int j = 0; j <= i; ++j) unsafeAtomicAdd(blk + i * kNB + j, H[6 * i + j]);
    }
    if (a != b) {
        double* blk;
        if (a > b) {
            jtj(J0, J1, H); blk = h_block_ptr<6>(tm, a, b);
            if constexpr (LP::kGeneral) nf.correct(H, nf.w0, nf.w1);
        } else {
            jtj(J1, J0, H); blk = h_block_ptr<6>(tm, b, a);
            if constexpr (LP::kGeneral) nf.correct(H, nf.w1, nf.w0);
        }
#pragma unroll
        for (int i = 0; i < 6; ++i)
#pragma unroll
            for (int j = 0; j < 6; ++j) unsafeAtomicAdd(blk + i * kNB + j, H[6 * i + j]);
    } else {  // self-loop: both Jacobians hit the same columns, the cross terms land on the diagonal block
        jtj(J0, J1, H);
        if constexpr (LP::kGeneral) nf.correct(H, nf.w0, nf.w1);   // (the rank-one term's two cross terms ride on H + H^T below)
        double* blk = h_block_ptr<6>(tm, a, a);
#pragma unroll
        for (int i = 0; i < 6; ++i)
#pragma unroll
            for (int j = 0; j <= i; ++j) unsafeAtomicAdd(blk + i * kNB + j, H[6 * i + j] + H[6 * j + i]);
    }
    if constexpr (LP::kGeneral) nf.grad(nf.w0, gv);
    else jtr(J0, r, gv);
#pragma unroll
    for (int i = 0; i < 6; ++i) unsafeAtomicAdd(g + (size_t)a * 6 + i, gv[i]);
    if constexpr (LP::kGeneral) nf.grad(nf.w1, gv);
    else jtr(J1, r, gv);
#pragma unroll
    for (int i = 0; i < 6; ++i) unsafeAtomicAdd(g + (size_t)b * 6 + i, gv[i]);
}

__global__ __launch_bounds__(64) void k_pg_priors(PGView v, TileMap tm, double* __restrict__ g) {
    const int k = blockIdx.x * 64 + threadIdx.x;
    if (k >= v.n_prior) return;
    double r[7];
    const double sc = prior_at<Se3Manifold>(v, k, r);
    const uint32_t a = v.prior_v[k];
    double* blk = h_block_ptr<6>(tm, a, a);
#pragma unroll
    for (int i = 0; i < 6; ++i) {   // J~ = sc [I6; 0]: J~^T J~ = sc^2 I6, J~^T r~ = sc r~[0..5]
        unsafeAtomicAdd(blk + i * kNB + i, sc * sc);
        unsafeAtomicAdd(g + (size_t)a * 6 + i, sc * r[i]);
    }
}

// ---- the 3-DOF manifolds' assembly (SE2, SO3): row-owned -----------------------------------------------------------
template <class M, class LP>
__global__ __launch_bounds__(256) void k_pg2_assemble(PGView v, TileMap tm, double* __restrict__ g) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= v.n_v) return;
    const uint32_t row = (uint32_t)i;
    double H[9], gv[3];
    const auto add_off = [&](uint32_t u, const double* B) {
        double* blk = h_block_ptr<3>(tm, row, u);
#pragma unroll
        for (int a = 0; a < 3; ++a)
#pragma unroll
            for (int b = 0; b < 3; ++b) blk[a * kNB + b] += B[3 * a + b];
    };
    if constexpr (kWeighted<LP>)
        pg_row_assemble_info<M>(row, v.posep, v.meas, v.e_from, v.e_to, v.inc_ptr, v.inc_edge, v.info, v.loss, H, gv, add_off);
    else
        pg_row_assemble<M>(row, v.posep, v.meas, v.e_from, v.e_to, v.inc_ptr, v.inc_edge, loss_param<LP>(v), H, gv, add_off);
    double* blk = h_block_ptr<3>(tm, row, row);   // (on top of the damping add_diag has put there)
#pragma unroll
    for (int a = 0; a < 3; ++a)
#pragma unroll
        for (int b = 0; b <= a; ++b) blk[a * kNB + b] += H[3 * a + b];
#pragma unroll
    for (int a = 0; a < 3; ++a) g[3 * (size_t)row + a] = gv[a];
}

// (a prior block has M::kAmb rows over the vertex's M::kDof columns: J~ = sc times the first kDof columns of I, so rows past
// them -- SO3's fourth, SE3's seventh -- count in the cost only)
template <class M>
__global__ __launch_bounds__(64) void k_pg2_priors(PGView v, TileMap tm, double* __restrict__ g) {
    constexpr int D = M::kDof;
    const int k = blockIdx.x * 64 + threadIdx.x;
    if (k >= v.n_prior) return;
    const uint32_t a = v.prior_v[k];
    if (k > 0 && v.prior_v[k - 1] == a) return;   // the first block of a vertex sums the whole run, in order
    double h = 0.0, gv[D] = {};
    for (int j = k; j < v.n_prior && v.prior_v[j] == a; ++j) {
        double r[M::kAmb];
        const double sc = prior_at<M>(v, j, r);   // J~ = sc [I_D; 0]: J~^T J~ = sc^2 I_D, J~^T r~ = sc r~[0..D)
        h += sc * sc;
#pragma unroll
        for (int i = 0; i < D; ++i) gv[i] += sc * r[i];
    }
    double* blk = h_block_ptr<D>(tm, a, a);
#pragma unroll
    for (int i = 0; i < D; ++i) {
        blk[i * kNB + i] += h;
        g[D * (size_t)a + i] += gv[i];
    }
}

// ---- SE3 assembly, row-owned (option "row_owned_assembly") -------------------------------------------------------
// Lane v walks the edges incident to v (pg_row_assemble6, pg_device.hpp): the diagonal block's lower triangle by plain
// read-add-write on top of the damping, the blocks (v, u), u < v, in full by plain read-add-write, g_v by a plain store.  kB:
// the workgroup size the instantiation is launched with (kRowBlock below); the per-lane state of a 6 x 6 row is what sets it.
template <class LP, int kB>
__global__ __launch_bounds__(kB) void k_pg6_assemble(PGView v, TileMap tm, double* __restrict__ g) {
    const int64_t i = (int64_t)blockIdx.x * kB + threadIdx.x;
    if (i >= v.n_v) return;
    const uint32_t row = (uint32_t)i;
    double H[36], gv[6];
    const auto add_off = [&](uint32_t u, const double* B) {
        double* blk = h_block_ptr<6>(tm, row, u);
#pragma unroll
        for (int a = 0; a < 6; ++a)
#pragma unroll
            for (int b = 0; b < 6; ++b) blk[a * kNB + b] += B[6 * a + b];
    };
    pg_row_assemble6<LP>(row, v.posep, v.meas, v.e_from, v.e_to, v.inc_ptr, v.inc_edge, v.info, loss_param<LP>(v), H, gv, add_off);
    double* blk = h_block_ptr<6>(tm, row, row);   // (on top of the damping add_diag has put there)
#pragma unroll
    for (int a = 0; a < 6; ++a)
#pragma unroll
        for (int b = 0; b <= a; ++b) blk[a * kNB + b] += H[6 * a + b];
#pragma unroll
    for (int a = 0; a < 6; ++a) g[6 * (size_t)row + a] = gv[a];
}
// lanes per workgroup of k_pg6_assemble<LP>: the largest at which the instantiation keeps its row in registers (no scratch)
template <class LP>
constexpr int kRowBlock = 256;

// ---- the kernels both manifolds share ------------------------------------------------------------------------------
template <class M>
__global__ __launch_bounds__(64) void k_pg_prior_export(PGView v, double* __restrict__ r_out) {
    const int k = blockIdx.x * 64 + threadIdx.x;
    if (k >= v.n_prior) return;
    double r[M::kAmb];
    (void)prior_at<M>(v, k, r);
    const int o = v.prior_slot ? v.prior_slot[k] : k;   // (sorted blocks go back to the caller's index)
    for (int a = 0; a < M::kAmb; ++a) r_out[M::kAmb * o + a] = r[a];
}

template <class M, class LP>
__global__ __launch_bounds__(256) void k_pg_cost_partial(PGView v, double* __restrict__ partial) {
    __shared__ double scratch[4];
    double acc = 0.0;
    if (blockIdx.x == 0)
        for (int k = threadIdx.x; k < v.n_prior; k += 256) {
            double r[M::kAmb];
            (void)prior_at<M>(v, k, r);
            acc = M::cost_add_prior(acc, r);
        }
    for (int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x; e < v.n_e; e += (int64_t)gridDim.x * 256) {
        double k0[M::kStride], k1[M::kStride], m[M::kStride], r[M::kDof];
        load_pose<M>(v.posep, v.e_from[e], k0);
        load_pose<M>(v.posep, v.e_to[e], k1);
        load_pose<M>(v.meas, e, m);
        M::residual(k0, k1, m, r);
        double s = sumsq<M::kDof>(r);
        if constexpr (kWeighted<LP>) {   // s = r^T Omega r
            double W[M::kDof * M::kDof];
            load_info<M::kDof>(v.info, e, W);
            s = info_sqnorm<M::kDof>(W, r);
        }
        if constexpr (LP::kGeneral) {   // |r~|^2 = residual_scaling^2 s: in the second arm that is not rho' s
            const double sc = pg_loss_corrector(v.loss, s).residual_scaling;
            acc += (sc * sc) * s;
        } else {
            const double sc = pg_huber_scale(v.huber_delta, s);
            acc += (sc * sc) * s;
        }
    }
    acc = block_sum_256(acc, scratch);
    if (threadIdx.x == 0) partial[blockIdx.x] = acc;
}

template <class M>
__global__ __launch_bounds__(256) void k_pg_retract(int64_t n_v, const double* __restrict__ poses,
                                                      const double* __restrict__ d, double sign,
                                                      const uint8_t* __restrict__ fix, double* __restrict__ poses_out) {
    const int64_t v = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (v >= n_v) return;
    double dd[M::kDof], p[M::kAmb], o[M::kAmb];
#pragma unroll
    for (int a = 0; a < M::kDof; ++a) dd[a] = fix[M::kDof * v + a] ? 0.0 : sign * d[M::kDof * v + a];
#pragma unroll
    for (int a = 0; a < M::kAmb; ++a) p[a] = poses[M::kAmb * v + a];
    M::plus(p, dd, o);
#pragma unroll
    for (int a = 0; a < M::kAmb; ++a) poses_out[M::kAmb * v + a] = o[a];
}

__global__ __launch_bounds__(256) void k_pg_negate(int64_t n, const double* __restrict__ x, double* __restrict__ y) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i < n) y[i] = -x[i];
}

template <class M, class LP>
__global__ __launch_bounds__(256) void k_pg_export(PGView v, double* __restrict__ r_out, double* __restrict__ j_out) {
    const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (e >= v.n_e) return;
    double k0[M::kStride], k1[M::kStride], m[M::kStride];
    load_pose<M>(v.posep, v.e_from[e], k0);
    load_pose<M>(v.posep, v.e_to[e], k1);
    load_pose<M>(v.meas, e, m);
    if constexpr (kWeighted<LP>) {
        double W[M::kDof * M::kDof];
        load_info<M::kDof>(v.info, e, W);
        M::export_edge_info(k0, k1, m, v.loss, W, r_out ? r_out + M::kDof * e : nullptr, j_out ? j_out + 2 * M::kDof * M::kDof * e : nullptr);
        return;
    }
    M::export_edge(k0, k1, m, loss_param<LP>(v), r_out ? r_out + M::kDof * e : nullptr,
                   j_out ? j_out + 2 * M::kDof * M::kDof * e : nullptr);
}

// ---- Dog-Leg -------------------------------------------------------------------------------------------------------
// g.Hg, g.Hh, h.Hh for H = J^T J without H: with u = J a, w = J b they are u.u, u.w, w.w, summed over the residual blocks.
// One pass over the edges and priors, each edge linearised as the assembly does (M::edge_jv); a, b in internal column order.
// A self-loop reads both of its vertex segments from the same place, so both Jacobians land on one vertex by themselves.  A
// prior block is J~ = sc [I_dof; 0]: it adds sc^2 a_v.a_v etc.  No atomics: partial[3 block + k], then k_sum_partials in index
// order -- two calls on one state give the same bits, on both manifolds.
template <class M, class LP>
__global__ __launch_bounds__(256) void k_pg_jv_gram(PGView v, const double* __restrict__ a, const double* __restrict__ b,
                                                     double* __restrict__ partial) {
    __shared__ double scratch[4];
    constexpr int D = M::kDof;
    double uu = 0.0, uw = 0.0, ww = 0.0;
    if (blockIdx.x == 0)
        for (int k = threadIdx.x; k < v.n_prior; k += 256) {
            double r[M::kAmb];
            const double sc = prior_at<M>(v, k, r);
            const size_t c = (size_t)D * v.prior_v[k];
            double aa = 0.0, ab = 0.0, bb = 0.0;
#pragma unroll
            for (int i = 0; i < D; ++i) {
                const double ai = a[c + i], bi = b[c + i];
                aa += ai * ai; ab += ai * bi; bb += bi * bi;
            }
            const double s2 = sc * sc;
            uu += s2 * aa; uw += s2 * ab; ww += s2 * bb;
        }
    for (int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x; e < v.n_e; e += (int64_t)gridDim.x * 256) {
        const uint32_t from = v.e_from[e], to = v.e_to[e];
        double k0[M::kStride], k1[M::kStride], m[M::kStride], a0[D], a1[D], b0[D], b1[D], u[D], w[D];
        load_pose<M>(v.posep, from, k0);
        load_pose<M>(v.posep, to, k1);
        load_pose<M>(v.meas, e, m);
#pragma unroll
        for (int i = 0; i < D; ++i) {
            a0[i] = a[(size_t)D * from + i]; a1[i] = a[(size_t)D * to + i];
            b0[i] = b[(size_t)D * from + i]; b1[i] = b[(size_t)D * to + i];
        }
        double su = 0.0, sx = 0.0, sw = 0.0;
        if constexpr (kWeighted<LP>) {   // u, w corrected but not whitened: the products close with Omega
            double W[D * D], Wu[D], Ww[D];
            load_info<D>(v.info, e, W);
            M::edge_jv_info(k0, k1, m, v.loss, W, a0, a1, b0, b1, u, w);
            info_mv<D>(W, u, Wu);
            info_mv<D>(W, w, Ww);
            su = dotn<D>(u, Wu); sx = dotn<D>(u, Ww); sw = dotn<D>(w, Ww);
        } else {
            M::edge_jv(k0, k1, m, loss_param<LP>(v), a0, a1, b0, b1, u, w);
#pragma unroll
            for (int i = 0; i < D; ++i) { su += u[i] * u[i]; sx += u[i] * w[i]; sw += w[i] * w[i]; }
        }
        uu += su; uw += sx; ww += sw;
    }
    uu = block_sum_256(uu, scratch);
    uw = block_sum_256(uw, scratch);
    ww = block_sum_256(ww, scratch);
    if (threadIdx.x == 0) { partial[3 * blockIdx.x] = uu; partial[3 * blockIdx.x + 1] = uw; partial[3 * blockIdx.x + 2] = ww; }
}

// ---- launchers -----------------------------------------------------------------------------------------------------
static inline int grid256(int64_t n) { return (int)((n + 255) / 256); }

// the one place a manifold id becomes a type: f is called with an Se3Manifold, an Se2Manifold or an So3Manifold
template <class F>
static inline void with_manifold(int manifold, F f) {
    if (manifold == kManifoldSE2) f(Se2Manifold{});
    else if (manifold == kManifoldSO3) f(So3Manifold{});
    else f(Se3Manifold{});
}
// the one place a view's loss becomes a policy type: the weighted instantiation when the view carries information matrices,
// else the legacy instantiation unless a loss was set through apexgpu_pg_set_loss
template <class F>
static inline void with_loss(const PGView& v, F f) {
    if (v.info) f(LossWeighted{});
    else if (v.loss.kind != kLossNone) f(LossGeneral{});
    else f(LossLegacy{});
}

void launch_pg_prepare(int manifold, int64_t n, const double* poses, double* posep, hipStream_t s) {
    if (n <= 0) return;
    with_manifold(manifold, [&](auto M) {
        hipLaunchKernelGGL(k_pg_prepare<decltype(M)>, dim3(grid256(n)), dim3(256), 0, s, n, poses, posep);
    });
}
void launch_pg_assemble(int manifold, bool row_owned, const PGView& v, const TileMap& tm, double* g, hipStream_t s) {
    const dim3 prior_grid((v.n_prior + 63) / 64);
    if (row_owned) {
        with_manifold(manifold, [&](auto M) {
            using Man = decltype(M);
            if (v.n_v > 0)
                with_loss(v, [&](auto LP) {
                    using L = decltype(LP);
                    if constexpr (Man::kDof == 3) {
                        hipLaunchKernelGGL((k_pg2_assemble<Man, L>), dim3(grid256(v.n_v)), dim3(256), 0, s, v, tm, g);
                    } else {
                        constexpr int B = kRowBlock<L>;
                        hipLaunchKernelGGL((k_pg6_assemble<L, B>), dim3((unsigned)((v.n_v + B - 1) / B)), dim3(B), 0, s, v, tm, g);
                    }
                });
            if (v.n_prior > 0) hipLaunchKernelGGL(k_pg2_priors<Man>, prior_grid, dim3(64), 0, s, v, tm, g);
        });
    } else {   // (SE3 only: pg_row_owned(manifold) handles are never assembled here)
        if (v.n_e > 0)
            with_loss(v, [&](auto LP) {
                hipLaunchKernelGGL(k_pg_edges<decltype(LP)>, dim3(grid256(v.n_e)), dim3(256), 0, s, v, tm, g);
            });
        if (v.n_prior > 0) hipLaunchKernelGGL(k_pg_priors, prior_grid, dim3(64), 0, s, v, tm, g);
    }
}
void launch_pg_prior_export(int manifold, const PGView& v, double* r_out, hipStream_t s) {
    if (v.n_prior <= 0) return;
    with_manifold(manifold, [&](auto M) {
        hipLaunchKernelGGL(k_pg_prior_export<decltype(M)>, dim3((v.n_prior + 63) / 64), dim3(64), 0, s, v, r_out);
    });
}
void launch_pg_cost(int manifold, const PGView& v, double* partial, int n_partial, double* out_sumsq, hipStream_t s) {
    with_manifold(manifold, [&](auto M) {
        with_loss(v, [&](auto LP) {
            hipLaunchKernelGGL((k_pg_cost_partial<decltype(M), decltype(LP)>), dim3(n_partial), dim3(256), 0, s, v, partial);
        });
    });
    launch_sum_partials(partial, n_partial, 1, out_sumsq, s);
}
void launch_pg_retract(int manifold, int64_t n_v, const double* poses, const double* d, double sign, const uint8_t* fix,
                       double* poses_out, hipStream_t s) {
    if (n_v <= 0) return;
    with_manifold(manifold, [&](auto M) {
        hipLaunchKernelGGL(k_pg_retract<decltype(M)>, dim3(grid256(n_v)), dim3(256), 0, s, n_v, poses, d, sign, fix, poses_out);
    });
}
void launch_pg_negate(int64_t n, const double* x, double* y, hipStream_t s) {
    if (n > 0) hipLaunchKernelGGL(k_pg_negate, dim3(grid256(n)), dim3(256), 0, s, n, x, y);
}
void launch_pg_export(int manifold, const PGView& v, double* r_out, double* j_out, hipStream_t s) {
    if (v.n_e <= 0) return;
    with_manifold(manifold, [&](auto M) {
        with_loss(v, [&](auto LP) {
            hipLaunchKernelGGL((k_pg_export<decltype(M), decltype(LP)>), dim3(grid256(v.n_e)), dim3(256), 0, s, v, r_out, j_out);
        });
    });
}

void launch_pg_jv_gram(int manifold, const PGView& v, const double* a, const double* b, double* partial, int n_partial,
                       double* out3, hipStream_t s) {
    with_manifold(manifold, [&](auto M) {
        with_loss(v, [&](auto LP) {
            hipLaunchKernelGGL((k_pg_jv_gram<decltype(M), decltype(LP)>), dim3(n_partial), dim3(256), 0, s, v, a, b, partial);
        });
    });
    launch_sum_partials(partial, n_partial, 3, out3, s);
}

}  // namespace apex
