"""Reference arithmetic for the landmark covariance tests (CPU only; tests/test_landmark_cov_ref_host.py,
tests/test_gpu_landmark_cov_crafted.py): the 3 x 3 landmark blocks of the inverse of the matrix a direct solve factorised,
landmark by landmark, from the per-observation blocks a handle exports (schur_ref.SchurRef: Jc, Jl, r and the index lists).

    Sigma_l = Hinv_l + sum_{i in obs(l)} sum_{j in obs(l)} U_i^T Z_{c(i) c(j)} U_j        U_i = W_i Hinv_l,  Z = S^-1

in np.longdouble, with Z from tile_ref's long double Cholesky and triangular inverse of the dense S, and every ORDERED pair
(i, j) summed as it stands -- one product of the landmark's stacked U with the k x k grid of Z blocks its cameras select.  The
same class with dtype = float64 and np.linalg.inv(S) is the fp64 restatement (e_np of the referee rule).  The device's kernel
(csrc/cov_kernels.hip) forms X + X^T over unordered pairs with a half weight on the diagonal, in chunks, per lane; none of
that is mirrored here.

Jacobi scaling.  The handle exports unscaled blocks; with a column scaling D on, the factorised matrix is D H D + lambda I and
the device returns D_l^-1 (hinv_l + ...) D_l^-1 with hinv_l = D_l V_l^-1 D_l its landmark record -- the landmark block of the
inverse of the SCALED matrix (tests/test_gpu_landmark_covariance.py, dense_reference; anchored on the camera blocks, which are
the diagonal blocks of Z).  The reference is therefore this module's formula on Jc D_c and Jl D_l.

Gated landmarks.  `hinv_dev` = {landmark: the 3 x 3 record the device exported}: the reference takes D_l^-1 hinv D_l^-1 in
place of its own inverse of that landmark's block, in S and in Sigma_l alike -- the covariance kernel is on trial, not the gate
(tests/test_gpu_gate_ladder.py owns that).

Pass condition of a landmark, entrywise on its 3 x 3 block:   err_l <= max(8 e_np_l, floor_l)
  err_l    |Sigma_dev - Sigma_ld|
  e_np_l   the same distance of the fp64 restatement (tile_ref.referee)
  floor_l  gamma(P_l + C0) M_l + 8 n u max(1, kappa(S)) M_l
  M_l      |Hinv_l| + sum_{i, j} |U_i|^T |Z_{c(i) c(j)}| |U_j|: the magnitude of the block's own terms
  P_l      k (k + 1) / 2 (d_c + 3), k the landmark's observations: the terms of its pair sum
  n        the columns of S (n_cam d_c); kappa(S) from the fp64 S of the reference, never from device output.
The second term is the Z floor of tests/test_gpu_tile_cholesky.py (8 n u max(1, kappa)): the device's Z is the selected inverse
of a backward-stable factor, not an exact inverse, and is known to kappa(S) u relative to its own size.

Given S.  `S_given` (n_cam d_c square, camera-major columns) replaces the S this module assembles.  The `gate` case passes the
device's own exported S there: the gated landmark's camera block is H_cc - W Hinv W^T with terms of 4e12 that cancel to 4e6, so
any fp64 assembly of it is off by a million times u |S_cc| -- 1.4 .. 2.5 x the floor when this module's long double S judged the
device there.  That is the assembly's rounding (tests/test_gpu_schur_crafted.py owns it), not the covariance pass's; with the
device's S taken as the matrix, Z and the kernel are judged against its exact inverse under the same two-term floor.

gamma(P) = gamma_{P + C0}, gamma_m = m u / (1 - m u), u = 2^-53, C0 = 35.  Derivation (Higham, Accuracy and Stability, ch. 3: a
sum of m terms in ANY order -- lanes, chunks, the butterfly -- is within gamma_{m-1} sum |terms|).  One elementary term of an
entry is Ui[a][p] Z[a][b] Uj[b][q].  Its two U factors (obs_u): the camera scale 1, the inner product of length two of
W = Jc^T Jl 2, the product with Hinv of length three 3: six roundings each, 12.  The Jacobians themselves are not on trial: the
kernel linearises with the functions of the export (ba_device.hpp, fp contraction off) and gives the same bits.  pair_term: row
a of Z Uj is a sum of d_c products, at most d_c = 9 roundings; folding it with Ui one product and at most d_c additions, 10;
the weight (1 or 1/2) is exact.  The pair sum itself -- at most k (k + 1) / 2 additions over lanes and the butterfly -- is inside
P_l.  After it: X + X^T 1, + Hinv 1, the product d_p d_q and the quotient of the point scaling 2.
C0 = 12 + 9 + 10 + 1 + 1 + 2 = 35.  The roundings of U are counted against |U| as the rule states M_l; what cond(Hll_l) adds to
Hinv_l is the same for any fp64 evaluation and is what the 8 e_np arm is for (schur_ref.py).  No factor for safety, nothing
fitted to device output.

Camera blocks (the anchor of the convention and of Z): err <= max(8 e_np, 8 n u max(1, kappa(S)) sqrt(Z_aa Z_bb)) entrywise --
|Z_ab| <= sqrt(Z_aa Z_bb) for a positive definite Z, so the magnitude does not lean on the entry's own cancellation.
"""
from __future__ import annotations

import numpy as np

import schur_ref as sr
import tile_ref as tr
from tile_ref import LD, U

C0 = 35
SMALL_K, CHUNK, GROUPS = 8, 32, 16       # kLcSmallK, kLcChunk (csrc/ba_kernels.h), groups of a small-landmark workgroup
NB = tr.NB


def gamma(P):
    m = (np.asarray(P, dtype=np.float64) + C0) * U
    return m / (1.0 - m)


def scaled_blocks(jc, jl, cam_idx, pt_idx, scale_c, scale_l, dtype):
    """Jc D_c, Jl D_l per observation in `dtype` (scale_c (n_cam, d_c), scale_l (n_pt, 3); None: unscaled)."""
    jc = np.asarray(jc, dtype=dtype); jl = np.asarray(jl, dtype=dtype)
    if scale_c is not None:
        jc = jc * np.asarray(scale_c, dtype=dtype)[np.asarray(cam_idx, dtype=np.int64)][:, None, :]
        jl = jl * np.asarray(scale_l, dtype=dtype)[np.asarray(pt_idx, dtype=np.int64)][:, None, :]
    return jc, jl


class LandmarkCovRef(sr.SchurRef):
    """SchurRef plus Z = S^-1 and the landmark blocks Sigma (n_pt, 3, 3), their magnitudes M and term counts P."""

    def __init__(self, n_cam, n_pt, cam_idx, pt_idx, jc, jl, r, lam, dtype=LD, scale_c=None, scale_l=None, hinv_dev=None, S_given=None):
        jc, jl = scaled_blocks(jc, jl, cam_idx, pt_idx, scale_c, scale_l, dtype)
        given = {}
        for l, h in (hinv_dev or {}).items():      # before S is formed: beside a plain inverse of cond > 1e10 the difference of the
            h = np.asarray(h, dtype=dtype)          # two W Hinv W^T would carry |W|^2 |Hinv| eps, far more than lambda
            if scale_l is not None:
                dl = np.asarray(scale_l, dtype=dtype)[l]
                h = h / dl[:, None] / dl[None, :]
            given[l] = h
        super().__init__(n_cam, n_pt, cam_idx, pt_idx, jc, jl, r, lam, dtype, dense=True, hinv_given=given)
        T, dc = self.T, self.dc
        self.order = np.argsort(self.li, kind="stable")
        self.ptr = np.concatenate([[0], np.cumsum(self.k_l)]).astype(np.int64)
        self.gated = sorted(given)
        n = self.n = n_cam * dc
        self.S = np.ascontiguousarray(self.S4.transpose(0, 2, 1, 3).reshape(n, n))
        self.kappa = float(np.linalg.cond(np.asarray(self.S, dtype=np.float64)))      # (of the reference's own S, also beside a given one)
        if S_given is not None:
            self.S = np.array(S_given, dtype=T)
            assert self.S.shape == (n, n) and np.array_equal(self.S, self.S.T)
        if T is LD:
            Li = tr.tri_inv_ld(tr.chol_ld(self.S))
            Z = Li.T @ Li
        else:
            Z = np.linalg.inv(self.S)
        self.Z4 = np.ascontiguousarray(Z.reshape(n_cam, dc, n_cam, dc).transpose(0, 2, 1, 3))
        self.Sigma = np.zeros((n_pt, 3, 3), dtype=T)
        self.M = np.zeros((n_pt, 3, 3))
        for l in range(n_pt):
            self.Sigma[l], self.M[l] = self.landmark(l)
        k = self.k_l.astype(np.int64)
        self.P_l = k * (k + 1) // 2 * (dc + 3)

    def obs(self, l):
        """The observations of landmark l (caller's indices, caller's order)."""
        return self.order[self.ptr[l]:self.ptr[l + 1]]

    def landmark(self, l):
        """(Sigma_l, M_l): every ordered pair of the landmark's observations, as one product over the stacked U."""
        o = self.obs(l)
        k, dc = len(o), self.dc
        c = self.ci[o]
        Uf = self.TW[o].reshape(k * dc, 3)
        Zs = self.Z4[c[:, None], c[None, :]].transpose(0, 2, 1, 3).reshape(k * dc, k * dc)
        sigma = self.Hinv[l] + Uf.T @ (Zs @ Uf)
        a = np.abs(np.asarray(Uf, dtype=np.float64))
        mag = np.abs(np.asarray(self.Hinv[l], dtype=np.float64)) + a.T @ (np.abs(np.asarray(Zs, dtype=np.float64)) @ a)
        return sigma, mag

    def z_floor(self):
        return 8.0 * self.n * U * max(1.0, self.kappa)

    def cam_blocks(self):
        """(n_cam, d_c, d_c) diagonal blocks of Z and their magnitudes sqrt(Z_aa Z_bb)."""
        d = np.arange(self.n_cam)
        Zd = self.Z4[d, d]
        dg = np.sqrt(np.abs(np.asarray(np.einsum("caa->ca", Zd), dtype=np.float64)))
        return Zd, dg[:, :, None] * dg[:, None, :]


def pair(n_cam, n_pt, cam_idx, pt_idx, jc, jl, r, lam, scale_c=None, scale_l=None, hinv_dev=None, S_given=None):
    """(long double reference, fp64 restatement) of one factorised system."""
    a = (n_cam, n_pt, cam_idx, pt_idx, jc, jl, r, lam)
    return (LandmarkCovRef(*a, LD, scale_c, scale_l, hinv_dev, S_given), LandmarkCovRef(*a, np.float64, scale_c, scale_l, hinv_dev, S_given))


def _ratio(err, bound):
    err = np.asarray(err, dtype=np.float64); bound = np.asarray(bound, dtype=np.float64)
    out = np.zeros_like(err)
    nz = bound > 0
    out[nz] = err[nz] / bound[nz]
    out[~nz & (err > 0)] = np.inf
    return out


def landmark_floor(ld):
    """floor_l (n_pt, 3, 3)"""
    return (gamma(ld.P_l)[:, None, None] + ld.z_floor()) * ld.M


def landmark_check(dev, ld, f64):
    """Per-landmark ratios max_entries err / max(8 e_np, floor) (n_pt,) of device blocks (n_pt, 3, 3)."""
    err = np.abs(np.asarray(dev, dtype=LD) - ld.Sigma).astype(np.float64)
    e_np = np.abs(np.asarray(f64.Sigma, dtype=LD) - ld.Sigma).astype(np.float64)
    floor = landmark_floor(ld)
    return _ratio(err, np.maximum(8.0 * e_np, floor)).max(axis=(1, 2))


def camera_check(dev, ld, f64):
    """Per-camera ratios of the same rule for the diagonal blocks of Z; dev (n_cam, >= d_c, >= d_c)."""
    dc = ld.dc
    Zd, mag = ld.cam_blocks()
    Z64, _ = f64.cam_blocks()
    err = np.abs(np.asarray(dev, dtype=LD)[:, :dc, :dc] - Zd).astype(np.float64)
    e_np = np.abs(np.asarray(Z64, dtype=LD) - Zd).astype(np.float64)
    return _ratio(err, np.maximum(8.0 * e_np, ld.z_floor() * mag)).max(axis=(1, 2))


def report(label, ratio, ld):
    """One LCOVREF line: the worst ratio, its landmark, that landmark's k, kappa(S)."""
    l = int(np.argmax(ratio))
    print(f"LCOVREF {label}: worst {float(ratio[l]):.3g} @ landmark {l} k {int(ld.k_l[l])}  kappa(S) {ld.kappa:.3g}")
    return l
