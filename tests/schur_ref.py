"""Reference arithmetic for the Schur assembly tests (CPU only; tests/test_schur_ref_host.py, tests/test_gpu_schur_crafted.py).

A plain restatement of the explicit Schur complement, block by block, in np.longdouble (tile_ref.LD) with one dtype switch
for the numpy fp64 side of the referee rule.  Its inputs are what a handle exports per observation -- the corrected Jacobian
blocks Jc (2 x d_c, columns [pose 6 | intrinsics 3]) and Jl (2 x 3), the corrected residual r and the two index lists -- so
the linearisation is not on trial here.  Where lambda enters, the signs and the column order are np_ref.schur_dense's and the
oracle's:

    Hcc_c = sum_k Jc_k^T Jc_k + lambda I        g_c = sum_k Jc_k^T r_k            (k: observations of camera c)
    Hll_l = sum_k Jl_k^T Jl_k + lambda I        g_l = sum_k Jl_k^T r_k            (k: observations of landmark l)
    W_k   = Jc_k^T Jl_k                                                             (d_c x 3)
    S_ij  = [i == j] Hcc_i - sum_l sum_{a in obs(i, l)} sum_{b in obs(j, l)} W_a Hll_l^-1 W_b^T
    g_red = -g_c + sum_l W Hll_l^-1 g_l
    dl_l  = Hll_l^-1 (-g_l - sum_k W_k^T dc_cam(k))                                 (back-substitution for a given camera step)
    (S x)_i = Hcc_i x_i - sum_l W_il Hll_l^-1 (sum_j W_jl^T x_j)                    (matrix-free)

Every landmark must be in the plain-inverse regime of the eigenvalue gate (asserted by the callers through `cond`).

Pass condition of a camera-pair block:   err_ij <= max(8 e_np_ij, gamma(P_ij) M_ij)
  err_ij   max |S_dev - S_ld| over the d_c x d_c block
  e_np_ij  the same distance of the fp64 restatement (the project's referee rule, tile_ref.referee)
  M_ij     the magnitude of the block's own terms, [i == j] sum_k |Jc_k|^2 + sum_l |W_il| |Hll_l^-1| |W_jl| in spectral norms
           (an entry of a product is bounded by the product of the spectral norms) -- test_cheirality_and_no_loss's quantity
  P_ij     the number of terms summed into the block: ordered observation pairs (a, b) with cam(a) = i, cam(b) = j of a common
           landmark (so a pair on the diagonal counts twice: B + B^T), plus on the diagonal the camera's observations (Hcc).

gamma(P) = gamma_{P + C0}, gamma_m = m u / (1 - m u), u = 2^-53, C0 = 114.  Derivation (Higham, Accuracy and Stability, ch. 3):
a sum of P terms in ANY order (lanes, folds, atomics) is within gamma_{P-1} sum |terms|.  One term W_a Hll^-1 W_b^T is evaluated
as a chain of small products, N = Jl Hll^-1 (inner length 3), M = N Jl^T (3), U = Jc^T M (2), and the rank-2 update U V of 18
FMA per 3 x 3 sub-block (inner length 2, fused into the sum): gamma_{3+3+2+2} = gamma_10 relative to the product of the
norms.  Its four Jacobian factors are REBUILT from the projection record and the camera (ba_device.hpp, jac_from_rec): the
longest dependent chain from the inputs to an entry is 24 roundings (depth p_c.z 3, reciprocal 1, r2 2, r4 1, dist 2, t2 2,
t2 xn 1, dxx 1, f w inz 2, J00 1, J02 2, a 3, the pose column's cross product 2, the weight 1), each at most u relative to
the Jacobian's norm: 4 x 24 = 96.  The 3 x 3 inverse by cofactors is 8 roundings deep (minor 2, determinant 3 + 2, quotient 1)
relative to |Hll^-1|; what cond(Hll) adds to a BLOCK of S is not in gamma: it is the same for any fp64 evaluation and is what
the 8 e_np arm of the rule is for.  C0 = 10 + 96 + 8 = 114.  No factor for "safety" is applied and the constant is not fitted to
any device output.

Vectors pass the same rule row by row (a row = a camera or a landmark, err = max over its components), with the magnitude of
the row's own terms and the number of terms of its sum:
  g_red_i  sum_k |Jc_k| |r_k| + sum_l |W_il| |Hll_l^-1| sum_{k in l} |Jl_k| |r_k|        n_i + max_l k_l
  Hll^-1_l cond(Hll_l) |Hll_l^-1|                                                         k_l
  g_l      sum_k |Jl_k| |r_k|                                                             k_l
  dl_l     |Hll_l^-1| (sum_k |Jl_k| |r_k| + sum_k |W_k| |dc_cam(k)|)                      2 k_l
  (S x)_i  sum_j M_ij |x_j|   (matrix-free: |Hcc_i| |x_i| + sum_l |W_il| |Hll_l^-1| sum_j |W_jl| |x_j|)
                                                                                          max_j P_ij + d_c (partners of i + 1)
H_ll^-1 on its own carries cond(H_ll) in its magnitude: the inverse of a matrix known to a relative eps is known to
cond eps |H^-1| (Higham, section 14.1: |X^ - A^-1| <= c u cond(A) |A^-1| for any inversion method), eps being the rounding of
the k_l-term sum that forms H_ll and of the cofactors.  The first form of this module left cond out and relied on the 8 e_np
arm alone; the device then sat at up to 6.9 x the bound on single landmarks of cond 1e2..1e3 whose numpy inverse happened to
round well (errors of ~800 u |H^-1| against a cond of ~700: what a correct fp64 inverse gives).  The magnitude moved, C0 did
not; the blocks of S, g_red, the landmark step and S x keep the magnitudes without cond.
"""
from __future__ import annotations

import numpy as np

import tile_ref as tr
from tile_ref import LD, U, referee  # noqa: F401  (re-exported: the tests take them from here)

C0 = 114


def gamma(P):
    m = (np.asarray(P, dtype=np.float64) + C0) * U
    return m / (1.0 - m)


def inv3(B):
    """Inverse of (n, 3, 3) blocks by cofactors, in B's dtype (numpy's LAPACK does not take long double)."""
    m = lambda r, c: B[:, r, c]
    c00 = m(1, 1) * m(2, 2) - m(2, 1) * m(1, 2)
    c01 = m(1, 0) * m(2, 2) - m(2, 0) * m(1, 2)
    c02 = m(1, 0) * m(2, 1) - m(2, 0) * m(1, 1)
    det = m(0, 0) * c00 - m(0, 1) * c01 + m(0, 2) * c02
    out = np.empty_like(B)
    out[:, 0, 0] = c00; out[:, 0, 1] = m(0, 2) * m(2, 1) - m(2, 2) * m(0, 1); out[:, 0, 2] = m(0, 1) * m(1, 2) - m(1, 1) * m(0, 2)
    out[:, 1, 0] = -c01; out[:, 1, 1] = m(0, 0) * m(2, 2) - m(2, 0) * m(0, 2); out[:, 1, 2] = m(0, 2) * m(1, 0) - m(1, 2) * m(0, 0)
    out[:, 2, 0] = c02; out[:, 2, 1] = m(0, 1) * m(2, 0) - m(2, 1) * m(0, 0); out[:, 2, 2] = m(0, 0) * m(1, 1) - m(1, 0) * m(0, 1)
    return out / det[:, None, None]


def _scatter(n, idx, vals, dtype):
    out = np.zeros((n,) + vals.shape[1:], dtype=dtype)
    np.add.at(out, idx, vals)
    return out


def _n2(a):
    return np.linalg.norm(np.asarray(a, dtype=np.float64), ord=2, axis=(1, 2))


class SchurRef:
    """The Schur system of one linearisation in `dtype`.  dense=False leaves out S (S4, M, P): vectors and matvec only.
    hinv_given = {landmark: 3 x 3}: H_ll^-1 of these landmarks is taken as given, not computed.
    mags = (M_Jc, M_Jl, M_r): entrywise magnitudes >= |Jc|, |Jl|, |r| of blocks that are themselves on trial (projection_ref.py);
    every magnitude below is then formed from the norms of these instead of the blocks' own (|W| <= |M_Jc| |M_Jl|), and
    H_ll^-1 on its own gets, beside cond(H_ll), the relative magnitude of H_ll = sum_k Jl_k^T Jl_k + lambda I itself,
    kap_l = max(1, (sum_k (2 |M_Jl_k| |Jl_k| - |Jl_k|^2) + lambda) / |H_ll|) in spectral norms (the magnitude of a square is
    2 M |x| - x^2 to first order): cond eps |H^-1| with eps the relative uncertainty of H_ll."""

    def __init__(self, n_cam, n_pt, cam_idx, pt_idx, jc, jl, r, lam, dtype=LD, dense=True, chunk=20000, hinv_given=None, mags=None,
                 lam_cams=None):
        T = self.T = dtype
        # lam_cams (boolean per camera, None: all): the cameras whose H_cc carries lambda -- a shard's partial system (shard_cases.py)
        lam_c = np.where(np.ones(n_cam, dtype=bool) if lam_cams is None else np.asarray(lam_cams, dtype=bool), T(lam), T(0)).astype(T)
        self.n_cam, self.n_pt, self.lam = int(n_cam), int(n_pt), float(lam)
        ci = self.ci = np.asarray(cam_idx, dtype=np.int64); li = self.li = np.asarray(pt_idx, dtype=np.int64)
        Jc = np.asarray(jc, dtype=T); Jl = np.asarray(jl, dtype=T); rr = np.asarray(r, dtype=T).reshape(-1, 2)
        dc = self.dc = Jc.shape[2]
        eye_c, eye_l = np.eye(dc, dtype=T), np.eye(3, dtype=T)
        self.Hcc = _scatter(n_cam, ci, np.einsum("kra,krb->kab", Jc, Jc), T) + lam_c[:, None, None] * eye_c
        self.gc = _scatter(n_cam, ci, np.einsum("kra,kr->ka", Jc, rr), T)
        self.Hll = _scatter(n_pt, li, np.einsum("kra,krb->kab", Jl, Jl), T) + T(lam) * eye_l
        self.gl = _scatter(n_pt, li, np.einsum("kra,kr->ka", Jl, rr), T)
        self.Hinv = inv3(self.Hll)
        for l, h in (hinv_given or {}).items():       # a block inverse taken as given (landmark_cov_ref.py: a gated landmark)
            self.Hinv[l] = np.asarray(h, dtype=T)
        W = self.W = np.einsum("kra,krb->kab", Jc, Jl)                         # (n_obs, dc, 3)
        self.TW = np.einsum("kab,kbc->kac", W, self.Hinv[li])                  # W_k Hll^-1
        self.gred = -self.gc + _scatter(n_cam, ci, np.einsum("kab,kb->ka", self.TW, self.gl[li]), T)
        # magnitudes (fp64 is plenty for a bound)
        self.k_l = np.bincount(li, minlength=n_pt); self.n_i = np.bincount(ci, minlength=n_cam)
        self.wn, self.hn = _n2(W), _n2(self.Hinv)
        self.jcn, self.jln = _n2(Jc), _n2(Jl)
        self.rn = np.linalg.norm(np.asarray(rr, dtype=np.float64), axis=1)
        self.kap = np.ones(n_pt)
        if mags is not None:
            mjl = _n2(mags[1])
            mag_h = _scatter(n_pt, li, 2.0 * mjl * self.jln - self.jln ** 2, np.float64) + abs(lam)
            self.jcn, self.jln = _n2(mags[0]), mjl
            self.rn = np.linalg.norm(np.asarray(mags[2], dtype=np.float64).reshape(-1, 2), axis=1)
            self.wn = self.jcn * self.jln
        self.hcc_mag = _scatter(n_cam, ci, self.jcn ** 2, np.float64) + np.abs(lam_c.astype(np.float64))
        self.gl_mag = _scatter(n_pt, li, self.jln * self.rn, np.float64)
        self.gred_mag = _scatter(n_cam, ci, self.jcn * self.rn + self.wn * self.hn[li] * self.gl_mag[li], np.float64)
        kmax_i = np.zeros(n_cam, dtype=np.int64); np.maximum.at(kmax_i, ci, self.k_l[li])
        self.gred_terms = self.n_i + kmax_i
        ev = np.linalg.eigvalsh(np.asarray(self.Hll, dtype=np.float64))
        self.cond = ev[:, 2] / ev[:, 0]
        if mags is not None:
            self.kap = np.maximum(1.0, mag_h / ev[:, 2])
        self.hinv_mag = self.cond * self.hn * self.kap
        self.dense = dense
        if not dense:
            return
        # every ordered pair (a, b) of observations of one landmark, self pairs included
        order = np.argsort(li, kind="stable")
        ptr = np.concatenate([[0], np.cumsum(self.k_l)])
        k_of = self.k_l[li[order]]
        a = np.repeat(order, k_of)                                             # a repeated k_l times
        start = np.repeat(ptr[li[order]], k_of)
        within = np.arange(len(a)) - np.repeat(np.cumsum(k_of) - k_of, k_of)
        b = order[start + within]
        self.S4 = np.zeros((n_cam, n_cam, dc, dc), dtype=T)
        self.M = np.zeros((n_cam, n_cam)); self.P = np.zeros((n_cam, n_cam), dtype=np.int64)
        for s in range(0, len(a), chunk):
            aa, bb = a[s:s + chunk], b[s:s + chunk]
            np.subtract.at(self.S4, (ci[aa], ci[bb]), np.einsum("pac,pbc->pab", self.TW[aa], W[bb]))
            np.add.at(self.M, (ci[aa], ci[bb]), self.wn[aa] * self.hn[li[aa]] * self.wn[bb])
            np.add.at(self.P, (ci[aa], ci[bb]), 1)
        d = np.arange(n_cam)
        self.S4[d, d] += self.Hcc
        self.M[d, d] += self.hcc_mag; self.P[d, d] += self.n_i

    # ---- operations ---------------------------------------------------------------------------------------------------
    def back_substitute(self, dcam):
        """(n_cam, dc) camera step -> (n_pt, 3) landmark step and the magnitude of its terms."""
        x = np.asarray(dcam, dtype=self.T)
        rhs = -self.gl - _scatter(self.n_pt, self.li, np.einsum("kab,ka->kb", self.W, x[self.ci]), self.T)
        dl = np.einsum("lab,lb->la", self.Hinv, rhs)
        xn = np.linalg.norm(np.asarray(x, dtype=np.float64), axis=1)
        mag = self.hn * (self.gl_mag + _scatter(self.n_pt, self.li, self.wn * xn[self.ci], np.float64))
        return dl, mag

    def matvec(self, x):
        """(n_cam, dc) -> S x (n_cam, dc), matrix-free, and the magnitude sum_j M_ij |x_j| per camera."""
        x = np.asarray(x, dtype=self.T)
        t = _scatter(self.n_pt, self.li, np.einsum("kab,ka->kb", self.W, x[self.ci]), self.T)
        y = np.einsum("cab,cb->ca", self.Hcc, x) - _scatter(self.n_cam, self.ci, np.einsum("kab,kb->ka", self.TW, t[self.li]), self.T)
        xn = np.linalg.norm(np.asarray(x, dtype=np.float64), axis=1)
        tm = _scatter(self.n_pt, self.li, self.wn * xn[self.ci], np.float64)
        mag = self.hcc_mag * xn + _scatter(self.n_cam, self.ci, self.wn * self.hn[self.li] * tm[self.li], np.float64)
        return y, mag

    def matvec_terms(self):
        """Terms of row i of S x: the longest block of the row plus the dot products over its partners."""
        seen = np.zeros(self.n_cam, dtype=np.int64); np.maximum.at(seen, self.ci, self.k_l[self.li])
        partners = _scatter(self.n_cam, self.ci, self.k_l[self.li].astype(np.float64), np.float64).astype(np.int64)
        pmax = self.P.max(axis=1) if self.dense else self.n_i * 2 + seen
        return pmax + self.dc * (np.minimum(partners, self.n_cam) + 1)


def pair(n_cam, n_pt, cam_idx, pt_idx, jc, jl, r, lam, dense=True, lam_cams=None):
    """(long double reference, fp64 restatement) of one linearisation."""
    return (SchurRef(n_cam, n_pt, cam_idx, pt_idx, jc, jl, r, lam, LD, dense, lam_cams=lam_cams),
            SchurRef(n_cam, n_pt, cam_idx, pt_idx, jc, jl, r, lam, np.float64, dense, lam_cams=lam_cams))


# ---- column order ---------------------------------------------------------------------------------------------------------
def cam_cols(layout, n_cam, dc):
    """(n_cam, dc) reference columns of every camera's [pose 6 | intrinsics 3] entries."""
    cols = layout.pose_col[:n_cam, None] + np.arange(6)[None]
    if dc == 9:
        cols = np.concatenate([cols, layout.intr_col[:n_cam, None] + np.arange(3)[None]], axis=1)
    return cols


def blocks_of(S, cols):
    """Dense S in the reference column order -> (n_cam, n_cam, dc, dc)."""
    n, dc = cols.shape
    return np.ascontiguousarray(S[np.ix_(cols.ravel(), cols.ravel())].reshape(n, dc, n, dc).transpose(0, 2, 1, 3))


def dense_of(S4, cols, n, fill_diag=0.0):
    """(n_cam, n_cam, dc, dc) -> dense n x n in the reference column order; columns no block covers get fill_diag."""
    nc, dc = cols.shape
    out = np.zeros((n, n), dtype=S4.dtype)
    out[np.arange(n), np.arange(n)] = fill_diag
    out[np.ix_(cols.ravel(), cols.ravel())] = S4.transpose(0, 2, 1, 3).reshape(nc * dc, nc * dc)
    return out


# ---- the rule ---------------------------------------------------------------------------------------------------------------
def _ratio(err, bound):
    err = np.asarray(err, dtype=np.float64); bound = np.asarray(bound, dtype=np.float64)
    out = np.zeros_like(err)
    nz = bound > 0
    out[nz] = err[nz] / bound[nz]
    out[~nz & (err > 0)] = np.inf
    return out


def block_check(S4_dev, ld, f64):
    """Ratios err_ij / max(8 e_np_ij, gamma(P_ij) M_ij) (n_cam, n_cam) and the failing blocks [(i, j), ...], worst first.  A
    block without a common landmark has bound 0: anything but exact zeros fails it."""
    err = np.abs(np.asarray(S4_dev, dtype=LD) - ld.S4).max(axis=(2, 3)).astype(np.float64)
    e_np = np.abs(np.asarray(f64.S4, dtype=LD) - ld.S4).max(axis=(2, 3)).astype(np.float64)
    bound = np.maximum(8.0 * e_np, gamma(ld.P) * ld.M)
    bound[ld.P == 0] = 0.0
    ratio = _ratio(err, bound)
    bad = np.argwhere(ratio > 1.0)
    bad = sorted(((int(i), int(j)) for i, j in bad), key=lambda ij: -ratio[ij])
    return ratio, bad


def vec_check(dev, ref_ld, ref_64, mag, terms):
    """Row-wise ratios of the same rule for a vector quantity of shape (rows, ...)."""
    flat = lambda a: np.asarray(a, dtype=LD).reshape(len(mag), -1)
    err = np.abs(flat(dev) - flat(ref_ld)).max(axis=1).astype(np.float64)
    e_np = np.abs(flat(ref_64) - flat(ref_ld)).max(axis=1).astype(np.float64)
    return _ratio(err, np.maximum(8.0 * e_np, gamma(terms) * np.asarray(mag, dtype=np.float64)))


def worst(ratio):
    """(value, index tuple) of the largest ratio."""
    ratio = np.asarray(ratio)
    if ratio.size == 0:
        return 0.0, ()
    k = np.unravel_index(int(np.argmax(ratio)), ratio.shape)
    return float(ratio[k]), tuple(int(x) for x in k)


def report(label, ratios):
    """One SCHURREF line: the worst ratio of every checked quantity and where it sits."""
    parts = []
    for name, r in ratios.items():
        v, at = worst(r)
        parts.append(f"{name} {v:.3g}@{','.join(str(a) for a in at)}")
    print(f"SCHURREF {label}: " + "  ".join(parts))
