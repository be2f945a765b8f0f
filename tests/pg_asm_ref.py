"""Reference arithmetic for the pose-graph assembly tests (CPU only; tests/test_pg_asm_ref_host.py, tests/test_gpu_pg_crafted.py).

A plain restatement of the block-sparse normal equations of a pose graph, vertex pair by vertex pair, in np.longdouble
(tile_ref.LD) with one dtype switch for the numpy fp64 side of the referee rule.  Its inputs are what a handle exports per
edge -- the corrected Jacobian blocks J~_e = [J~_e,from | J~_e,to] (D x 2 D, whitened when information matrices are set), the
corrected residual r~_e and the two index lists -- plus the prior blocks (vertex, corrected residual r~, sc = sqrt(rho') of the
block's Huber loss; J~ = sc [I_D; 0]), so the linearisation is not on trial here: WHERE the kernels put the products is.

    H_vv  = lambda I + sum_{e at v} J~_ev^T J~_ev (+ J~_e0^T J~_e1 + its transpose for a self-loop) + sum_{priors on v} sc^2 I
    H_vu  = sum_{e between v and u} J~_ev^T J~_eu                      (v > u stored; the export must be exactly symmetric)
    g_v   = sum_{e at v} J~_ev^T r~_e + sum_{priors on v} sc r~[:D]
    cost  = 1/2 (sum |r~_e|^2 + sum |r~_prior|^2)
    (u.u, u.w, w.w),  u_e = J~_e0 a_from + J~_e1 a_to,  w likewise with b;  a prior adds sc^2 (a_v.a_v, a_v.b_v, b_v.b_v)
Column scaling s (Jacobi): every J~ column and prior column is multiplied by its s before anything is formed; lambda is added
after (PoseGraphSolver::assemble).

Pass condition of a D x D block, a vertex row of g, the cost and the jv-Gram sums:   err <= max(8 e_np, gamma(P + C0) M)
  err   max |dev - ld| over the block            e_np  the same distance of the fp64 restatement (tile_ref.referee's rule)
  P     the number of terms summed into it: edge ends at v (a self-loop: its two ends and its two cross terms), priors on v and
        lambda for H_vv; edges between the pair for H_vu; edge ends and priors for g_v; n_e + n_prior for the scalars.  Edges
        whose rho' is 0 are not terms: the kernels leave before any block is formed.  A block with no term at all has bound 0:
        it must be exactly lambda I, a gradient row exactly 0, a pair without an edge exactly 0.
  M     the magnitude of the terms THE KERNEL sums, in spectral norms (an entry of a product is bounded by the product of the
        norms):
          no loss, huber_delta (LossLegacy)  J is scaled by sqrt(rho') and multiplied: |J~_a| |J~_b|, |J~_a| |r~| -- the exports'
          LossGeneral    EdgeNormal6::correct forms rho' (J_a^T J_b - kap w_a w_b^T), w = J^T r, kap = a (2 - a s), from the
                         UNcorrected blocks: rho' (|J_a| |J_b| + |kap| |w_a| |w_b|);  g: |gsc| |J_a| |r|
          LossWeighted   the same with G_ab = J_a^T Omega J_b from UNwhitened Jacobians and w = J^T Omega r:
                         rho' (|J_a| |Omega| |J_b| + |kap| |w_a| |w_b|);  g: |gsc| |J_a| |Omega| |r|
        (SE3's forms; SE2's row kernels multiply corrected factors, see "SE2" below.  The uncorrected, unwhitened blocks and
        the corrector's scalars come from the numpy references, tests/loss_graphs.linearize and np_ref_loss, not from
        U_e^-1 J~ of the export: the same J to a few ulp, without a triangular solve per edge, and the device test holds the
        exports to those references and get_information to the Omega used here; fp64 is plenty for a bound).  jv-Gram: per edge m_x = f (|J_0| |x_from| + |J_1| |x_to|), f = 1 on the exports, sqrt(rho' |Omega|) (1 + a s) on
        the uncorrected blocks; M = sum m_a m_b.  Cost: sum |r~|^2.

gamma(P) = gamma_{P + C0}, gamma_m = m u / (1 - m u), u = 2^-53 (Higham, Accuracy and Stability, ch. 3: a sum of P terms in ANY
order -- lanes, atomics, a row's walk -- is within gamma_{P-1} sum |terms|).  C0 = 2 LIN + PROD counts the roundings of one term:

LIN  The kernels REBUILD the linearisation in registers; nothing is read from the export kernel's output.  Both call the same
     inline function, but the compiler contracts multiply-adds per kernel, so the two evaluations may differ by the roundings
     of the longest dependent chain from the prepared poses to a Jacobian entry, each at most u relative to the factor's norm.
     SE3 (pg_device.hpp, between_linearize): se3_inv 7 (two cross products 4, scale 1, sums 2), two se3_mul 8 each, so3_log 7,
     so3_left_jacobian_inv 12, r = D t 3, se3_q_block 15, D Q D 6, B R_m 3, the sum with D T_m 1: LIN = 70.  SE2 (pg2_device.hpp
     / np_ref_se2.between_linearize): K1^-1 K0 4, (.) M 3, Log 9, right_jacobian_inv 8, two 3 x 3 products 6: LIN = 30.
     A block has two such factors (for g the residual's chain is a prefix of the Jacobian's): 2 LIN.
PROD the products, with D = 6 | 3:
     legacy    the scale by sqrt(rho') once per factor 2, the inner product of length D (the SE3 T^T T + P^T P block: one more
               addition) D + 1:                                                        PROD = D + 3
     general   the kernel: part A rho' (1) times (J^T J (D + 1) minus (1)) and its product (1): D + 4; part B kap (a s, 2 - a s,
               the product: 3) times w_a (D + 1) times w_b (D + 1), two products, the subtraction, rho' and its product: 2 D + 10;
               the larger counts, relative to M.  The export: J~ = sqrt(rho') (J - a r (r^T J)) is D + 4 roundings per factor
               relative to sqrt(rho') |J| (1 + a s); a s = alpha is in [0, 1], so a product of two such factors carries
               2 x (D + 4) x (1 + alpha)^2 <= 8 (D + 4) relative to rho' |J_a| |J_b| <= M.  The corrector's scalars (rho', rho'',
               the discriminant, two square roots, alpha: 10) are rebuilt too.            PROD = 2 D + 10 + 8 (D + 4) + 10 = 10 D + 52
     weighted  the kernel: Omega J_b (D + 1) and J_a^T (.) (D + 1) in place of J^T J, w = J^T (Omega r) 2 D + 2 each:
               3 + 2 (2 D + 2) + 5 = 4 D + 12.  The export whitens with U of its own Cholesky, U^T U = Omega + E,
               |E| <= gamma_{D+1} |Omega|: D + 1 relative to |J_a| |Omega| |J_b|; a factor is (Omega r)^T J 2 D, a 1, r w 1, the
               subtraction 1, U (.) D, sqrt(rho') 1 = 3 D + 4, as above times 8; the corrector 10.
                                                                                         PROD = 4 D + 12 + D + 1 + 8 (3 D + 4) + 10 = 29 D + 55
     Under column scaling the export scales each factor once more: + 2.
SE2  The general and weighted chains above are SE3's (EdgeNormal6, pg_edge_weighted).  The SE2 row kernels never form
     rho' (J^T J - kap w w^T): pg2_assemble_row multiplies the corrected factors of between2_corrected, and pg2_assemble_row_info
     forms J^ = sqrt(rho') (J - a r (Omega r)^T J) and then J^_v^T (Omega J^_u).  So the SE2 magnitude is that of those
     products, rho' (1 + a s)^2 |J_a| |Omega| |J_b| and sqrt(rho') residual_scaling (1 + a s) |J_a| |Omega| |r| (edge_magnitudes,
     D = 3; equal to the SE3 form when a = 0, as for Cauchy and Tukey), and the SE2 chain is shorter than the one counted:
     general: the two factors (D + 4 each, as the export's) and the product D + 1, against the same factors in the export --
     at most 8 (D + 4) + D + 1 < 10 D + 52; weighted: Omega r D, the factor 2 D + 4, Omega J^ D + 1, the product D + 1, against
     the export's whitening -- at most 4 D + 6 + D + 1 + 8 (3 D + 4) + 10 < 29 D + 55.  SE2 keeps the SE3 constants as upper
     bounds: one table, and nothing is fitted.
A prior block is sc^2 and sc r~ (one product each) on an sc that the reference takes from the numpy restatement of the prior's
Huber scale (delta / sqrt(s), two square roots, the squared norm: under 12 roundings): covered by every PROD.
No factor for "safety" is applied and no constant is fitted to a device output.
"""
from __future__ import annotations

import numpy as np

from tile_ref import LD, U  # noqa: F401  (re-exported: the tests take them from here)

NB = 144
LIN = {6: 70, 3: 30}
POLICIES = ("legacy", "general", "weighted")


def c0(D, policy, scaled=False):
    prod = {"legacy": D + 3, "general": 10 * D + 52, "weighted": 29 * D + 55}[policy]
    return 2 * LIN[D] + prod + (2 if scaled else 0)


def gamma(P, C0):
    m = (np.asarray(P, dtype=np.float64) + C0) * U
    return m / (1.0 - m)


def _n2(a):
    a = np.asarray(a, dtype=np.float64)
    return np.linalg.norm(a, ord=2, axis=(1, 2)) if len(a) else np.zeros(0)


def _vn(a):
    return np.linalg.norm(np.asarray(a, dtype=np.float64), axis=1)


def edge_magnitudes(D, J, r, raw=None, corr=None, info=None):
    """Per-edge magnitudes of the terms the kernel sums (module docstring).  J, r: the exported corrected blocks.  raw = (r, J)
    uncorrected and unwhitened and corr = (sqrt_rho1, residual_scaling, alpha_sq_norm, s) per edge select the general
    policies; info (n_e, D, D) the weighted one.  -> dict of (n_e,) arrays haa hbb hab ga gb ja jb f and live (bool)."""
    n_e = len(r)
    if raw is None:
        na, nb, nr = _n2(np.asarray(J)[:, :, :D]), _n2(np.asarray(J)[:, :, D:]), _vn(r)
        return dict(haa=na * na, hbb=nb * nb, hab=na * nb, ga=na * nr, gb=nb * nr, ja=na, jb=nb, f=np.ones(n_e), live=np.ones(n_e, dtype=bool))
    r0, J0 = (np.asarray(x, dtype=np.float64) for x in raw)
    sq, rs, a, s = (np.asarray(x, dtype=np.float64) for x in corr)
    W = np.broadcast_to(np.eye(D), (n_e, D, D)) if info is None else np.asarray(info, dtype=np.float64)
    nW = _n2(W)
    Wr = np.einsum("kij,kj->ki", W, r0)
    na, nb, nr = _n2(J0[:, :, :D]), _n2(J0[:, :, D:]), _vn(r0)
    wa, wb = _vn(np.einsum("kra,kr->ka", J0[:, :, :D], Wr)), _vn(np.einsum("kra,kr->ka", J0[:, :, D:], Wr))
    rho1, alpha = sq * sq, a * s
    kap = np.abs(a * (2.0 - alpha))
    gsc = np.abs(sq * rs * (1.0 - alpha))
    live = sq != 0.0
    if D == 3:    # SE2: products of the corrected factors J^ = sqrt(rho') (J - a r w^T), |J^| <= sqrt(rho') (1 + a s) |J|
        grow = (1.0 + np.abs(alpha)) ** 2
        h = lambda x, y, wx, wy: np.where(live, rho1 * grow * x * nW * y, 0.0)
        gsc = np.abs(sq * rs) * (1.0 + np.abs(alpha))
    else:
        h = lambda x, y, wx, wy: np.where(live, rho1 * (x * nW * y + kap * wx * wy), 0.0)
    return dict(haa=h(na, na, wa, wa), hbb=h(nb, nb, wb, wb), hab=h(na, nb, wa, wb), ga=np.where(live, gsc * na * nW * nr, 0.0),
                gb=np.where(live, gsc * nb * nW * nr, 0.0), ja=na, jb=nb, f=np.where(live, sq * np.sqrt(nW) * (1.0 + np.abs(alpha)), 0.0), live=live)


class PgAsmRef:
    """The normal equations of one linearisation in `dtype`, as blocks: Hd (n_v, D, D), Ho (n_pair, D, D) for the pairs
    (hi, lo), hi > lo, of `pairs`; g (n_v, D); cost.  Magnitudes and term counts in fp64 / int64."""

    def __init__(self, D, n_v, e_from, e_to, J, r, lam, priors=None, mags=None, scaling=None, dtype=LD):
        T = self.T = dtype
        self.D, self.n_v, self.lam = D, int(n_v), float(lam)
        ef = self.ef = np.asarray(e_from, dtype=np.int64); et = self.et = np.asarray(e_to, dtype=np.int64)
        J = np.asarray(J, dtype=T); r = self.r = np.asarray(r, dtype=T)
        Ja, Jb = J[:, :, :D], J[:, :, D:]
        mags = dict(edge_magnitudes(D, J, r) if mags is None else mags)
        pv, pr, psc = priors if priors is not None else (np.zeros(0, np.int64), np.zeros((0, D)), np.zeros(0))
        pv = self.pv = np.asarray(pv, dtype=np.int64); pr = self.pr = np.asarray(pr, dtype=T); psc = self.psc = np.asarray(psc, dtype=T)
        s = np.ones((n_v, D), dtype=T) if scaling is None else np.asarray(scaling, dtype=T).reshape(n_v, D)
        smax = np.abs(np.asarray(s, dtype=np.float64)).max(axis=1)
        if scaling is not None:
            Ja = Ja * s[ef][:, None, :]; Jb = Jb * s[et][:, None, :]
            for k, (x, y) in dict(haa=(ef, ef), hbb=(et, et), hab=(ef, et)).items():
                mags[k] = mags[k] * smax[x] * smax[y]
            mags["ga"] = mags["ga"] * smax[ef]; mags["gb"] = mags["gb"] * smax[et]
            mags["ja"] = mags["ja"] * smax[ef]; mags["jb"] = mags["jb"] * smax[et]
        self.Ja, self.Jb, self.mags = Ja, Jb, mags
        live = mags["live"]
        loop = self.loop = ef == et
        Haa = np.einsum("kra,krb->kab", Ja, Ja); Hbb = np.einsum("kra,krb->kab", Jb, Jb); Hab = np.einsum("kra,krb->kab", Ja, Jb)
        self.Hd = np.zeros((n_v, D, D), dtype=T)
        np.add.at(self.Hd, ef, Haa); np.add.at(self.Hd, et, Hbb)
        np.add.at(self.Hd, ef[loop], Hab[loop] + Hab[loop].transpose(0, 2, 1))
        x = ~loop
        hi, lo = np.maximum(ef, et)[x], np.minimum(ef, et)[x]
        blk = np.where((ef > et)[x][:, None, None], Hab[x], Hab[x].transpose(0, 2, 1))      # row hi, column lo: J_hi^T J_lo
        key, inv = np.unique(hi * n_v + lo, return_inverse=True)
        self.pairs = np.stack([key // n_v, key % n_v], axis=1) if len(key) else np.zeros((0, 2), dtype=np.int64)
        self.pair_of_edge = np.full(len(ef), -1, dtype=np.int64); self.pair_of_edge[x] = inv
        self.Ho = np.zeros((len(key), D, D), dtype=T)
        np.add.at(self.Ho, inv, blk)
        self.g = np.zeros((n_v, D), dtype=T)
        np.add.at(self.g, ef, np.einsum("kra,kr->ka", Ja, r)); np.add.at(self.g, et, np.einsum("kra,kr->ka", Jb, r))
        d = np.arange(D)
        for k in range(len(pv)):                    # J~ = sc [I; 0] (scaled columns: sc s)
            c = psc[k] * s[pv[k]]
            self.Hd[pv[k], d, d] += c * c
            self.g[pv[k]] += c * pr[k, :D]
        self.Hd[:, d, d] += T(lam)
        self.cost = T(0.5) * (np.sum(r * r) + np.sum(pr * pr))
        # term counts and magnitudes
        li = live.astype(np.int64)
        self.P_d = np.zeros(n_v, dtype=np.int64)
        np.add.at(self.P_d, ef, li); np.add.at(self.P_d, et, li); np.add.at(self.P_d, ef[loop], 2 * li[loop]); np.add.at(self.P_d, pv, 1)
        self.P_g = np.zeros(n_v, dtype=np.int64)
        np.add.at(self.P_g, ef, li); np.add.at(self.P_g, et, li); np.add.at(self.P_g, pv, 1)
        self.M_d = np.zeros(n_v); self.M_g = np.zeros(n_v)
        np.add.at(self.M_d, ef, mags["haa"]); np.add.at(self.M_d, et, mags["hbb"]); np.add.at(self.M_d, ef[loop], 2.0 * mags["hab"][loop])
        psc64 = np.abs(np.asarray(psc, dtype=np.float64))
        np.add.at(self.M_d, pv, (psc64 * smax[pv]) ** 2)
        np.add.at(self.M_g, ef, mags["ga"]); np.add.at(self.M_g, et, mags["gb"])
        np.add.at(self.M_g, pv, psc64 * smax[pv] * _vn(np.asarray(pr, dtype=np.float64)[:, :D]) if len(pv) else np.zeros(0))
        self.touched = self.P_d > 0                 # (before lambda is counted: a vertex with no live term is exactly lambda I)
        self.M_d += abs(lam); self.P_d = self.P_d + 1
        self.P_o = np.zeros(len(key), dtype=np.int64); self.M_o = np.zeros(len(key))
        np.add.at(self.P_o, inv, li[x]); np.add.at(self.M_o, inv, mags["hab"][x])
        self.n_terms = int(live.sum()) + len(pv)
        self.M_cost = float(np.sum(np.asarray(r, dtype=np.float64) ** 2) + np.sum(np.asarray(pr, dtype=np.float64) ** 2))

    def column_norms_sq(self):
        """diag of H without lambda: the squared column norms of J~"""
        d = np.arange(self.D)
        return self.Hd[:, d, d] - self.T(self.lam)

    def jv_gram(self, a, b):
        """a, b (n_v, D) in the caller's vertex order -> ((u.u, u.w, w.w) in dtype, their magnitudes)"""
        T = self.T
        a = np.asarray(a, dtype=T); b = np.asarray(b, dtype=T)
        u = np.einsum("kra,ka->kr", self.Ja, a[self.ef]) + np.einsum("kra,ka->kr", self.Jb, a[self.et])
        w = np.einsum("kra,ka->kr", self.Ja, b[self.ef]) + np.einsum("kra,ka->kr", self.Jb, b[self.et])
        s2 = self.psc * self.psc
        av, bv = a[self.pv], b[self.pv]
        out = np.array([np.sum(u * u) + np.sum(s2 * np.sum(av * av, axis=1)), np.sum(u * w) + np.sum(s2 * np.sum(av * bv, axis=1)),
                        np.sum(w * w) + np.sum(s2 * np.sum(bv * bv, axis=1))], dtype=T)
        m = self.mags
        na, nb = _vn(a), _vn(b)
        mu = m["f"] * (m["ja"] * na[self.ef] + m["jb"] * na[self.et]); mw = m["f"] * (m["ja"] * nb[self.ef] + m["jb"] * nb[self.et])
        p2 = np.asarray(s2, dtype=np.float64)
        mag = np.array([np.sum(mu * mu) + np.sum(p2 * na[self.pv] ** 2), np.sum(mu * mw) + np.sum(p2 * na[self.pv] * nb[self.pv]),
                        np.sum(mw * mw) + np.sum(p2 * nb[self.pv] ** 2)])
        return out, mag


def matvec(ref, x):
    """H x for x (n_v, D) in the caller's vertex order, block by block in ref's dtype"""
    x = np.asarray(x, dtype=ref.T)
    y = np.einsum("vab,vb->va", ref.Hd, x)
    hi, lo = ref.pairs[:, 0], ref.pairs[:, 1]
    np.add.at(y, hi, np.einsum("pab,pb->pa", ref.Ho, x[lo]))
    np.add.at(y, lo, np.einsum("pab,pa->pb", ref.Ho, x[hi]))
    return y


def pair(D, n_v, e_from, e_to, J, r, lam, priors=None, mags=None, scaling=None):
    """(long double reference, fp64 restatement) of one linearisation."""
    return (PgAsmRef(D, n_v, e_from, e_to, J, r, lam, priors, mags, scaling, LD),
            PgAsmRef(D, n_v, e_from, e_to, J, r, lam, priors, mags, scaling, np.float64))


# ---- dense exports <-> blocks -------------------------------------------------------------------------------------------------
def blocks_of(H, pose_col, D):
    """Dense H in the caller's global column order -> (n_v, n_v, D, D) in the caller's vertex order (a copy)."""
    cols = (np.asarray(pose_col, dtype=np.int64)[:, None] + np.arange(D)[None]).ravel()
    n_v = len(pose_col)
    return np.ascontiguousarray(H[np.ix_(cols, cols)].reshape(n_v, D, n_v, D).transpose(0, 2, 1, 3))


def rows_of(g, pose_col, D):
    return np.asarray(g)[np.asarray(pose_col, dtype=np.int64)[:, None] + np.arange(D)[None]]


def to_columns(x, pose_col, D):
    """(n_v, D) in vertex order -> a vector in the global column order"""
    out = np.zeros(x.size, dtype=x.dtype)
    out[np.asarray(pose_col, dtype=np.int64)[:, None] + np.arange(D)[None]] = x
    return out


# ---- the rule -----------------------------------------------------------------------------------------------------------------
def _ratio(err, bound):
    err = np.asarray(err, dtype=np.float64); bound = np.asarray(bound, dtype=np.float64)
    out = np.zeros_like(err)
    nz = bound > 0
    out[nz] = err[nz] / bound[nz]
    out[~nz & (err > 0)] = np.inf
    return out


def _dist(a, b):
    a = np.asarray(a, dtype=LD); b = np.asarray(b, dtype=LD)
    return np.abs(a - b).reshape(len(a), -1).max(axis=1).astype(np.float64) if len(a) else np.zeros(0)


def h_check(H4, ld, f64, C0, use_referee=True):
    """H4 (n_v, n_v, D, D) against the reference.  -> (ratios {diag, lower, upper}, bad [(kind, vr, vc), ...] worst first,
    stray: the number of non-zero entries in blocks of pairs without an edge).  Lower and upper blocks are read separately."""
    n_v = ld.n_v
    d = np.arange(n_v)
    hi, lo = ld.pairs[:, 0], ld.pairs[:, 1]
    ref = lambda on: 8.0 * on if use_referee else 0.0 * on
    b_d = np.maximum(ref(_dist(f64.Hd, ld.Hd)), gamma(ld.P_d, C0) * ld.M_d); b_d[~ld.touched] = 0.0
    b_o = np.maximum(ref(_dist(f64.Ho, ld.Ho)), gamma(ld.P_o, C0) * ld.M_o); b_o[ld.P_o == 0] = 0.0
    ratios = dict(diag=_ratio(_dist(H4[d, d], ld.Hd), b_d), lower=_ratio(_dist(H4[hi, lo], ld.Ho), b_o),
                  upper=_ratio(_dist(H4[lo, hi].transpose(0, 2, 1), ld.Ho), b_o))
    bad = [("diag", int(v), int(v), float(ratios["diag"][v])) for v in np.nonzero(ratios["diag"] > 1.0)[0]]
    for kind in ("lower", "upper"):
        bad += [(kind, int(hi[k]), int(lo[k]), float(ratios[kind][k])) for k in np.nonzero(ratios[kind] > 1.0)[0]]
    bad.sort(key=lambda t: -t[3])
    rest = H4 != 0.0
    rest[d, d] = False; rest[hi, lo] = False; rest[lo, hi] = False
    return ratios, [t[:3] for t in bad], int(rest.sum())


def g_check(g_rows, ld, f64, C0, use_referee=True):
    e_np = _dist(f64.g, ld.g) if use_referee else 0.0
    return _ratio(_dist(g_rows, ld.g), np.maximum(8.0 * e_np, gamma(ld.P_g, C0) * ld.M_g))


def scalar_check(dev, ref_ld, ref_64, mag, terms, C0, use_referee=True):
    dev = np.atleast_1d(np.asarray(dev, dtype=LD)); ref_ld = np.atleast_1d(np.asarray(ref_ld, dtype=LD))
    e_np = np.abs(np.atleast_1d(np.asarray(ref_64, dtype=LD)) - ref_ld).astype(np.float64) if use_referee else 0.0
    return _ratio(np.abs(dev - ref_ld).astype(np.float64), np.maximum(8.0 * e_np, gamma(terms, C0) * np.atleast_1d(np.asarray(mag, dtype=np.float64))))


def norms_check(norms_rows, ld, f64, C0, use_referee=True):
    """compute_column_norms (n_v, D) against sqrt(diag J~^T J~): compared as squares, two more roundings (the root, the square)"""
    n2 = np.asarray(norms_rows, dtype=LD) ** 2
    e_np = _dist(f64.column_norms_sq(), ld.column_norms_sq()) if use_referee else 0.0
    return _ratio(_dist(n2, ld.column_norms_sq()), np.maximum(8.0 * e_np, gamma(ld.P_d + 2, C0) * ld.M_d))


def worst(ratio):
    ratio = np.asarray(ratio)
    if ratio.size == 0:
        return 0.0, ()
    k = np.unravel_index(int(np.argmax(ratio)), ratio.shape)
    return float(ratio[k]), tuple(int(x) for x in k)


def report(label, ratios):
    """One PGASM line: the worst ratio of every checked quantity and where it sits."""
    parts = []
    for name, r in ratios.items():
        v, at = worst(r)
        parts.append(f"{name} {v:.3g}@{','.join(str(a) for a in at)}")
    print(f"PGASM {label}: " + "  ".join(parts))


# ---- the kernels' placement, restated on the host (for the mutation tests) ----------------------------------------------------
MUTATIONS = ("cross_transposed", "loop_without_transpose", "owner_smaller", "vpt_off_by_one", "prior_run_cut", "stale_gradient")


def emulate_export(ref, mutation=None, vmap=None, stale=1.0):
    """What get_hessian would return -- (H4 (n_v, n_v, D, D), g (n_v, D)) in the caller's vertex order -- had the kernels placed
    the products of the fp64 restatement `ref` the way pg_kernels.hip does: internal vertex vmap[v], block address tile
    (vr / vpt, vc / vpt), row (vr % vpt) D, column (vc % vpt) D of a lower-triangular tile matrix, the export mirroring the
    lower triangle.  mutation: one of MUTATIONS damages that placement; None reproduces ref exactly up to summation order."""
    assert mutation is None or mutation in MUTATIONS
    D, n_v = ref.D, ref.n_v
    vpt = NB // D
    vm = np.arange(n_v) if vmap is None else np.asarray(vmap, dtype=np.int64)
    vk = vpt - 1 if mutation == "vpt_off_by_one" else vpt
    pos = lambda v: (v // vk) * NB + (v % vk) * D                     # h_block_ptr's row / column of an internal vertex
    n_pad = ((n_v * D + NB - 1) // NB) * NB
    size = int(pos(np.int64(vm.max())) + D) if n_v else 0
    size = max(size, n_pad)
    Tm = np.zeros((size, size))

    def add(vr, vc, B, lower_only=False):
        r0, c0_ = int(pos(vr)), int(pos(vc))
        Tm[r0:r0 + D, c0_:c0_ + D] += np.tril(B) if lower_only else B

    Ja, Jb = np.asarray(ref.Ja, dtype=np.float64), np.asarray(ref.Jb, dtype=np.float64)
    live = ref.mags["live"]
    g = np.zeros((n_v, D))
    if mutation == "stale_gradient":
        g[~(ref.P_g > 0)] = stale                                     # a row nobody stores into keeps what the buffer held
    rr = np.asarray(ref.r, dtype=np.float64)
    for e in range(len(ref.ef)):
        if not live[e]:
            continue
        a, b = int(vm[ref.ef[e]]), int(vm[ref.et[e]])
        add(a, a, Ja[e].T @ Ja[e], True); add(b, b, Jb[e].T @ Jb[e], True)
        Hab = Ja[e].T @ Jb[e]
        if a == b:
            add(a, a, Hab if mutation == "loop_without_transpose" else Hab + Hab.T, True)
        else:
            hi, lo, B = (a, b, Hab) if a > b else (b, a, Hab.T)
            if mutation == "cross_transposed":
                B = B.T
            if mutation == "owner_smaller":
                add(lo, hi, B.T)                                      # (lands above the diagonal: the export never reads it)
            else:
                add(hi, lo, B)
        g[ref.ef[e]] += Ja[e].T @ rr[e]; g[ref.et[e]] += Jb[e].T @ rr[e]
    # priors: SE2's run rule on the blocks sorted by internal vertex (k_pg2_priors); a cut run loses what follows the boundary
    order = np.argsort(vm[ref.pv], kind="stable") if len(ref.pv) else np.zeros(0, dtype=np.int64)
    sv = vm[ref.pv][order] if len(order) else order
    psc, pr = np.asarray(ref.psc, dtype=np.float64), np.asarray(ref.pr, dtype=np.float64)
    for k in range(len(order)):
        if k > 0 and sv[k - 1] == sv[k]:
            continue
        j = k
        while j < len(order) and sv[j] == sv[k] and not (mutation == "prior_run_cut" and j // 64 != k // 64):
            src = order[j]
            add(int(sv[k]), int(sv[k]), psc[src] ** 2 * np.eye(D), True)
            g[ref.pv[src]] += psc[src] * pr[src, :D]
            j += 1
    lam_rows = np.arange(n_v * D)
    Tm[lam_rows, lam_rows] += ref.lam
    # the export: the lower triangle of the n_pad x n_pad tile matrix at the TRUE addresses, mirrored
    Tm = Tm[:n_pad, :n_pad]
    Hs = np.tril(Tm) + np.tril(Tm, -1).T
    cols = (vm[:, None] * D + np.arange(D)[None]).ravel()
    H4 = Hs[np.ix_(cols, cols)].reshape(n_v, D, n_v, D).transpose(0, 2, 1, 3)
    return np.ascontiguousarray(H4), g
