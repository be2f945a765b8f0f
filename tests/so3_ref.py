"""Long-double reference of the SO3 pose-graph math (rotation averaging) -- TEST INFRASTRUCTURE ONLY (CPU;
tests/test_so3_ref_host.py holds it against itself, the host and GPU tests hold the device code against it).

Built on the cancellation-free pieces of tests/manifold_ref.py (so3_log, so3_left_jacobian_inv, _qmul and the compensated
products), with the branches where the reference solver has them (file:line under the apex-solver tree):
  SO3::from(DVector) / coeffs()      crates/apex-manifolds/src/so3.rs:225-229, 210-213   [qw, qx, qy, qz], normalised (twice,
                                     as the project normalises an SE3 pose's quaternion)
  log / exp                          so3.rs:313-357, 558-577          sin^2 | theta^2 against 1e-10 (lib.rs:61)
  right_jacobian_inv = Jl^-1 ^T      so3.rs:618-644
  between, right plus                lib.rs:401-419, 269-283
  BetweenFactor<SO3>::linearize      src/factors/between_factor.rs:268-322
      r = Log((k1^-1 k0) m),  J0 = Jr^-1(r) Adj(m^-1),  J1 = Jr^-1(r) (Adj(m^-1) (-Adj((k1^-1 k0)^-1))),  Adj(R) = R
  PriorFactor                        src/factors/prior_factor.rs:96-108, src/linearizer/cpu/sparse.rs:201-204
      r = coeffs(x) - data (4 rows), the 4 x 4 identity truncated to the three tangent columns

Everything is batched: quaternions (n, 4), tangents (n, 3).  Inputs are fp64 (taken exactly), outputs long double.
So3Problem is the dense problem (H, g, cost, steps, the optimiser loops' interface of np_ref_trust_region) under any loss of
np_ref_loss and optional information matrices, with the block-by-block assembly of pg_asm_ref (PgAsmRef, D = 3)."""
from __future__ import annotations

from dataclasses import dataclass

import numpy as np

import manifold_ref as mr
import np_ref_info as ni
import np_ref_loss as nl
import np_ref_se2
import pg_asm_ref as par
from manifold_ref import LD, SMALL2, _dot, _eye, _ld, _mm, _q_to_R, _qconj, _qmul, sinc, so3_left_jacobian_inv, so3_log


def so3_from_vec(q):
    """SO3::from(DVector): the quaternion normalised twice (manifold_ref.se3_from_vec on its rotational part)"""
    q = _ld(np.atleast_2d(q))
    for _ in range(2):
        q = q / np.sqrt(_dot(q, q))[:, None]
    return q


def so3_right_jacobian_inv(th):
    return np.swapaxes(so3_left_jacobian_inv(th), -1, -2)


def so3_between(k0, k1, meas):
    """r (n, 3), J (n, 3, 6) = [dr/dk0 | dr/dk1] of r = Log((k1^-1 k0) meas), uncorrected"""
    q0, q1, qm = so3_from_vec(k0), so3_from_vec(k1), so3_from_vec(meas)
    qA = _qmul(_qconj(q1), q0)
    qD = _qmul(qA, qm)
    r = so3_log(qD)
    Jr = so3_right_jacobian_inv(r)
    Rm_t = np.swapaxes(_q_to_R(qm), -1, -2)          # Adj(m^-1)
    J0 = _mm(Jr, Rm_t)
    # Adj(m^-1) (-Adj(A^-1)) = -Adj((A m)^-1) = -R(D)^T: the same matrix in exact arithmetic, one product fewer
    J1 = -_mm(Jr, np.swapaxes(_q_to_R(qD), -1, -2))
    return r, np.concatenate([J0, J1], -1)


def so3_exp(th):
    th = _ld(np.atleast_2d(th))
    a = (th * th).sum(-1)
    big = a > SMALL2
    n = np.sqrt(np.where(big, a, LD(1))) / 2
    q_big = np.concatenate([np.cos(n)[:, None], (th / 2) * sinc(n)[:, None]], -1)
    qs = np.concatenate([np.ones((len(th), 1), dtype=LD), th / 2], -1)
    q_small = qs / np.sqrt((qs * qs).sum(-1))[:, None]
    return np.where(big[:, None], q_big, q_small)


def so3_plus(q, d):
    """q (+) d = q * Exp(d) on the stored (un-normalised) quaternion, stored un-normalised; q (+) 0 = q"""
    qq, dd = _ld(np.atleast_2d(q)), _ld(np.atleast_2d(d))
    out = _qmul(qq, so3_exp(dd))
    return np.where(np.all(dd == 0, axis=-1)[:, None], qq, out)


def so3_prior(x, data, delta):
    """corrected r (n, 4) and sqrt(rho') (n,) of PriorFactor blocks: r = coeffs(from(x)) - data under Huber(delta) | None"""
    r = so3_from_vec(x) - _ld(np.atleast_2d(data))
    s = (r * r).sum(-1)
    sc = np.array([mr.huber_scale(dl, s[k:k + 1])[0] for k, dl in enumerate(np.broadcast_to(np.asarray(delta, dtype=object), (len(r),)))], dtype=LD)
    return r * sc[:, None], sc


def f64(x):
    return np.asarray(x).astype(np.float64)


@dataclass
class So3Problem(np_ref_se2.Problem):
    """np_ref_se2.Problem's interface (edge_blocks, prior_blocks, cost, jacobian, normal_equations, solve, apply_step,
    parameter_norm, lm_optimize; np_ref_trust_region's loops take it) on SO3 vertices.  The per-edge math is evaluated in long
    double and rounded once to fp64; the loss goes through np_ref_loss.correct_edges and information matrices through
    np_ref_info.whiten, as for the other manifolds."""
    loss: object = None
    information: np.ndarray | None = None

    def __post_init__(self):
        self.poses = np.array(self.poses, dtype=np.float64)
        self.e_from = np.asarray(self.e_from, dtype=np.int64); self.e_to = np.asarray(self.e_to, dtype=np.int64)
        self.n_v = self.poses.shape[0]; self.n = 3 * self.n_v
        if self.loss is None:
            self.loss = ni.NO_LOSS

    @classmethod
    def from_problem(cls, prob, poses=None):
        d = prob.data
        return cls(d.poses if poses is None else poses, d.e_from, d.e_to, d.meas, prob.pose_col, prob.fix, None, list(prob.priors),
                   loss=ni.loss_of(prob), information=prob.information)

    def raw_blocks(self, dtype=np.float64):
        if not len(self.e_from):
            return np.zeros((0, 3), dtype), np.zeros((0, 3, 6), dtype)
        r, J = so3_between(self.poses[self.e_from], self.poses[self.e_to], self.meas)
        return r.astype(dtype), J.astype(dtype)

    def edge_blocks(self):
        r, J = self.raw_blocks()
        if self.information is not None:
            r, J = ni.whiten(r, J, self.information)
        r, J, self.arms, self.s = nl.correct_edges(r, J, self.loss)
        return r, J

    def prior_blocks(self):
        if not self.priors:
            return np.zeros((0, 4)), np.zeros(0)
        v = [p[0] for p in self.priors]
        r, sc = so3_prior(self.poses[v], np.array([p[1] for p in self.priors]), [p[2] for p in self.priors])
        return f64(r), f64(sc)

    def jacobian(self):
        """dense corrected (r, J) in residual-block order: edges (3 rows each), then priors (4 rows over 3 columns)"""
        r, Jb = self.edge_blocks()
        pr, psc = self.prior_blocks()
        ne, npri = r.shape[0], pr.shape[0]
        J = np.zeros((3 * ne + 4 * npri, self.n))
        C = self.cols()
        for e in range(ne):
            J[3 * e:3 * e + 3, C[self.e_from[e]]] += Jb[e, :, :3]
            J[3 * e:3 * e + 3, C[self.e_to[e]]] += Jb[e, :, 3:]
        for k, (v, _, _) in enumerate(self.priors):
            J[3 * ne + 4 * k + np.arange(3), C[v]] += psc[k]
        return np.concatenate([r.ravel(), pr.ravel()]), J

    def apply_step(self, step, sign=1.0):
        d = sign * step[self.cols()]
        d = np.where(self.fix.astype(bool), 0.0, d)
        self.poses = f64(so3_plus(self.poses, d))

    def blocks(self, lam=0.0):
        """(long double, fp64) PgAsmRef pair of the corrected blocks at the current point: H and g block by block"""
        r, J = self.edge_blocks()
        pri = None
        if self.priors:
            pr, psc = self.prior_blocks()
            pri = (np.array([p[0] for p in self.priors], dtype=np.int64), pr, psc)
        return par.pair(3, self.n_v, self.e_from, self.e_to, J, r, lam, priors=pri)

    def dense(self, lam=0.0):
        """H + lam I (n, n), g (n,), cost in long double, in the global column order, from the blocks"""
        ld, _ = self.blocks(lam)
        C = self.cols()
        H = np.zeros((self.n, self.n), dtype=LD)
        for v in range(self.n_v):
            H[np.ix_(C[v], C[v])] = ld.Hd[v]
        for k, (hi, lo) in enumerate(ld.pairs):
            H[np.ix_(C[hi], C[lo])] = ld.Ho[k]; H[np.ix_(C[lo], C[hi])] = ld.Ho[k].T
        g = np.zeros(self.n, dtype=LD)
        g[C] = ld.g
        return H, g, ld.cost


# ---- the block rule of pg_asm_ref for SO3 ---------------------------------------------------------------------------------
# pg_asm_ref.c0 counts the roundings of one term as 2 LIN + PROD with LIN the longest dependent chain of the linearisation; its
# table has SE2's 30.  The SO3 chain (pg_so3_device.hpp, between_so3_linearize), counted the way that file counts SE3's: two
# quaternion products 8 each (what it allows an se3_mul, which contains one), so3_log 7, so3_left_jacobian_inv 12 (both as
# counted there for SE3's rotational block), the transpose 0, quat_to_rot 4 (a square, three sums), two 3 x 3 products 6:
LIN_SO3 = 8 + 8 + 7 + 12 + 4 + 6          # 45


def c0(policy, scaled=False):
    """pg_asm_ref.c0 for D = 3 with SO3's linearisation chain in place of SE2's; PROD is manifold-free"""
    return par.c0(3, policy, scaled) + 2 * (LIN_SO3 - par.LIN[3])


def kernel_policy(P):
    """the instantiation a problem runs under: LossLegacy | LossGeneral | LossWeighted (pg_kernels.hip, with_loss)"""
    from apex_solver_amd import capi
    if P.information is not None:
        return "weighted"
    return "legacy" if P.loss.kind in (capi.LOSS_NONE, capi.LOSS_L2, capi.LOSS_HUBER) else "general"


def asm_reference(P, J, r, lam, prior_residuals=None):
    """(long double, fp64) PgAsmRef pair built from the blocks a handle EXPORTED (J, r corrected, whitened under information):
    the linearisation is not on trial, where the kernels put the products is.  The magnitudes of the terms come from this
    file's uncorrected blocks and np_ref_loss's corrector, as pg_asm_cases.magnitudes takes them for SE2."""
    kernel = kernel_policy(P)
    mags = None
    if kernel != "legacy":
        r0, J0 = P.raw_blocks()
        P.edge_blocks()                                   # (sets P.s: the squared norms the corrector saw)
        corr = np.array([[float(x) for x in nl.corrector(P.loss, s)[:3]] + [s] for s in P.s]).reshape(-1, 4).T
        mags = par.edge_magnitudes(3, J, r, raw=(r0, J0), corr=corr, info=P.information)
        # pg_asm_ref counts the corrector's scalars as ten roundings of a well-conditioned evaluation.  rho'(s) is not one near
        # a loss's cut-off (Tukey: rho' = (1 - s/c^2)^2 / 2 -> 0): the export kernel and the assembly kernel each rebuild s from
        # their own linearisation, and a relative difference eps in s moves rho' by kappa eps, kappa = |s rho''(s) / rho'(s)|,
        # the condition number of rho' -- and with it every term of that edge, which is proportional to rho' (sqrt(rho') in J~).
        # So an edge's magnitudes carry max(1, kappa): 1 wherever the rule of pg_asm_ref applies as it stands (kappa < 1 for
        # Cauchy at every s), kappa only on edges whose weight itself is ill-conditioned.  From the loss alone; nothing fitted.
        kap = np.ones(len(P.s))
        for e, sq in enumerate(P.s):
            rho = nl.evaluate(P.loss, sq)
            if float(rho[1]) > 0.0:
                kap[e] = max(1.0, abs(float(sq) * float(rho[2]) / float(rho[1])))
        mags = dict(mags)
        for k in ("haa", "hbb", "hab", "ga", "gb"):
            mags[k] = mags[k] * kap
        mags["f"] = mags["f"] * np.sqrt(kap)
        mags["kappa"] = kap
    pri = None
    if P.priors:
        pr_np, psc = P.prior_blocks()
        pri = (np.array([q[0] for q in P.priors], dtype=np.int64), pr_np if prior_residuals is None else prior_residuals, psc)
    return par.pair(3, P.n_v, P.e_from, P.e_to, J, r, lam, priors=pri, mags=mags)


def solve_ld(H, g, lam=0.0):
    """(H + lam I) x = -g by a long-double Cholesky (np_ref_info.solve_damped_ld)"""
    return ni.solve_damped_ld(np.asarray(H), np.asarray(g), lam)


# ---- crafted graphs shared by the host and device assembly tests ---------------------------------------------------------
VPT = 48


def random_rotations(rng, n, spread=None):
    """(n, 4) unit quaternions: uniform on SO3, or within about `spread` radians of the identity"""
    if spread is None:
        q = rng.standard_normal((n, 4))
    else:
        q = np.column_stack([np.ones(n), 0.5 * spread * rng.standard_normal((n, 3))])
    return q / np.linalg.norm(q, axis=1, keepdims=True)


def crafted(name, seed=0):
    """PoseGraphData of a crafted graph: 'loop' (a self-loop on a chain vertex and on a lonely one), 'multi' (2 and 64 parallel
    edges, in both directions, across a tile boundary), 'isolated' (vertices without an edge, one the last), 'hub' (a vertex of
    degree 70 that owns none | all of its blocks: 'hub_lo' | 'hub_hi'), 'cross' (edges whose endpoints lie in different tiles,
    in both directions), 'nv47' .. 'nv97' (a chain plus chords on that many vertices), 'ne255' .. 'ne257' (that many edges)."""
    from apex_solver_amd.synthetic import PoseGraphData

    rng = np.random.default_rng(seed + sum(map(ord, name)))
    chain = lambda n: [(i, i + 1) for i in range(n - 1)]
    if name == "loop":
        n_v = 8
        edges = [(a, b) for a, b in chain(8) if 5 not in (a, b)] + [(4, 6), (2, 2), (5, 5), (2, 2)]
    elif name == "multi":
        n_v = VPT + 6
        edges = chain(n_v) + [(3, VPT + 1), (VPT + 1, 3)] + [((5, VPT + 2) if j % 3 else (VPT + 2, 5)) for j in range(64)]
    elif name == "isolated":
        n_v = 10
        keep = [v for v in range(n_v) if v not in (3, 9)]
        edges = list(zip(keep[:-1], keep[1:])) + [(0, 5)]
    elif name in ("hub_lo", "hub_hi"):
        n_v = 71
        hub = 0 if name == "hub_lo" else 70
        edges = [((hub, v) if v % 3 else (v, hub)) for v in range(n_v) if v != hub]
    elif name == "cross":
        n_v = 2 * VPT + 1
        edges = chain(n_v) + [(VPT - 1, 2 * VPT), (2 * VPT, 0), (1, VPT + 1), (VPT + 3, 2)]
    elif name.startswith("nv"):
        n_v = int(name[2:])
        edges = chain(n_v) + [tuple(int(x) for x in rng.choice(n_v, 2, replace=False)) for _ in range(n_v // 2)]
    elif name.startswith("ne"):
        n_e = int(name[2:]); n_v = 100
        edges = chain(n_v)
        while len(edges) < n_e:
            edges.append(tuple(int(x) for x in rng.choice(n_v, 2, replace=False)))
    else:
        raise KeyError(name)
    ef = np.array([e[0] for e in edges], dtype=np.uint32); et = np.array([e[1] for e in edges], dtype=np.uint32)
    poses = random_rotations(rng, n_v, 0.8)
    meas = random_rotations(rng, len(ef), 0.8)
    out = np.arange(len(ef)) % 7 == 3                      # gross outliers: a turn of about 2.5 rad
    big = rng.standard_normal((len(ef), 3)); big = 2.5 * big / np.linalg.norm(big, axis=1, keepdims=True)
    meas[out] = f64(so3_plus(meas[out], big[out]))
    return PoseGraphData(ids=np.arange(n_v, dtype=np.int64), poses=poses, e_from=ef, e_to=et, meas=meas, name=name)


def random_information(n_e, seed=11):
    """random symmetric positive-definite 3 x 3 matrices with eigenvalues in [0.2, 20]"""
    rng = np.random.default_rng(seed)
    out = np.zeros((n_e, 3, 3))
    for e in range(n_e):
        Q, R = np.linalg.qr(rng.standard_normal((3, 3)))
        Q = Q * np.sign(np.diag(R))[None, :]
        W = (Q * np.exp(rng.uniform(np.log(0.2), np.log(20.0), 3))[None, :]) @ Q.T
        out[e] = 0.5 * (W + W.T)
    return out
