"""CPU reference for SE2 pose graphs, in numpy: a restatement of the reference solver's SE2 math and LM loop that shares no
code with apex-solver_amd/csrc/pg2_device.hpp (group elements are 3 x 3 homogeneous matrices here, not translation + unit
complex; the between-factor Jacobians come from adjoints of those matrices; everything is batched over edges).

Reference semantics (file:line under the apex-solver tree):
  SE2, vector form [x, y, theta]                crates/apex-manifolds/src/se2.rs:27-63
  inverse / compose / log / adjoint / exp       se2.rs:213-328, 468-494
  right_jacobian, right_jacobian_inv            se2.rs:497-534, 577-613   (small-angle: theta^2 vs 1e-10, lib.rs:61)
  BetweenFactor<SE2>::linearize                 src/factors/between_factor.rs:268-322
  PriorFactor                                   src/factors/prior_factor.rs:96-108
  HuberLoss + corrector                         src/core/loss_functions.rs:364-380, corrector.rs:143-181
  LM loop                                       src/optimizer/levenberg_marquardt.rs:823-1031 (in the form
                                                oracle/pg_oracle.c restates it for SE3: same config fields, same
                                                accept / reject and damping rule)
"""
from __future__ import annotations

from dataclasses import dataclass, field

import numpy as np

SMALL2 = 1e-10
# The closed forms of (1 - cos t) / t and of Jr^-1 subtract nearly equal numbers just above the small-angle threshold
# (|t| = 1e-5).  They are evaluated here in extended precision (numpy longdouble, 64-bit mantissa on x86), Jr^-1 in a
# regrouped form (see right_jacobian_inv), then rounded to fp64 -- the reference's FUNCTIONS to roundoff, not the last
# bits of one libm.
#
# This rests on np.longdouble being the x86 80-bit type (np.finfo(np.longdouble).nmant == 63).  Where long double is
# fp64 the module still runs, but the extended-precision claim is void and tests/golden/se2_manhattan_40.npz will not
# reproduce to 1e-14.  The regrouping of Jr^-1 (y/2 + x k) is the same algebraic step pg2_device.hpp takes -- the two
# differ in how k is evaluated (cot in extended precision here, a series there); the central-difference test of
# tests/test_se2_np_ref.py pins that step from outside.
LD = np.longdouble


def _cos(x):
    """cos / sin / atan2 through libm's long-double routines, rounded to fp64: the same bits on every x86 CPU (numpy's fp64
    loops pick SIMD kernels by CPU, which may differ in the last bit -- enough to move a 1e-14 golden)."""
    return np.cos(np.asarray(x, dtype=np.float64).astype(LD)).astype(np.float64)


def _sin(x):
    return np.sin(np.asarray(x, dtype=np.float64).astype(LD)).astype(np.float64)


def _atan2(y, x):
    return np.arctan2(np.asarray(y, dtype=np.float64).astype(LD), np.asarray(x, dtype=np.float64).astype(LD)).astype(np.float64)


# ---- group elements as homogeneous matrices (..., 3, 3) --------------------------------------------------------------
def wrap(th):
    """theta as SE2 -> DVector gives it: atan2(sin, cos); values in (-pi, pi] are their own image."""
    th = np.asarray(th, dtype=np.float64)
    inside = (th > -np.pi) & (th <= np.pi)
    return np.where(inside, th, _atan2(_sin(th), _cos(th)))


def mat(v):
    """[x, y, theta] -> T = [[c, -s, x], [s, c, y], [0, 0, 1]]"""
    v = np.asarray(v, dtype=np.float64)
    c, s = _cos(v[..., 2]), _sin(v[..., 2])
    T = np.zeros(v.shape[:-1] + (3, 3))
    T[..., 0, 0] = c; T[..., 0, 1] = -s; T[..., 0, 2] = v[..., 0]
    T[..., 1, 0] = s; T[..., 1, 1] = c; T[..., 1, 2] = v[..., 1]
    T[..., 2, 2] = 1.0
    return T


def vec(T):
    return np.stack([T[..., 0, 2], T[..., 1, 2], _atan2(T[..., 1, 0], T[..., 0, 0])], axis=-1)


def inv(T):
    R = T[..., :2, :2]
    Ti = np.zeros_like(T)
    Rt = np.swapaxes(R, -1, -2)
    Ti[..., :2, :2] = Rt
    Ti[..., :2, 2] = -np.einsum("...ij,...j->...i", Rt, T[..., :2, 2])
    Ti[..., 2, 2] = 1.0
    return Ti


def adjoint(T):
    A = np.zeros_like(T)
    A[..., :2, :2] = T[..., :2, :2]
    A[..., 0, 2] = T[..., 1, 2]
    A[..., 1, 2] = -T[..., 0, 2]
    A[..., 2, 2] = 1.0
    return A


def _ab(th):
    th = np.asarray(th, dtype=np.float64)
    t2 = th * th
    small = t2 < SMALL2
    t = np.where(small, 1.0, th).astype(LD)
    a = np.where(small, 1.0 - t2 / 6.0, (np.sin(t) / t).astype(np.float64))
    b = np.where(small, 0.5 * th - th * t2 / 24.0, ((1 - np.cos(t)) / t).astype(np.float64))
    return a, b


def exp(tau):
    tau = np.asarray(tau, dtype=np.float64)
    th = tau[..., 2]
    a, b = _ab(th)
    return mat(np.stack([a * tau[..., 0] - b * tau[..., 1], b * tau[..., 0] + a * tau[..., 1], th], axis=-1))


def log(T):
    v = vec(T)
    th = v[..., 2]
    a, b = _ab(th)
    den = a * a + b * b
    return np.stack([(a * v[..., 0] + b * v[..., 1]) / den, (-b * v[..., 0] + a * v[..., 1]) / den, th], axis=-1)


def right_jacobian(tau):
    tau = np.asarray(tau, dtype=np.float64)
    x, y, th = tau[..., 0], tau[..., 1], tau[..., 2]
    a, b = _ab(th)
    t2 = th * th
    small = t2 < SMALL2
    t2s = np.where(small, 1.0, t2)
    c, s = _cos(th), _sin(th)
    J = np.zeros(tau.shape[:-1] + (3, 3))
    J[..., 0, 0] = a; J[..., 0, 1] = b; J[..., 1, 0] = -b; J[..., 1, 1] = a; J[..., 2, 2] = 1.0
    J[..., 0, 2] = np.where(small, -y / 2 + th * x / 6, (-y + th * x + y * c - x * s) / t2s)
    J[..., 1, 2] = np.where(small, x / 2 + th * y / 6, (x + th * y - x * c - y * s) / t2s)
    return J


def right_jacobian_inv(tau):
    tau = np.asarray(tau, dtype=np.float64)
    x, y, th = tau[..., 0], tau[..., 1], tau[..., 2]
    t2 = th * th
    big = t2 > SMALL2
    u = (np.where(big, th, 1.0).astype(LD)) / 2
    J = np.zeros(tau.shape[:-1] + (3, 3))
    J[..., 0, 1] = -th / 2; J[..., 1, 0] = th / 2; J[..., 2, 2] = 1.0
    # se2.rs:588-603 regrouped (t sin t / (2 - 2 cos t) = (t/2) cot(t/2); the (0,2) and (1,2) entries are y/2 + x k and
    # -x/2 + y k with k = (1 - (t/2) cot(t/2)) / t): the literal quotients have numerators of order t^3 made of terms of
    # order 1, i.e. an fp64 error of 1e-16 / t^3 -- a percent just above the threshold.  In extended precision the
    # regrouped form is good to 1e-19 / t.
    d_ld = u * np.cos(u) / np.sin(u)
    k = ((1 - d_ld) / (2 * u)).astype(np.float64)
    d = np.where(big, d_ld.astype(np.float64), 1.0 - t2 / 12)
    J[..., 0, 0] = d; J[..., 1, 1] = d
    J[..., 0, 2] = np.where(big, y / 2 + x * k, y / 2 + th * x / 12)
    J[..., 1, 2] = np.where(big, -x / 2 + y * k, -x / 2 + th * y / 12)
    return J


def plus(v, d):
    """x (+) d = x * Exp(d), vector form; x (+) 0 = x with its own bits."""
    v = np.asarray(v, dtype=np.float64); d = np.asarray(d, dtype=np.float64)
    out = vec(mat(v) @ exp(d))
    still = np.all(d == 0.0, axis=-1)
    return np.where(still[..., None], v, out)


def minus(a, b):
    """right-minus a (-) b = Log(b^-1 a)"""
    return log(inv(mat(b)) @ mat(a))


# ---- factors ---------------------------------------------------------------------------------------------------------
def huber_scale(delta, s):
    s = np.asarray(s, dtype=np.float64)
    if delta is None or delta <= 0:
        return np.ones_like(s)
    out = np.ones_like(s)
    m = s > delta * delta
    out[m] = np.sqrt(delta / np.sqrt(s[m]))
    return out


def between_linearize(k0, k1, m):
    """r (n, 3), J (n, 3, 6) = [dr/dk0 | dr/dk1] of r = Log((k1^-1 k0) m); inputs (n, 3) or (3,) vectors."""
    single = np.ndim(k0) == 1
    K0, K1, M = mat(np.atleast_2d(k0)), mat(np.atleast_2d(k1)), mat(np.atleast_2d(m))
    A = inv(K1) @ K0
    D = A @ M
    r = log(D)
    Jl = right_jacobian_inv(r)
    Am = adjoint(inv(M))
    J0 = Jl @ Am
    J1 = Jl @ (Am @ (-adjoint(inv(A))))
    J = np.concatenate([J0, J1], axis=-1)
    return (r[0], J[0]) if single else (r, J)


@dataclass
class Problem:
    poses: np.ndarray            # (n_v, 3), held wrapped
    e_from: np.ndarray
    e_to: np.ndarray
    meas: np.ndarray
    pose_col: np.ndarray         # first column of every vertex
    fix: np.ndarray              # (n_v, 3) uint8
    huber_delta: float | None = None
    priors: list = field(default_factory=list)   # (vertex, data[3], delta | None)
    scaling: np.ndarray | None = None

    def __post_init__(self):
        self.poses = np.array(self.poses, dtype=np.float64)
        self.poses[:, 2] = wrap(self.poses[:, 2])
        self.e_from = np.asarray(self.e_from, dtype=np.int64); self.e_to = np.asarray(self.e_to, dtype=np.int64)
        self.n_v = self.poses.shape[0]; self.n = 3 * self.n_v

    @classmethod
    def from_problem(cls, prob, poses=None):
        """from an apex_solver_amd.pose_graph.PoseGraphProblem on SE2 data"""
        d = prob.data
        return cls(d.poses if poses is None else poses, d.e_from, d.e_to, d.meas, prob.pose_col, prob.fix, prob.huber_delta,
                   list(prob.priors))

    def cols(self):
        return self.pose_col[:, None] + np.arange(3)[None]

    def edge_blocks(self):
        r, J = between_linearize(self.poses[self.e_from], self.poses[self.e_to], self.meas) if len(self.e_from) else (np.zeros((0, 3)), np.zeros((0, 3, 6)))
        sc = huber_scale(self.huber_delta, np.einsum("ei,ei->e", r, r))
        return r * sc[:, None], J * sc[:, None, None]

    def prior_blocks(self):
        rs, scs = [], []
        for v, data, delta in self.priors:
            r = self.poses[v] - np.asarray(data, dtype=np.float64)
            sc = float(huber_scale(delta, np.array([r @ r]))[0])
            rs.append(r * sc); scs.append(sc)
        return np.array(rs).reshape(-1, 3), np.array(scs)

    def cost(self):
        r, _ = self.edge_blocks()
        pr, _ = self.prior_blocks()
        nrm = np.sqrt(np.sum(r * r) + np.sum(pr * pr))
        return 0.5 * nrm * nrm

    def jacobian(self):
        """dense corrected (r, J) in residual-block order: edges, then priors"""
        r, Jb = self.edge_blocks()
        pr, psc = self.prior_blocks()
        ne, npri = r.shape[0], pr.shape[0]
        J = np.zeros((3 * (ne + npri), self.n))
        C = self.cols()
        for e in range(ne):   # a self-loop adds both blocks onto the same columns
            J[3 * e:3 * e + 3, C[self.e_from[e]]] += Jb[e, :, :3]
            J[3 * e:3 * e + 3, C[self.e_to[e]]] += Jb[e, :, 3:]
        for k, (v, _, _) in enumerate(self.priors):
            J[3 * (ne + k):3 * (ne + k) + 3, C[v]] += psc[k] * np.eye(3)
        return np.concatenate([r.ravel(), pr.ravel()]), J

    def normal_equations(self):
        """H = J^T J, g = J^T r in the (scaled) global columns"""
        r, J = self.jacobian()
        if self.scaling is not None:
            J = J * self.scaling[None, :]
        return J.T @ J, J.T @ r

    def solve(self, lam):
        H, g = self.normal_equations()
        A = H + lam * np.eye(self.n)
        try:
            Lc = np.linalg.cholesky(A)
        except np.linalg.LinAlgError:
            return None, g
        y = np.linalg.solve(Lc.T, np.linalg.solve(Lc, -g))
        return y, g

    def apply_step(self, step, sign=1.0):
        d = sign * step[self.cols()]
        d = np.where(self.fix.astype(bool), 0.0, d)
        self.poses = plus(self.poses, d)

    def parameter_norm(self):
        return float(np.sqrt(np.sum(self.poses * self.poses)))

    def lm_optimize(self, max_iterations=50, cost_tolerance=1e-6, parameter_tolerance=1e-8, gradient_tolerance=1e-10, damping=1e-3,
                    damping_min=1e-12, damping_max=1e12, nu=2.0, trust_region_radius=1e4, min_trust_region_radius=1e-32,
                    min_cost_threshold=-1.0, use_jacobi_scaling=False):
        lam = damping
        cost = self.cost()
        initial = cost
        hist = []
        it, status = 0, 1
        while True:
            if use_jacobi_scaling and it == 0:
                self.scaling = None
                H0, _ = self.normal_equations()
                self.scaling = 1.0 / (1.0 + np.sqrt(np.diag(H0)))
            y, grad = self.solve(lam)
            if y is None:
                status = 100
                break
            step = y * self.scaling if self.scaling is not None else y
            gn, sn = float(np.sqrt(grad @ grad)), float(np.sqrt(step @ step))
            pred = 0.5 * float(np.sum(step * (lam * step - grad)))
            before = self.poses.copy()
            self.apply_step(step, 1.0)
            new_cost = self.cost()
            actual = cost - new_cost
            rho = (1.0 if actual > 0 else 0.0) if abs(pred) < 1e-15 else actual / pred
            red = 0.0
            if rho > 0:
                coff = 2 * rho - 1
                lam = max(lam * max(1.0 / 3.0, 1 - coff ** 3), damping_min)
                nu = 2.0; accepted = 1
                red = cost - new_cost; cost = new_cost
            else:
                lam = min(lam * nu, damping_max); nu *= 2; accepted = 0
                self.apply_step(step, -1.0)
            hist.append([cost, lam, rho, accepted, gn, sn, pred, new_cost])
            pn = self.parameter_norm()
            cost_before = cost + red if accepted else cost
            st = -1
            if not (np.isfinite(cost) and np.isfinite(sn) and np.isfinite(gn)): st = 11
            elif it >= max_iterations: st = 1
            elif accepted:
                if gn < gradient_tolerance: st = 4
                if st < 0 and it > 0:
                    if sn <= parameter_tolerance * (pn + parameter_tolerance): st = 3
                    elif abs(cost_before - cost) / max(cost_before, 1e-10) < cost_tolerance: st = 2
                if st < 0 and min_cost_threshold >= 0 and cost < min_cost_threshold: st = 9
                if st < 0 and trust_region_radius < min_trust_region_radius: st = 8
            it += 1
            if st >= 0:
                status = st
                break
        self.scaling = None
        return dict(status=status, iterations=it, initial_cost=initial, final_cost=cost, history=np.array(hist).reshape(-1, 8))
