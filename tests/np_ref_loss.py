"""The reference's loss functions and corrector restated in numpy, in np.longdouble -- TEST INFRASTRUCTURE ONLY.

Statement by statement from (file:line under the apex-solver tree):
  LossFunction::evaluate   src/core/loss_functions.rs  L2 176-178, L1 238-249, Huber 364-380, Cauchy 497-507, Fair 587-606,
                           Geman-McClure 676-686, Welsch 761-769, Tukey 850-868, Andrews 951-968, Ramsay 1039-1054,
                           trimmed mean 1134-1140, Lp 1209-1223, Barron 1318-1354, Student t 1447-1460, AdaptiveBarron 1569-1574
  the constructors         loss_functions.rs:340-351, 472-484, 575-582, 663-672, 745-757, 835-846, 935-947, 1024-1035,
                           1120-1130, 1199-1205, 1302-1314, 1432-1443
  Corrector::new           src/core/corrector.rs:143-181
  correct_jacobian         corrector.rs:233-254     J~ = sqrt(rho') (J - alpha_sq_norm r r^T J)
  correct_residuals        corrector.rs:292-298     r~ = residual_scaling r
The branches compare the fp64 squared norm, as the reference does; the arithmetic behind them is extended precision, so
that this file is a reference for fp64 code and not a second fp64 rounding of it.

A loss is anything with .kind (capi.LOSS_*), .p0, .p1: apex_solver_amd.pose_graph.Loss is one.
"""
from __future__ import annotations

import numpy as np

import np_ref_pg
import np_ref_se2
import np_ref_trust_region as tr
from apex_solver_amd import capi

LD = np.longdouble
EPS = float(np.finfo(np.float64).eps)        # f64::EPSILON
F64_MIN = LD(-np.finfo(np.float64).max)      # f64::MIN
PI = LD(np.pi)                               # std::f64::consts::PI (the fp64 constant)


def valid(loss) -> bool:
    """what each new() accepts"""
    k = loss.kind
    if k in (capi.LOSS_NONE, capi.LOSS_L2, capi.LOSS_L1):
        return True
    if k == capi.LOSS_BARRON:
        return loss.p1 > 0.0
    if capi.LOSS_HUBER <= k <= capi.LOSS_T_DISTRIBUTION:
        return loss.p0 > 0.0
    return False


def thresholds(loss):
    """the squared norms at which evaluate() or the corrector changes branch (besides s == 0)"""
    k, c = loss.kind, loss.p0
    if k in (capi.LOSS_L1, capi.LOSS_FAIR, capi.LOSS_LP_NORM):
        return [EPS]
    if k in (capi.LOSS_HUBER, capi.LOSS_TUKEY, capi.LOSS_TRIMMED_MEAN):
        return [c * c]
    if k == capi.LOSS_ANDREWS:   # suppression beyond pi c; rho'' changes sign at pi c / 2 (the corrector's arm)
        return [float(PI * LD(c)) ** 2, (0.5 * float(PI) * c) ** 2]
    return []


def evaluate(loss, s, dtype=LD):
    """[rho, rho', rho''] at the fp64 squared norm s.  dtype: the arithmetic behind the branches -- np.longdouble (the reference), or
    np.float64: the same statements as an fp64 evaluation of them, whose distance from the reference is what fp64 code may be off by
    (as tile_ref.selected_inverse takes a dtype)"""
    LD = dtype
    s64 = float(s)
    s = LD(s64)
    F64_MIN, PI = LD(-np.finfo(np.float64).max), LD(np.pi)
    k = loss.kind
    p0, p1 = LD(loss.p0), LD(loss.p1)
    l2 = np.array([s, LD(1), LD(0)], dtype=LD)
    if k in (capi.LOSS_NONE, capi.LOSS_L2):
        return l2
    if k == capi.LOSS_L1:
        if s64 < EPS:
            return l2
        q = np.sqrt(s)
        return np.array([2 * q, 1 / q, -1 / (2 * s * q)], dtype=LD)
    if k == capi.LOSS_HUBER:
        scale2 = float(np.float64(loss.p0) * np.float64(loss.p0))
        if s64 > scale2:
            r = np.sqrt(s)
            rho1 = max(p0 / r, F64_MIN)
            return np.array([2 * p0 * r - p0 * p0, rho1, -rho1 / (2 * s)], dtype=LD)
        return l2
    if k == capi.LOSS_CAUCHY:
        scale2 = p0 * p0
        c = 1 / scale2
        sm = 1 + s * c
        inv = 1 / sm
        return np.array([scale2 * np.log(sm) / 2, max(inv, F64_MIN), -c * (inv * inv)], dtype=LD)
    if k == capi.LOSS_FAIR:
        if s64 < EPS:
            return l2
        ax = abs(np.sqrt(s))
        cpx = p0 + ax
        return np.array([p0 * p0 * (ax / p0 - np.log(1 + ax / p0)), LD(0.5) / cpx, -1 / (4 * s * cpx * cpx)], dtype=LD)
    if k == capi.LOSS_GEMAN_MCCLURE:
        c = 1 / (p0 * p0)
        inv = 1 / (1 + s * c)
        inv2 = inv * inv
        return np.array([s * inv, inv2, -2 * c * inv2 * inv], dtype=LD)
    if k == capi.LOSS_WELSCH:
        scale2 = p0 * p0
        e = np.exp(-s / scale2)
        return np.array([(scale2 / 2) * (1 - e), LD(0.5) * e, -LD(0.5) / scale2 * e], dtype=LD)
    if k == capi.LOSS_TUKEY:
        scale2 = p0 * p0
        if float(np.sqrt(np.float64(s64))) > loss.p0:
            return np.array([scale2 / 6, 0, 0], dtype=LD)
        ratio = np.sqrt(s) / p0
        om = 1 - ratio * ratio
        return np.array([(scale2 / 6) * (1 - om * om * om), LD(0.5) * om * om, -(ratio / scale2) * om], dtype=LD)
    if k == capi.LOSS_ANDREWS:
        scale2 = p0 * p0
        if float(np.sqrt(np.float64(s64))) > float(np.float64(np.pi) * np.float64(loss.p0)):
            return np.array([2 * scale2, 0, 0], dtype=LD)
        x = np.sqrt(s)
        arg = x / p0
        return np.array([scale2 * (1 - np.cos(arg)), LD(0.5) * np.sin(arg), (LD(0.25) / p0) * np.cos(arg) / max(x, LD(EPS))], dtype=LD)
    if k == capi.LOSS_RAMSAY:
        x = np.sqrt(s)
        ax = p0 * x
        e = np.exp(-ax)
        return np.array([(1 / (p0 * p0)) * (1 - e * (1 + ax)), LD(0.5) * e, -(p0 / (4 * max(x, LD(EPS)))) * e], dtype=LD)
    if k == capi.LOSS_TRIMMED_MEAN:
        scale2 = float(np.float64(loss.p0) * np.float64(loss.p0))
        if s64 <= scale2:
            return np.array([s / 2, LD(0.5), 0], dtype=LD)
        return np.array([LD(scale2) / 2, 0, 0], dtype=LD)
    if k == capi.LOSS_LP_NORM:
        if s64 < EPS:
            return l2
        e0 = p0 / 2
        e1 = e0 - 1
        e2 = e1 - 1
        return np.array([np.power(s, e0), e0 * np.power(s, e1), e0 * e1 * np.power(s, e2)], dtype=LD)
    if k == capi.LOSS_BARRON:
        alpha, scale2 = p0, p1 * p1
        if abs(loss.p0) < 1e-6:
            den = 1 + s / scale2
            inv = 1 / den
            return np.array([(scale2 / 2) * np.log(den), max(inv, F64_MIN), -inv * inv / scale2], dtype=LD)
        if abs(loss.p0 - 2.0) < 1e-6:
            return l2
        nrm = np.sqrt(s) / p1
        inner = abs(alpha) / 2 * (nrm * nrm) + 1
        return np.array([(abs(alpha) / scale2) * (np.power(inner, alpha / 2) - 1), LD(0.5) * np.power(inner, alpha / 2 - 1),
                         (alpha - 2) / (4 * scale2) * np.power(inner, alpha / 2 - 2)], dtype=LD)
    if k == capi.LOSS_T_DISTRIBUTION:
        h = (p0 + 1) / 2
        den = p0 + s
        return np.array([h * np.log(1 + s / p0), h / den, -h / (den * den)], dtype=LD)
    raise ValueError(f"unknown loss kind {k}")


def corrector(loss, s, dtype=LD):
    """(sqrt_rho1, residual_scaling, alpha_sq_norm, arm) -- arm 1 | 2"""
    return corrector_of(evaluate(loss, s, dtype), s, dtype)


def corrector_of(rho, s, dtype=LD):
    """Corrector::new on a given (rho, rho', rho''), in the arithmetic of dtype"""
    LD = dtype
    rho = np.asarray(rho, dtype=LD)
    with np.errstate(invalid="ignore"):
        sq = np.sqrt(rho[1])
    if float(s) == 0.0 or rho[2] <= 0:
        return sq, sq, LD(0), 1
    d = max(1 + 2 * LD(float(s)) * rho[2] / rho[1], LD(0))
    alpha = 1 - np.sqrt(d)
    return sq, sq / (1 - alpha), alpha / LD(float(s)), 2


def six(loss, s):
    """what apexgpu_loss_evaluate returns, in extended precision"""
    c = corrector(loss, s)
    return np.concatenate([evaluate(loss, s), np.array(c[:3], dtype=LD)])


def correct(r, J, loss, dtype=LD):
    """(r~, the literal J~, arm) of one residual block: r (m,), J (m, n), uncorrected, fp64.  s is the fp64 squared norm the
    device forms (left to right).  dtype: the arithmetic of the correction (evaluate)."""
    LD = dtype
    r64 = np.asarray(r, dtype=np.float64)
    s = np.float64(0.0)
    for x in r64:
        s = s + x * x
    sq, rs, a, arm = corrector(loss, float(s), dtype)
    rl, Jl = r64.astype(LD), np.asarray(J, dtype=np.float64).astype(LD)
    if arm == 1:
        return rl * rs, Jl * sq, 1, float(s)
    return rl * rs, (Jl - a * np.outer(rl, rl @ Jl)) * sq, 2, float(s)


def correct_edges(r, J, loss):
    """edge arrays r (n, m), J (n, m, 2m) -> corrected fp64 copies, the arm and s of every edge"""
    ro = np.zeros_like(r); Jo = np.zeros_like(J); arms = np.zeros(len(r), int); ss = np.zeros(len(r))
    for e in range(len(r)):
        a, b, arms[e], ss[e] = correct(r[e], J[e], loss)
        ro[e], Jo[e] = a.astype(np.float64), b.astype(np.float64)
    return ro, Jo, arms, ss


def threshold_margin(loss, ss):
    """smallest relative distance of any s from a branch threshold of the loss"""
    m = np.inf
    for t in thresholds(loss):
        m = min(m, float(np.min(np.abs(np.asarray(ss) - t) / t)))
    return m


# ---- problems whose linearize goes through this file: the interface np_ref_trust_region's loops take ----------------
class Se3LossProblem(tr.Se3Problem):
    def __init__(self, *a, loss=None, **k):
        super().__init__(*a, **k)
        self.loss = loss

    @classmethod
    def from_problem(cls, prob, poses=None):
        d = prob.data
        return cls(d.poses if poses is None else poses, d.e_from, d.e_to, d.meas, prob.pose_col, prob.fix, None, prob.priors, loss=prob.loss)

    def edge_blocks(self):
        r, J = np_ref_pg.linearize(self.poses, self.e_from, self.e_to, self.meas, None)
        r, J, self.arms, self.s = correct_edges(r, J, self.loss)
        return r, J

    def cost(self):
        r, _ = self.edge_blocks()
        pr, _ = self.prior_blocks()
        nrm = np.sqrt(np.sum(r * r) + np.sum(pr * pr))
        return 0.5 * nrm * nrm

    def jacobian(self):
        r, Jb = self.edge_blocks()
        pr, psc = self.prior_blocks()
        ne, npri = r.shape[0], pr.shape[0]
        J = np.zeros((6 * ne + 7 * npri, self.n))
        for e in range(ne):
            c0 = self.pose_col[self.e_from[e]] + np.arange(6); c1 = self.pose_col[self.e_to[e]] + np.arange(6)
            J[6 * e:6 * e + 6, c0] += Jb[e, :, :6]
            J[6 * e:6 * e + 6, c1] += Jb[e, :, 6:]
        for k, (v, _, _) in enumerate(self.priors):
            J[6 * ne + 7 * k + np.arange(6), self.pose_col[v] + np.arange(6)] += psc[k]
        return np.concatenate([r.ravel(), pr.ravel()]), J


class Se2LossProblem(np_ref_se2.Problem):
    loss = None

    @classmethod
    def from_problem(cls, prob, poses=None):
        d = prob.data
        p = cls(d.poses if poses is None else poses, d.e_from, d.e_to, d.meas, prob.pose_col, prob.fix, None, list(prob.priors))
        p.loss = prob.loss
        return p

    def edge_blocks(self):
        r, J = np_ref_se2.between_linearize(self.poses[self.e_from], self.poses[self.e_to], self.meas)
        r, J, self.arms, self.s = correct_edges(r, J, self.loss)
        return r, J


def lm(P, max_iterations, damping=1e-3, damping_min=1e-12, damping_max=1e12, cost_tolerance=1e-6, parameter_tolerance=1e-8,
       gradient_tolerance=1e-10):
    """LevenbergMarquardt::optimize (levenberg_marquardt.rs) on a problem of np_ref_trust_region's interface, no scaling:
    the loop np_ref_se2.Problem.lm_optimize spells, beside gauss_newton and dog_leg.  history rows: LmIterC's columns."""
    lam, nu = damping, 2.0
    cost = P.cost(); initial = cost
    hist, it, status = [], 0, 1
    while True:
        H, g = P.normal_equations()
        y = tr.solve_damped(H, g, lam)
        if y is None:
            status = 100
            break
        gn, sn = float(np.sqrt(g @ g)), float(np.sqrt(y @ y))
        pred = 0.5 * float(np.sum(y * (lam * y - g)))
        P.apply_step(y, 1.0)
        new_cost = P.cost()
        actual = cost - new_cost
        rho = (1.0 if actual > 0 else 0.0) if abs(pred) < 1e-15 else actual / pred
        red = 0.0
        if rho > 0:
            lam = max(lam * max(1.0 / 3.0, 1 - (2 * rho - 1) ** 3), damping_min)
            nu = 2.0; accepted = 1
            red = cost - new_cost; cost = new_cost
        else:
            lam = min(lam * nu, damping_max); nu *= 2; accepted = 0
            P.apply_step(y, -1.0)
        hist.append([cost, lam, rho, accepted, gn, sn, pred, new_cost])
        cost_before = cost + red if accepted else cost
        st = tr.check_convergence(it, cost_before, cost, P.parameter_norm(), sn, gn, bool(accepted), max_iterations,
                                  gradient_tolerance, parameter_tolerance, cost_tolerance)
        it += 1
        if st >= 0:
            status = st
            break
    return dict(status=status, iterations=it, initial_cost=initial, final_cost=cost, history=np.array(hist).reshape(-1, 8))
