"""The reference's Gauss-Newton and Dog-Leg loops restated in numpy on dense H and g -- TEST INFRASTRUCTURE ONLY.

Statement by statement from (file:line under the apex-solver tree):
  GaussNewton::optimize_with_mode        src/optimizer/gauss_newton.rs:559-720   (step :491-526)
  DogLeg::compute_cauchy_point_and_alpha src/optimizer/dog_leg.rs:776-803
  DogLeg::compute_dog_leg_step           dog_leg.rs:818-902
  DogLeg::update_trust_region            dog_leg.rs:905-945
  DogLeg::compute_predicted_reduction    dog_leg.rs:948-960
  DogLeg::compute_optimization_step      dog_leg.rs:963-1089   (step reuse :969-1017, adaptive mu :1026-1039)
  DogLeg::optimize_with_mode             dog_leg.rs:1143-1354
  check_convergence, compute_step_quality src/optimizer/mod.rs:591-675
H = J^T J (undamped) and g = J^T r are what SparseCholeskySolver caches (cholesky.rs:103-157); with Jacobi scaling both are
in the scaled variables and the step handed to the retraction is D step_s.

The loops work on vectors, as the reference does.  `combine` is the same step from the six inner products only -- the form
apex-solver_amd/csrc/dogleg_combine.hpp takes -- kept here to check that header against, branch by branch.

A problem is anything with: n, scaling (None or a vector, settable), normal_equations() -> (H, g) in the scaled variables,
cost(), apply_step(step, sign), parameter_norm().  np_ref_se2.Problem is one; Se3Problem below is the SE3 one on np_ref_pg.
"""
from __future__ import annotations

import numpy as np

import np_ref_pg

GAUSS_NEWTON, STEEPEST_DESCENT, DOG_LEG = 0, 1, 2
MAX_CACHE_REUSE = 5


class Se3Problem:
    """SE3 pose graph with PriorFactor blocks on np_ref_pg: the interface np_ref_se2.Problem has."""

    def __init__(self, poses, e_from, e_to, meas, pose_col, fix, huber_delta=None, priors=()):
        self.poses = np.array(poses, dtype=np.float64)
        self.e_from = np.asarray(e_from, dtype=np.int64); self.e_to = np.asarray(e_to, dtype=np.int64)
        self.meas = np.asarray(meas, dtype=np.float64)
        self.pose_col = np.asarray(pose_col, dtype=np.int64); self.fix = np.asarray(fix)
        self.huber_delta = huber_delta; self.priors = list(priors)
        self.n_v = self.poses.shape[0]; self.n = 6 * self.n_v
        self.scaling = None

    @classmethod
    def from_problem(cls, prob, poses=None):
        d = prob.data
        return cls(d.poses if poses is None else poses, d.e_from, d.e_to, d.meas, prob.pose_col, prob.fix, prob.huber_delta, prob.priors)

    def _vector(self, v):   # SE3::from(DVector).to_vector(): the quaternion normalised twice
        p = self.poses[v].copy()
        for _ in range(2):
            p[3:7] = p[3:7] / np.sqrt(p[3:7] @ p[3:7])
        return p

    def prior_blocks(self):
        rs, scs = [], []
        for v, data, delta in self.priors:
            r = self._vector(v) - np.asarray(data, dtype=np.float64)
            s = r @ r
            sc = np.sqrt(delta / np.sqrt(s)) if (delta is not None and delta > 0 and s > delta * delta) else 1.0
            rs.append(r * sc); scs.append(sc)
        return np.array(rs).reshape(-1, 7), np.array(scs)

    def cost(self):
        r, _ = np_ref_pg.linearize(self.poses, self.e_from, self.e_to, self.meas, self.huber_delta)
        pr, _ = self.prior_blocks()
        nrm = np.sqrt(np.sum(r * r) + np.sum(pr * pr))
        return 0.5 * nrm * nrm

    def jacobian(self):
        """dense corrected (r, J): edges, then priors (7 rows each, J = sc [I6; 0])"""
        r, Jb = np_ref_pg.linearize(self.poses, self.e_from, self.e_to, self.meas, self.huber_delta)
        pr, psc = self.prior_blocks()
        ne, npri = r.shape[0], pr.shape[0]
        J = np.zeros((6 * ne + 7 * npri, self.n))
        for e in range(ne):   # a self-loop adds both blocks onto the same columns
            c0 = self.pose_col[self.e_from[e]] + np.arange(6); c1 = self.pose_col[self.e_to[e]] + np.arange(6)
            J[6 * e:6 * e + 6, c0] += Jb[e, :, :6]
            J[6 * e:6 * e + 6, c1] += Jb[e, :, 6:]
        for k, (v, _, _) in enumerate(self.priors):
            J[6 * ne + 7 * k + np.arange(6), self.pose_col[v] + np.arange(6)] += psc[k]
        return np.concatenate([r.ravel(), pr.ravel()]), J

    def normal_equations(self):
        r, J = self.jacobian()
        if self.scaling is not None:
            J = J * self.scaling[None, :]
        return J.T @ J, J.T @ r

    def apply_step(self, step, sign=1.0):
        self.poses = np_ref_pg.retract(self.poses, step, self.pose_col, self.fix, sign)

    def parameter_norm(self):
        return float(np.sqrt(np.sum(self.poses * self.poses)))


# ---- the pieces of a Dog-Leg step, on vectors ------------------------------------------------------------------------
def solve_damped(H, g, mu):
    """(H + mu I) h = -g by Cholesky; None on a non-positive pivot (solve_augmented_equation's error)"""
    try:
        L = np.linalg.cholesky(H + mu * np.eye(H.shape[0]))
    except np.linalg.LinAlgError:
        return None
    return np.linalg.solve(L.T, np.linalg.solve(L, -g))


def cauchy_point(H, g):
    g_h_g = float(g @ (H @ g))
    alpha = float(g @ g) / g_h_g if abs(g_h_g) > 1e-15 else 1.0
    return alpha, -alpha * g


def dog_leg_step(sd, p_c, h, delta):
    """(step, type, beta) -- dog_leg.rs:818-902"""
    gn_norm, cauchy_norm, sd_norm = np.linalg.norm(h), np.linalg.norm(p_c), np.linalg.norm(sd)
    if gn_norm <= delta:
        return h.copy(), GAUSS_NEWTON, 0.0
    if cauchy_norm >= delta:
        return sd * (delta / sd_norm), STEEPEST_DESCENT, 0.0
    v = h - p_c
    a = float(v @ v); b = float(p_c @ v); c = cauchy_norm * cauchy_norm - delta * delta
    d2 = b * b - a * c
    if d2 < 0.0:
        beta = 1.0
    elif abs(a) < 1e-15:
        beta = 1.0
    else:
        d = np.sqrt(d2)
        beta = (-b + d) / a if b <= 0.0 else -c / (b + d)
    beta = min(max(beta, 0.0), 1.0)
    return p_c + beta * v, DOG_LEG, beta


def predicted_reduction(step, g, H):
    return -float(step @ g) - 0.5 * float(step @ (H @ step))


def combine(gg, hh, gh, uu, uw, ww, delta):
    """The same step from the inner products g.g, h.h, g.h, g.Hg, g.Hh, h.Hh: step = c_g (-g) + c_h h."""
    alpha = gg / uu if abs(uu) > 1e-15 else 1.0
    gn_norm, sd_norm = np.sqrt(hh), np.sqrt(gg)
    cauchy_norm = abs(alpha) * sd_norm
    beta = 0.0
    if gn_norm <= delta:
        typ, cg, ch = GAUSS_NEWTON, 0.0, 1.0
    elif cauchy_norm >= delta:
        typ, cg, ch = STEEPEST_DESCENT, delta / sd_norm, 0.0
    else:
        a = hh + 2.0 * alpha * gh + alpha * alpha * gg
        b = -alpha * gh - alpha * alpha * gg
        c = cauchy_norm * cauchy_norm - delta * delta
        d2 = b * b - a * c
        if d2 < 0.0:
            beta = 1.0
        elif abs(a) < 1e-15:
            beta = 1.0
        else:
            d = np.sqrt(d2)
            beta = (-b + d) / a if b <= 0.0 else -c / (b + d)
        beta = min(max(beta, 0.0), 1.0)
        typ, cg, ch = DOG_LEG, alpha * (1.0 - beta), beta
    n2 = cg * cg * gg - 2.0 * cg * ch * gh + ch * ch * hh
    pred = cg * gg - ch * gh - 0.5 * (cg * cg * uu - 2.0 * cg * ch * uw + ch * ch * ww)
    return dict(alpha=alpha, beta=beta, c_g=cg, c_h=ch, step_norm=float(np.sqrt(max(n2, 0.0))), predicted_reduction=pred, type=typ)


def sums_of(H, g, h):
    Hg, Hh = H @ g, H @ h
    return float(g @ g), float(h @ h), float(g @ h), float(g @ Hg), float(g @ Hh), float(h @ Hh)


# ---- convergence -----------------------------------------------------------------------------------------------------
def check_convergence(iteration, cost_before, cost, pnorm, sn, gn, accepted, max_iterations, gradient_tolerance, parameter_tolerance,
                      cost_tolerance, min_cost_threshold=None, radius=None, min_radius=None):
    if not (np.isfinite(cost) and np.isfinite(sn) and np.isfinite(gn)): return 11
    if iteration >= max_iterations: return 1
    if not accepted: return -1
    if gn < gradient_tolerance: return 4
    if iteration > 0:
        if sn <= parameter_tolerance * (pnorm + parameter_tolerance): return 3
        if abs(cost_before - cost) / max(cost_before, 1e-10) < cost_tolerance: return 2
    if min_cost_threshold is not None and cost < min_cost_threshold: return 9
    if radius is not None and min_radius is not None and radius < min_radius: return 8
    return -1


def step_quality(cost, new_cost, pred):
    actual = cost - new_cost
    if abs(pred) < 1e-15:
        return 1.0 if actual > 0.0 else 0.0
    return actual / pred


def _init_scaling(P, on):
    P.scaling = None
    if on:   # process_jacobian_generic (optimizer/mod.rs:749-763): from the Jacobian of iteration 0
        H0, _ = P.normal_equations()
        P.scaling = 1.0 / (1.0 + np.sqrt(np.diag(H0)))


# ---- the loops -------------------------------------------------------------------------------------------------------
def gauss_newton(P, max_iterations=50, cost_tolerance=1e-6, parameter_tolerance=1e-8, gradient_tolerance=1e-10,
                 min_cost_threshold=None, use_jacobi_scaling=False):
    """history rows: cost, 0, 0, 1, |g|, |step|, -, trial cost (LmIterC's columns)"""
    cost = P.cost(); initial = cost
    _init_scaling(P, use_jacobi_scaling)
    hist, it, status = [], 0, 1
    while True:
        H, g = P.normal_equations()
        y = solve_damped(H, g, 0.0)   # solve_normal_equation
        if y is None:
            status = 100
            break
        step = y * P.scaling if P.scaling is not None else y
        gn, sn = float(np.linalg.norm(g)), float(np.linalg.norm(step))
        cost_before = cost
        P.apply_step(step, 1.0)
        cost = P.cost()
        hist.append([cost, 0.0, 0.0, 1.0, gn, sn, np.nan, cost])
        st = check_convergence(it, cost_before, cost, P.parameter_norm(), sn, gn, True, max_iterations, gradient_tolerance,
                               parameter_tolerance, cost_tolerance, min_cost_threshold)
        it += 1
        if st >= 0:
            status = st
            break
    P.scaling = None
    return dict(status=status, iterations=it, initial_cost=initial, final_cost=cost, history=np.array(hist).reshape(-1, 8))


def dog_leg(P, max_iterations=50, cost_tolerance=1e-6, parameter_tolerance=1e-8, gradient_tolerance=1e-10, trust_region_radius=1e4,
            trust_region_min=1e-12, trust_region_max=1e12, trust_region_decrease_factor=0.5, good_step_quality=0.75,
            poor_step_quality=0.25, use_jacobi_scaling=True, initial_mu=1e-4, min_mu=1e-8, max_mu=1.0, mu_increase_factor=10.0,
            enable_step_reuse=True, min_cost_threshold=None):
    """history rows: cost, radius, mu, rho, accepted, |g|, |step|, predicted, trial cost, type, beta, reused (DlIterC's columns);
    `margins`: per iteration the smallest relative distance of a decision from its threshold (|h|, |p_c| against the radius;
    rho against 1e-4, poor, good)."""
    radius, mu = trust_region_radius, initial_mu
    reuse_flag, cache, reuse_count = False, None, 0
    solver_H = None   # linear_solver.get_hessian(): the Hessian of the last solve
    cost = P.cost(); initial = cost
    _init_scaling(P, use_jacobi_scaling)
    hist, margins, it, status = [], [], 0, 1
    while True:
        reused = bool(reuse_flag and enable_step_reuse and reuse_count < MAX_CACHE_REUSE and cache is not None)
        if reused:
            reuse_count += 1
            h, p_c, g = cache
            H = solver_H
        else:
            H, g = P.normal_equations()   # at the current point
            h, attempts = None, 0
            while attempts < 10 and mu <= max_mu:
                h = solve_damped(H, g, mu)
                if h is not None:
                    break
                mu = min(mu * mu_increase_factor, max_mu)
                attempts += 1
            if h is None:
                status = 100
                break
            solver_H = H
            _, p_c = cauchy_point(H, g)
            cache = (h, p_c, g)
        gn = float(np.linalg.norm(g))
        step_s, typ, beta = dog_leg_step(-g, p_c, h, radius)
        step = step_s * P.scaling if P.scaling is not None else step_s
        pred = predicted_reduction(step_s, g, H)
        sn = float(np.linalg.norm(step))
        P.apply_step(step, 1.0)
        new_cost = P.cost()
        rho = step_quality(cost, new_cost, pred)
        m = [abs(np.linalg.norm(h) - radius) / radius]
        if np.linalg.norm(h) > radius:
            m.append(abs(np.linalg.norm(p_c) - radius) / radius)
        m += [abs(rho - 1e-4) / 1e-4, abs(rho - poor_step_quality) / poor_step_quality, abs(rho - good_step_quality) / good_step_quality]
        margins.append(min(m))
        accepted = rho > 1e-4
        if rho > good_step_quality:
            radius = min(max(radius, 3.0 * sn), trust_region_max)
            mu = max(mu / (0.5 * mu_increase_factor), min_mu)
            reuse_flag, cache, reuse_count = False, None, 0
        elif rho < poor_step_quality:
            radius = max(radius * trust_region_decrease_factor, trust_region_min)
            reuse_flag = enable_step_reuse
        else:
            reuse_flag, cache, reuse_count = False, None, 0
        red = 0.0
        if accepted:
            red = cost - new_cost; cost = new_cost
        else:
            P.apply_step(step, -1.0)
        hist.append([cost, radius, mu, rho, float(accepted), gn, sn, pred, new_cost, float(typ), beta, float(reused)])
        cost_before = cost + red if accepted else cost
        st = check_convergence(it, cost_before, cost, P.parameter_norm(), sn, gn, accepted, max_iterations, gradient_tolerance,
                               parameter_tolerance, cost_tolerance, min_cost_threshold, radius, trust_region_min)
        it += 1
        if st >= 0:
            status = st
            break
    P.scaling = None
    return dict(status=status, iterations=it, initial_cost=initial, final_cost=cost, history=np.array(hist).reshape(-1, 12),
                margins=np.array(margins), radius=radius, mu=mu)


# ---- the reference's Rosenbrock factor pair (dog_leg.rs:1426-1485): r1 = 10 (x2 - x1^2), r2 = 1 - x1 on two Rn(1) variables --------
class Rosenbrock:
    def __init__(self, x=(-1.2, 1.0)):
        self.x = np.array(x, dtype=np.float64); self.n = 2; self.scaling = None

    def residual(self):
        return np.array([10.0 * (self.x[1] - self.x[0] * self.x[0]), 1.0 - self.x[0]])

    def cost(self):
        nrm = np.linalg.norm(self.residual())
        return 0.5 * nrm * nrm

    def normal_equations(self):
        J = np.array([[-20.0 * self.x[0], 10.0], [-1.0, 0.0]])
        if self.scaling is not None:
            J = J * self.scaling[None, :]
        return J.T @ J, J.T @ self.residual()

    def apply_step(self, step, sign=1.0):
        self.x = self.x + sign * np.asarray(step)

    def parameter_norm(self):
        return float(np.linalg.norm(self.x))
