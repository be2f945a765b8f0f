"""Bundle adjustment behind the problem interface of tests/np_ref_trust_region.py -- TEST INFRASTRUCTURE ONLY.

BaProblem has n, scaling, normal_equations(), cost(), apply_step(), parameter_norm() on np_ref.py (jacobian_blocks,
sparse_jacobian, retract), the general losses of np_ref_ba_loss.py and the per-DOF masks of fixed_masks.py, so that the numpy
Dog-Leg loop (np_ref_trust_region.dog_leg) runs on a BA problem as it does on a pose graph.  H = J^T J is dense and in the
reference's global column order; a fixed DOF keeps its column and is zeroed where the step is applied (core/problem.rs:185-197).

The cases at the bottom are what tests/test_ba_trust_region_ref_host.py (CPU: the premises, on numpy alone) and
tests/test_gpu_ba_trust_region.py (device) share.  Their constants -- start noise, seed, first radius -- were chosen by running the
numpy loop alone until every decision of the run (|h| and |p_c| against the radius, rho against 1e-4, 0.25, 0.75) stayed more
than 1e-6 relative from its threshold; the CPU test asserts that, so that a flipped branch cannot hide in the device test.
"""
from __future__ import annotations

import functools
import os

import numpy as np

import apex_solver_amd as pkg
import ba_custom
import fixed_masks as fm
import np_ref
import np_ref_ba_loss as nb
import np_ref_trust_region as tr
from apex_solver_amd import capi
from apex_solver_amd.loss import Loss
from apex_solver_amd.solver import OptimizationType, Problem
from apex_solver_amd.synthetic import BAProblemData

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
OT = {"ba": OptimizationType.BundleAdjustment, "selfcal": OptimizationType.SelfCalibration}


def huber(delta):
    return Loss(capi.LOSS_HUBER, float(delta))


class BaProblem:
    """d: BAProblemData (structure and measurements); params: (poses, intr, points), default d's; opt: OptimizationType;
    loss: Loss or None; masks: a fixed_masks dict or None."""

    def __init__(self, d, opt=OptimizationType.SelfCalibration, loss=None, masks=None, params=None):
        self.d, self.opt, self.loss = d, opt, loss
        self.lay = pkg.layout.reference_column_layout(d.n_cam, d.n_pt)
        self.masks = masks if masks is not None else fm.empty(d.n_cam, d.n_pt)
        p = params if params is not None else (d.poses, d.intr, d.points)
        self.params = tuple(np.array(x, dtype=np.float64) for x in p)
        self.ci, self.pi = d.cam_idx.astype(int), d.pt_idx.astype(int)
        self.selfcal = opt.value in (1, 4, 5, 6)   # the intrinsics have columns on the device (d_c = 9)
        self.n = self.lay.total_dof
        self.scaling = None

    def jacobian(self):
        """(r~, J~): corrected, sparse, the reference's global columns, unscaled"""
        r, Jp, Jl, Ji, _, _ = nb.linearize(*self.params, self.ci, self.pi, self.d.obs_uv, self.loss)
        fp, fl, fi = self.opt.flags
        J = np_ref.sparse_jacobian(Jp * fp, Jl * fl, Ji * (fi if self.selfcal else 0), self.ci, self.pi, self.lay, selfcal=self.selfcal)
        return r.ravel(), J

    def normal_equations(self):
        r, J = self.jacobian()
        J = J.toarray()
        if self.scaling is not None:
            J = J * self.scaling[None, :]
        return J.T @ J, J.T @ r

    def cost(self):
        r = np_ref.residuals(*self.params, self.ci, self.pi, self.d.obs_uv, huber_delta=0)[0]
        rt = r * nb.weights(self.loss, nb.squared_norms(r))[:, None]
        nrm = np.sqrt(np.sum(rt * rt))
        return 0.5 * nrm * nrm

    def apply_step(self, step, sign=1.0):
        m = self.masks
        self.params = np_ref.retract(*self.params, np.asarray(step), self.lay, fix_pose=m["pose"], fix_intr=m["intr"], fix_pt=m["pt"], sign=sign)

    def parameter_norm(self):
        return float(np.sqrt(sum(np.sum(x * x) for x in self.params)))

    def mask_vector(self):
        """True at every fixed global column"""
        v = np.zeros(self.n, bool)
        lay, m = self.lay, self.masks
        for col, w, key in ((lay.pose_col, 6, "pose"), (lay.intr_col, 3, "intr"), (lay.pt_col, 3, "pt")):
            v[col[:, None] + np.arange(w)[None]] = m[key].astype(bool)
        return v


# ---- the problems -----------------------------------------------------------------------------------------------------------------
def golden_data(name):
    """(BAProblemData at the golden's start, OptimizationType, huber delta, the npz)"""
    g = np.load(os.path.join(GOLDEN, name + ".npz"))
    d = BAProblemData(g["poses0"], g["intr0"], g["points0"], g["cam_idx"], g["pt_idx"], np.ascontiguousarray(g["obs_uv"]))
    return d, OT[str(g["mode"])], float(g["huber_delta"]), g


# ba_custom structure: a landmark of ONE observation, a landmark of more than 256 (it crosses a 256-lane workgroup of the Gram
# kernel, whatever its place in the stream) and an observation count that is no multiple of 64 (a partial last wave)
CUSTOM_CAMS = 12


def custom_lists():
    rng = np.random.default_rng(3)
    lists = [[0], list(np.arange(300) % CUSTOM_CAMS)]
    for l in range(2, 60):
        lists.append(list(rng.choice(CUSTOM_CAMS, size=2 + l % 4, replace=False)))
    return lists


@functools.lru_cache(maxsize=None)
def custom_data(outlier_every=0):
    d = ba_custom.custom_problem(CUSTOM_CAMS, custom_lists(), seed=5, noise=0.7, outlier_every=outlier_every)
    assert d.n_obs % 64 != 0 and np.bincount(d.pt_idx).max() > 256 and np.bincount(d.pt_idx).min() == 1
    return d


def gauge(d):
    return fm.with_gauge(fm.empty(d.n_cam, d.n_pt))


def device_problem(P):
    """the apex_solver_amd Problem of a BaProblem: no huber_delta, the loss through set_loss, the masks by name"""
    return fm.apply_to_problem(Problem(P.d, P.opt, None, loss=P.loss), P.masks)


def first_linearisation(P, scaling, mu):
    """H, g (scaled variables), D (or None), h, alpha, p_c at P's point"""
    tr._init_scaling(P, scaling)
    H, g = P.normal_equations()
    h = tr.solve_damped(H, g, mu)
    alpha, p_c = tr.cauchy_point(H, g)
    return H, g, P.scaling, h, alpha, p_c


def mu_for_condition(H, bound=1e5):
    """the smallest power of ten mu with cond(H + mu I) <= bound"""
    ev = np.linalg.eigvalsh(H)
    mu = 10.0 ** np.ceil(np.log10(max(ev[-1], 1e-300) / (bound - 1.0)))
    return float(mu)


# ---- the Dog-Leg runs the history tests compare with ---------------------------------------------------------------------------------
# (problem, loss): the golden's own start (its parameters are the truth plus the generator's noise).  RADIUS0: the first radius as a
# fraction of the Cauchy step's length at the run's first mu; DL_ITERS: iterations compared.
# MU: Dog-Leg's mu range where it is not the default.  The unscaled run without a loss takes good steps from the start, and the
# default mu sinks from 1e-4 to 1.6e-7 by the fourth iteration while lambda_max(H) = 1.1e6 px^2: cond(H + mu I) = 7e12, at which
# two fp64 solves of one system (numpy's dense Cholesky, the device's Schur elimination) agree to cond 2^-53 = 8e-4 in the step and
# to 2e-6 in the cost -- measured on the device, and no statement about either.  That run therefore keeps mu in [1e-2, 1e4] px^2
# (cond <= 1.2e8: 1.3e-8 in the step; tests/test_ba_trust_region_ref_host.py asserts both condition numbers on the numpy matrix), the damping a caller working in pixels would choose; the other three run at the defaults.
DL_ITERS = 12
HISTORY_CASES = {
    "selfcal-huber-scaled": ("ba6x40_selfcal", True, True),
    "selfcal-huber-plain": ("ba6x40_selfcal", True, False),
    "ba-noloss-scaled": ("ba6x40_ba", False, True),
    "ba-noloss-plain": ("ba6x40_ba", False, False),
}
RADIUS0 = {"selfcal-huber-scaled": 0.5, "selfcal-huber-plain": 0.5, "ba-noloss-scaled": 0.5, "ba-noloss-plain": 0.5}
MU = {"ba-noloss-plain": dict(initial_mu=1.0, min_mu=1e-2, max_mu=1e4)}


def history_problem(case):
    name, with_loss, scaling = HISTORY_CASES[case]
    d, opt, delta, _ = golden_data(name)
    return BaProblem(d, opt, huber(delta) if with_loss else None, gauge(d)), scaling


@functools.lru_cache(maxsize=None)
def dogleg_reference(case):
    P, scaling = history_problem(case)
    mu = MU.get(case, {})
    _, _, _, _, _, p_c = first_linearisation(P, scaling, mu.get("initial_mu", 1e-4))
    P.scaling = None
    radius0 = RADIUS0[case] * float(np.linalg.norm(p_c))
    out = tr.dog_leg(P, trust_region_radius=radius0, use_jacobi_scaling=scaling, max_iterations=DL_ITERS, **mu)
    out["radius0"] = radius0
    return out
