"""Bundle adjustment under the robust loss family, in numpy -- TEST INFRASTRUCTURE ONLY.

np_ref.residuals / jacobian_blocks with huber_delta = 0 give the raw r, J of every observation; np_ref_loss.evaluate /
corrector (extended precision) give the weight.  Only first-arm losses occur here (rho'' <= 0 or s == 0: r~ = sqrt(rho') r,
J~ = sqrt(rho') J); linearize asserts it.  From these: dense H, g, S, g_red, the cost and the damped step through
np_ref.sparse_jacobian, schur_dense and direct_step, and an LM loop like np_ref_loss.lm.

A loss is anything with .kind, .p0, .p1 (apex_solver_amd.loss.Loss); None is no loss.
"""
from __future__ import annotations

import numpy as np

import np_ref
import np_ref_loss as nl
from apex_solver_amd import capi
from apex_solver_amd.loss import Loss

NONE = Loss(capi.LOSS_NONE)


def squared_norms(r):
    """s = |r|^2 of the 2-vector residuals in fp64 (the device forms fma(r0, r0, r1 r1): the last bit may differ, which is why
    the tests keep every s away from the thresholds)"""
    return r[:, 0] * r[:, 0] + r[:, 1] * r[:, 1]


def weights(loss, s):
    """sqrt(rho'(s)) per observation, fp64 from the extended-precision reference; every corrector takes its first arm"""
    loss = loss or NONE
    w = np.empty(len(s))
    for i, si in enumerate(s):
        sq, rs, a, arm = nl.corrector(loss, float(si))
        assert arm == 1 and float(a) == 0.0 and rs == sq, (loss, si)
        w[i] = float(sq)
    return w


def linearize(poses, intr, pts, cam_idx, pt_idx, obs_uv, loss):
    """(r~, Jpose~, Jpt~, Jintr~, s, w): corrected blocks, the raw squared norms and the weights"""
    r, _, Jp, Jl, Ji = np_ref.jacobian_blocks(poses, intr, pts, cam_idx, pt_idx, obs_uv, huber_delta=0)
    s = squared_norms(r)
    w = weights(loss, s)
    return r * w[:, None], Jp * w[:, None, None], Jl * w[:, None, None], Ji * w[:, None, None], s, w


def cost(poses, intr, pts, cam_idx, pt_idx, obs_uv, loss):
    r = np_ref.residuals(poses, intr, pts, cam_idx, pt_idx, obs_uv, huber_delta=0)[0]
    rt = r * weights(loss, squared_norms(r))[:, None]
    return 0.5 * float(np.sum(rt * rt))


class System:
    """everything the parity tests compare, at one parameter set.  selfcal: the intrinsics have columns (d_c = 9).  flags:
    (POSE, LANDMARK, INTRINSIC) of OptimizeParams -- a block that is not optimised has zero columns."""

    def __init__(self, d, lay, loss, selfcal, params=None, flags=(1, 1, 1)):
        poses, intr, pts = params if params is not None else (d.poses, d.intr, d.points)
        ci, pi = d.cam_idx.astype(int), d.pt_idx.astype(int)
        self.r, self.Jp, self.Jl, self.Ji, self.s, self.w = linearize(poses, intr, pts, ci, pi, d.obs_uv, loss)
        self.Jp, self.Jl, self.Ji = self.Jp * flags[0], self.Jl * flags[1], self.Ji * (flags[2] if selfcal else 0)
        self.J = np_ref.sparse_jacobian(self.Jp, self.Jl, self.Ji, ci, pi, lay, selfcal=selfcal)
        self.lay, self.nc = lay, lay.cam_dof
        self.cost = 0.5 * float(np.sum(self.r * self.r))
        self.H = (self.J.T @ self.J).toarray()
        self.g = self.J.T @ self.r.ravel()

    def schur(self, lam):
        return np_ref.schur_dense(self.H, self.g, self.nc, lam)

    def step(self, lam):
        return np.linalg.solve(self.H + lam * np.eye(self.H.shape[0]), -self.g)

    def column_norms(self):
        return np.sqrt(np.asarray(self.J.multiply(self.J).sum(axis=0)).ravel())


def lm(d, lay, loss, selfcal, fix_pose, iterations, damping=1e-3, damping_min=1e-12, damping_max=1e12):
    """LevenbergMarquardt::optimize without scaling and without a convergence test, `iterations` times: the update rule of
    np_ref_loss.lm.  history rows: cost, damping, rho, accepted, |g|, |step|, predicted, trial cost; margins: |rho| of every
    iteration (the accept / reject decision is rho > 0) for the caller to assert away from 0."""
    params = (d.poses.copy(), d.intr.copy(), d.points.copy())
    ci, pi = d.cam_idx.astype(int), d.pt_idx.astype(int)
    lam, nu = damping, 2.0
    c = cost(*params, ci, pi, d.obs_uv, loss)
    hist = []
    for _ in range(iterations):
        P = System(d, lay, loss, selfcal, params)
        y = P.step(lam)
        gn, sn = float(np.sqrt(P.g @ P.g)), float(np.sqrt(y @ y))
        pred = 0.5 * float(np.sum(y * (lam * y - P.g)))
        trial = np_ref.retract(*params, y, lay, fix_pose=fix_pose)
        new_cost = cost(*trial, ci, pi, d.obs_uv, loss)
        actual = c - new_cost
        rho = (1.0 if actual > 0 else 0.0) if abs(pred) < 1e-15 else actual / pred
        if rho > 0:
            lam = max(lam * max(1.0 / 3.0, 1 - (2 * rho - 1) ** 3), damping_min)
            nu = 2.0; accepted = 1
            c = new_cost; params = trial
        else:
            lam = min(lam * nu, damping_max); nu *= 2; accepted = 0
        hist.append([c, lam, rho, accepted, gn, sn, pred, new_cost])
    return np.array(hist).reshape(-1, 8), params
