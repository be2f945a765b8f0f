"""Bundle adjustment with PriorFactor blocks on camera poses and intrinsics, in numpy -- TEST INFRASTRUCTURE ONLY.

np_ref.py's sparse Jacobian and residual (through np_ref_ba_tr.BaProblem: losses, masks, modes) with the prior rows appended
behind the observations' (src/factors/prior_factor.rs:93-105, src/linearizer/cpu/sparse.rs:201-204):

  pose prior on camera c, data [tx,ty,tz,qw,qx,qy,qz]   r = w (to_vector(pose_c) - data) over the normalised pose, seven rows;
                                                        J = w I7 truncated to the pose's six tangent columns: row a < 6 has the
                                                        one entry w at column pose_col[c] + a, the seventh row has none
  intrinsics prior on camera c, data [f,k1,k2]          r = w (intr_c - data), J = w I3 at intr_col[c]
  the block's Huber delta (None / <= 0: none)           s = |r|^2 over all rows of the block (w included); where s > delta^2 both r
                                                        and J are scaled by sqrt(rho') = sqrt(delta / sqrt(s)) (the corrector's first arm)

From the augmented (r~, J~) everything else follows as it does without priors: np_ref.direct_step, np_ref.schur_dense, the
cost, the gradient, the jv-Gram sums and the column norms; PriorBaProblem is a BaProblem, so np_ref_trust_region's loops run on it.
"""
from __future__ import annotations

import numpy as np
import scipy.sparse as sp

import np_ref_ba_tr as bt


def _rows(priors, amb):
    """(cam [n], data [n][amb], delta [n] (<= 0: none), w [n]) of a list of (cam, data, huber delta or None, weight)"""
    cam = np.array([q[0] for q in priors], dtype=np.int64).reshape(-1)
    data = np.array([q[1] for q in priors], dtype=np.float64).reshape(-1, amb)
    delta = np.array([-1.0 if q[2] is None else q[2] for q in priors], dtype=np.float64).reshape(-1)
    w = np.array([q[3] for q in priors], dtype=np.float64).reshape(-1)
    return cam, data, delta, w


def huber_scale(delta, s):
    """sqrt(rho') of a block with squared norm s"""
    out = (delta > 0) & (s > delta * delta)
    return np.where(out, np.sqrt(np.where(out, delta, 1.0) / np.sqrt(np.where(out, s, 1.0))), 1.0)


def pose_vector(poses):
    """to_vector of the poses the kernels see: translation, then the normalised quaternion"""
    q = poses[:, 3:7] / np.linalg.norm(poses[:, 3:7], axis=1, keepdims=True)
    q = q / np.linalg.norm(q, axis=1, keepdims=True)
    return np.concatenate([poses[:, 0:3], q], axis=1)


def prior_blocks(x, priors, amb):
    """corrected residuals [n][amb] and the blocks' Jacobian scale sqrt(rho') w [n]; x [n_cam][amb] the variables' vectors"""
    cam, data, delta, w = _rows(priors, amb)
    r = w[:, None] * (x[cam] - data)
    sc = huber_scale(delta, np.sum(r * r, axis=1))
    return r * sc[:, None], sc * w, cam


def prior_system(poses, intr, pose_priors, intr_priors, lay):
    """(r~ [7 n_pose + 3 n_intr], J~ sparse over lay.total_dof columns): pose blocks first, each set in list order"""
    rp, jp, cp = prior_blocks(pose_vector(poses), pose_priors, 7)
    ri, ji, ci = prior_blocks(intr, intr_priors, 3)
    rows, cols, vals = [], [], []
    for k in range(len(cp)):
        for a in range(6):   # the seventh row has no column
            rows.append(7 * k + a); cols.append(lay.pose_col[cp[k]] + a); vals.append(jp[k])
    for k in range(len(ci)):
        for a in range(3):
            rows.append(7 * len(cp) + 3 * k + a); cols.append(lay.intr_col[ci[k]] + a); vals.append(ji[k])
    n_rows = 7 * len(cp) + 3 * len(ci)
    J = sp.csc_matrix((vals, (rows, cols)), shape=(n_rows, lay.total_dof))
    return np.concatenate([rp.ravel(), ri.ravel()]), J


class PriorBaProblem(bt.BaProblem):
    """BaProblem plus prior lists: (camera, data, huber delta or None, weight) each"""

    def __init__(self, d, opt=bt.OptimizationType.SelfCalibration, loss=None, masks=None, params=None, pose_priors=(), intr_priors=()):
        super().__init__(d, opt, loss, masks, params)
        self.pose_priors, self.intr_priors = list(pose_priors), list(intr_priors)
        assert self.selfcal or not self.intr_priors, "intrinsics priors need the intrinsics' columns"

    def prior_residuals(self):
        rp = prior_blocks(pose_vector(self.params[0]), self.pose_priors, 7)[0]
        ri = prior_blocks(self.params[1], self.intr_priors, 3)[0]
        return rp, ri

    def jacobian(self):
        r, J = super().jacobian()
        if not self.pose_priors and not self.intr_priors:
            return r, J
        rp, Jp = prior_system(self.params[0], self.params[1], self.pose_priors, self.intr_priors, self.lay)
        return np.concatenate([r, rp]), sp.vstack([J, Jp]).tocsc()

    def cost(self):
        c = super().cost()
        rp, ri = self.prior_residuals()
        nrm = np.sqrt(2.0 * c + np.sum(rp * rp) + np.sum(ri * ri))
        return 0.5 * nrm * nrm

    def device_problem(self):
        p = bt.device_problem(self)
        p.pose_priors, p.intr_priors = list(self.pose_priors), list(self.intr_priors)
        return p

    # what the device exports, from (r~, J~)
    def gradient(self):
        r, J = self.jacobian()
        return J.T @ r

    def column_norms(self):
        _, J = self.jacobian()
        return np.sqrt(np.asarray(J.multiply(J).sum(axis=0)).ravel())

    def jv_gram(self, a, b):
        _, J = self.jacobian()
        u, w = J @ a, J @ b
        return np.array([u @ u, u @ w, w @ w]), u, w


def camera_blocks_agree(H_dev, H_ref, lay, cams, tol=1e-12):
    """the block check of the device tests: the 9 x 9 (pose, intrinsics) diagonal blocks of the given cameras, relative to the
    block's largest entry"""
    for c in cams:
        idx = np.concatenate([lay.pose_col[c] + np.arange(6), lay.intr_col[c] + np.arange(3)])
        A, B = H_dev[np.ix_(idx, idx)], H_ref[np.ix_(idx, idx)]
        if not np.abs(A - B).max() <= tol * max(np.abs(B).max(), 1e-300):
            return False
    return True


def lm(P, iterations, damping=1e-3, damping_min=1e-12, damping_max=1e12):
    """np_ref_ba_loss.lm's loop (LevenbergMarquardt::optimize without scaling and without a convergence test) on a problem
    object: history rows cost, damping, rho, accepted, |g|, |step|, predicted, trial cost.  P is moved to the final point."""
    lam, nu = damping, 2.0
    c = P.cost()
    hist = []
    for _ in range(iterations):
        H, g = P.normal_equations()
        y = np.linalg.solve(H + lam * np.eye(P.n), -g)
        gn, sn = float(np.sqrt(g @ g)), float(np.sqrt(y @ y))
        pred = 0.5 * float(np.sum(y * (lam * y - g)))
        P.apply_step(y)
        new_cost = P.cost()
        actual = c - new_cost
        rho = (1.0 if actual > 0 else 0.0) if abs(pred) < 1e-15 else actual / pred
        if rho > 0:
            lam = max(lam * max(1.0 / 3.0, 1 - (2 * rho - 1) ** 3), damping_min)
            nu = 2.0; accepted = 1
            c = new_cost
        else:
            P.apply_step(y, sign=-1.0)
            lam = min(lam * nu, damping_max); nu *= 2; accepted = 0
        hist.append([c, lam, rho, accepted, gn, sn, pred, new_cost])
    return np.array(hist).reshape(-1, 8)
