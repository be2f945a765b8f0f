"""Edge information matrices restated in numpy -- TEST INFRASTRUCTURE ONLY.

Omega = U^T U with U = np.linalg.cholesky(Omega).T.  The uncorrected (r, J) of loss_graphs.linearize are whitened,
r_w = U r, J_w = U J, and handed to the corrector of np_ref_loss unchanged (whiten, then robustify).  H, g and the cost are
J~^T J~, J~^T r~ and 1/2 |r~|^2 of the literal corrected blocks, accumulated in np.longdouble.

The problems below have the interface np_ref_trust_region's loops take."""
from __future__ import annotations

from types import SimpleNamespace

import numpy as np

import np_ref_loss as nl
import np_ref_pg
import np_ref_se2
from apex_solver_amd import capi

LD = np.longdouble
NO_LOSS = SimpleNamespace(kind=capi.LOSS_NONE, p0=0.0, p1=0.0)


def loss_of(prob):
    """the loss of a PoseGraphProblem as np_ref_loss takes it"""
    if prob.loss is not None:
        return prob.loss
    if prob.huber_delta is not None and prob.huber_delta > 0:
        return SimpleNamespace(kind=capi.LOSS_HUBER, p0=float(prob.huber_delta), p1=0.0)
    return NO_LOSS


def whiten(r, J, info):
    """(U r, U J) of every edge, fp64"""
    rw = np.zeros_like(r); Jw = np.zeros_like(J)
    for e in range(len(r)):
        U = np.linalg.cholesky(info[e]).T
        rw[e] = U @ r[e]; Jw[e] = U @ J[e]
    return rw, Jw


def corrected_edges(r, J, info, loss):
    """uncorrected r (n, D), J (n, D, 2 D) -> whitened and corrected fp64 (r~, J~), the arm and s of every edge"""
    rw, Jw = whiten(r, J, info)
    return nl.correct_edges(rw, Jw, loss)


class _Weighted:
    """edge_blocks through the whitening; H, g, cost accumulated in long double"""
    information = None
    long_double = True   # False: plain fp64 products (the optimiser loops, whose bounds are 1e-7)

    def cost(self):
        r, _ = self.edge_blocks()
        pr, _ = self.prior_blocks()
        return float(LD(0.5) * (np.sum(r.astype(LD) ** 2) + np.sum(pr.astype(LD) ** 2)))

    def normal_equations(self):
        r, J = self.jacobian()
        if self.scaling is not None:
            J = J * self.scaling[None, :]
        if not self.long_double:
            return J.T @ J, J.T @ r
        Jl, rl = J.astype(LD), r.astype(LD)
        return (Jl.T @ Jl).astype(np.float64), (Jl.T @ rl).astype(np.float64)


class Se3InfoProblem(_Weighted, nl.Se3LossProblem):
    @classmethod
    def from_problem(cls, prob, poses=None):
        d = prob.data
        p = cls(d.poses if poses is None else poses, d.e_from, d.e_to, d.meas, prob.pose_col, prob.fix, None, prob.priors, loss=loss_of(prob))
        p.information = prob.information
        return p

    def edge_blocks(self):
        r, J = np_ref_pg.linearize(self.poses, self.e_from, self.e_to, self.meas, None)
        r, J, self.arms, self.s = corrected_edges(r, J, self.information, self.loss)
        return r, J


class Se2InfoProblem(_Weighted, nl.Se2LossProblem):
    @classmethod
    def from_problem(cls, prob, poses=None):
        d = prob.data
        p = cls(d.poses if poses is None else poses, d.e_from, d.e_to, d.meas, prob.pose_col, prob.fix, None, list(prob.priors))
        p.loss = loss_of(prob)
        p.information = prob.information
        return p

    def edge_blocks(self):
        r, J = np_ref_se2.between_linearize(self.poses[self.e_from], self.poses[self.e_to], self.meas)
        r, J, self.arms, self.s = corrected_edges(r, J, self.information, self.loss)
        return r, J


def numpy_problem(prob, poses=None):
    return (Se2InfoProblem if prob.manifold == "se2" else Se3InfoProblem).from_problem(prob, poses)


def solve_damped_ld(H, g, mu):
    """(H + mu I) h = -g by a Cholesky factorisation carried out in long double"""
    n = H.shape[0]
    A = H.astype(LD) + LD(mu) * np.eye(n, dtype=LD)
    L = np.zeros((n, n), dtype=LD)
    for j in range(n):
        L[j, j] = np.sqrt(A[j, j] - L[j, :j] @ L[j, :j])
        L[j + 1:, j] = (A[j + 1:, j] - L[j + 1:, :j] @ L[j, :j]) / L[j, j]
    y = np.zeros(n, dtype=LD)
    b = -g.astype(LD)
    for i in range(n):
        y[i] = (b[i] - L[i, :i] @ y[:i]) / L[i, i]
    x = np.zeros(n, dtype=LD)
    for i in range(n - 1, -1, -1):
        x[i] = (y[i] - L[i + 1:, i] @ x[i + 1:]) / L[i, i]
    return x
