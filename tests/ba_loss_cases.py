"""The bundle-adjustment problem and the losses that the BA robust-loss tests share (tests/test_ba_loss_ref_host.py on the
CPU, tests/test_gpu_ba_loss.py on the device) -- TEST INFRASTRUCTURE ONLY.

problem(): make_problem(12, 400, 3, 6) with a fifth of the observations shifted by tens of pixels -- one observation each of
landmarks spread over the set, so that a redescending loss which cuts them leaves every landmark at least two -- and a
handful of measurements put ON the projection of the initial parameters (s below f64::EPSILON: the L2 fall-backs of L1,
Fair and Lp).  Scales that have a threshold sit strictly between two neighbouring residual norms (scale_between, as
loss_graphs.scale_between)."""
from __future__ import annotations

import numpy as np

import apex_solver_amd as pkg
import np_ref
import np_ref_ba_loss as nb
import np_ref_loss as nl
from apex_solver_amd import capi
from apex_solver_amd.loss import Loss, create_loss_function
from apex_solver_amd.synthetic import BAProblemData

CONFIG_ID = 412
SEED = 7


def with_outliers(d, seed=SEED, exact=8):
    rng = np.random.default_rng(seed)
    uv = d.obs_uv.copy()
    pt = d.pt_idx.astype(int)
    first = np.unique(pt, return_index=True)[1]          # one observation per landmark
    n_out = d.n_obs // 5
    chosen = rng.permutation(first)[:min(n_out, len(first))]
    ang = rng.uniform(0.0, 2 * np.pi, len(chosen))
    mag = rng.uniform(20.0, 60.0, len(chosen))
    uv[chosen] += np.stack([mag * np.cos(ang), mag * np.sin(ang)], -1)
    # a few measurements on the projection itself: residuals of rounding size
    rest = np.setdiff1d(np.arange(d.n_obs), chosen)
    on = rng.permutation(rest)[:exact]
    proj = np_ref.project(d.poses, d.intr, d.points, d.cam_idx.astype(int), pt)[0]
    uv[on] = proj[on]
    uv[on[: exact // 2], 0] += 1e-9
    return BAProblemData(poses=d.poses, intr=d.intr, points=d.points, cam_idx=d.cam_idx, pt_idx=d.pt_idx, obs_uv=uv, name=d.name), chosen


def problem():
    d = pkg.synthetic.make_problem(12, 400, 3, 6, config_id=CONFIG_ID)
    return with_outliers(d)[0]


def raw_residuals(d):
    return np_ref.residuals(d.poses, d.intr, d.points, d.cam_idx.astype(int), d.pt_idx.astype(int), d.obs_uv, huber_delta=0)[0]


def scale_between(r, q):
    """a scale strictly between two neighbouring residual norms at quantile q: observations on both sides, none near it"""
    x = np.sort(np.sqrt(nb.squared_norms(r)))
    k = int(q * (len(x) - 1))
    while x[k + 1] - x[k] < 1e-4 * x[k + 1]:
        k += 1
    return 0.5 * (x[k] + x[k + 1])


# every name create_loss_function knows whose loss bundle adjustment accepts (andrews is refused; lp's default p is 1.5)
SWEEP = ("l2", "l1", "huber", "cauchy", "fair", "welsch", "tukey", "geman", "ramsay", "trimmed", "lp", "barron0", "barron1",
         "barron-2", "t-distribution", "adaptive-barron")
REFUSED = {"andrews": Loss(capi.LOSS_ANDREWS, 1.339), "lp3": Loss(capi.LOSS_LP_NORM, 3.0), "barron3": Loss(capi.LOSS_BARRON, 3.0, 1.0)}


def sweep_losses(r):
    """name -> Loss; Huber, Tukey and the trimmed mean change branch at residual quantiles of this problem, the smooth kinds take
    scales of the size of the inlier residuals (the defaults of the names are tuned to whitened residuals, not to pixels)"""
    out = {}
    for name in SWEEP:
        if name == "huber":
            out[name] = create_loss_function(name, scale_between(r, 0.5))
        elif name == "tukey":
            out[name] = create_loss_function(name, scale_between(r, 0.85))
        elif name == "trimmed":
            out[name] = create_loss_function(name, scale_between(r, 0.9))
        elif name in ("l2", "l1", "lp", "t-distribution"):
            out[name] = create_loss_function(name)
        elif name == "ramsay":
            out[name] = create_loss_function(name, 0.3)
        else:
            out[name] = create_loss_function(name, scale_between(r, 0.6))
    return out


def check_conditions(name, loss, d):
    """The facts the tests rely on, asserted on the numpy reference alone: both sides of every branch of the loss are populated,
    no s lies within a relative 1e-6 of a threshold, and for Tukey and the trimmed mean some rho' = 0 while every landmark keeps
    at least two observations with rho' > 0.  Returns (s, rho')."""
    r = raw_residuals(d)
    s = nb.squared_norms(r)
    for t in nl.thresholds(loss):
        assert (s < t).sum() >= 2 and (s > t).sum() >= 2, (name, t, (s < t).sum(), (s > t).sum())
    assert nl.threshold_margin(loss, s) > 1e-6, (name, nl.threshold_margin(loss, s))
    rho1 = np.array([float(nl.evaluate(loss, x)[1]) for x in s])
    arms = np.array([nl.corrector(loss, x)[3] for x in s])
    assert (arms == 1).all(), name
    if name in ("tukey", "trimmed"):
        kept = np.bincount(d.pt_idx.astype(int), weights=(rho1 > 0).astype(float), minlength=d.n_pt)
        assert (rho1 == 0.0).sum() >= 10 and kept.min() >= 2, (name, (rho1 == 0.0).sum(), kept.min())
    return s, rho1
