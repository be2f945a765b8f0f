"""The graphs and losses the robust-loss tests share (tests/test_loss_device_math_host.py on the CPU,
tests/test_gpu_pg_loss.py on the device) -- TEST INFRASTRUCTURE ONLY.

graph(manifold, n): make_sphere(8, 12) | make_manhattan(n) with every fifth edge's measurement moved far away (gross
outliers: residual norms of several units) and one self-loop edge appended.  The generators start from the odometry chain,
so their odometry edges have residuals of rounding size (s < f64::EPSILON: the L2 fall-backs and the s ~ 0 end of every
loss), the loop closures carry the drift, the outliers sit beyond the redescending losses' thresholds."""
from __future__ import annotations

import numpy as np

import apex_solver_amd as pkg
import np_ref_loss as nl
import np_ref_pg
import np_ref_se2
from apex_solver_amd import capi
from apex_solver_amd.pose_graph import Loss, create_loss_function


def graph(manifold: str, n: int | None = None, jitter: bool = False):
    """jitter: the poses are moved by 1e-3 so that no residual is of rounding size.  For Andrews' wave: its rho'(s) -> 0 like
    sqrt(s) and its corrector's alpha / s grows like 1 / s, so on a residual of 1e-16 -- whose digits are rounding noise of
    whoever computed it -- the literal J~ is noise times 1e-9; H, g and the cost do not see it, an entry-wise comparison of
    J~ would."""
    d = pkg.synthetic.make_manhattan(n or 120) if manifold == "se2" else pkg.synthetic.make_sphere(8, 12)
    rng = np.random.default_rng(5)
    if jitter:
        poses = d.poses + 1e-3 * rng.standard_normal(d.poses.shape)
        if manifold == "se3":
            poses[:, 3:7] /= np.linalg.norm(poses[:, 3:7], axis=1, keepdims=True)
        d = pkg.synthetic.PoseGraphData(ids=d.ids, poses=poses, e_from=d.e_from, e_to=d.e_to, meas=d.meas, name=d.name)
    meas = d.meas.copy()
    out = np.arange(2, d.n_e, 5)
    if manifold == "se2":
        meas[out, :2] += rng.normal(0.0, 2.5, (len(out), 2))
        meas[out, 2] += rng.uniform(0.5, 2.0, len(out)) * rng.choice([-1.0, 1.0], len(out))
        loop = np.array([[0.3, -0.2, 0.4]])
    else:
        meas[out, :3] += rng.normal(0.0, 2.5, (len(out), 3))
        q = meas[out, 3:7] + rng.normal(0.0, 0.6, (len(out), 4))
        meas[out, 3:7] = q / np.linalg.norm(q, axis=1, keepdims=True)
        loop = np.array([[0.3, -0.2, 0.4, 0.9, 0.1, -0.3, 0.2]])
        loop[0, 3:7] /= np.linalg.norm(loop[0, 3:7])
    v = np.uint32(d.n_v // 2)
    return pkg.synthetic.PoseGraphData(ids=d.ids, poses=d.poses, e_from=np.append(d.e_from, v).astype(np.uint32),
                                       e_to=np.append(d.e_to, v).astype(np.uint32), meas=np.vstack([meas, loop]), name=d.name)


def linearize(d):
    """uncorrected (r, J) of every edge by the numpy references"""
    if d.manifold == "se2":
        P = np.array(d.poses, dtype=np.float64)
        P[:, 2] = np_ref_se2.wrap(P[:, 2])   # the variable is held wrapped (se2.rs:55-63)
        return np_ref_se2.between_linearize(P[d.e_from.astype(int)], P[d.e_to.astype(int)], d.meas)
    return np_ref_pg.linearize(d.poses, d.e_from.astype(int), d.e_to.astype(int), d.meas, None)


def squared_norms(r):
    s = np.zeros(len(r))
    for x in r.T:
        s = s + x * x
    return s


def scale_between(r, q):
    """a scale strictly between two neighbouring residual norms at quantile q: edges on both sides, none near it"""
    x = np.sort(np.sqrt(squared_norms(r)))
    k = int(q * (len(x) - 1))
    while x[k + 1] - x[k] < 1e-6 * x[k + 1]:
        k += 1
    return 0.5 * (x[k] + x[k + 1])


def sweep_losses(r):
    """name -> Loss of the parity sweep; Tukey and the trimmed mean cut at residual quantiles of this graph"""
    return {
        "cauchy": create_loss_function("cauchy"), "tukey": create_loss_function("tukey", scale_between(r, 0.8)),
        "andrews": create_loss_function("andrews"), "lp3": create_loss_function("lp", 3.0),
        "barron1": create_loss_function("barron1"), "barron-2": create_loss_function("barron-2"),
        "t-distribution": create_loss_function("t-distribution"), "welsch": create_loss_function("welsch"),
        "fair": create_loss_function("fair"), "l1": create_loss_function("l1"),
        "trimmed": create_loss_function("trimmed", scale_between(r, 0.7)),
    }


def needs_jitter(name):
    return name == "andrews"


SWEEP = ("cauchy", "tukey", "andrews", "lp3", "barron1", "barron-2", "t-distribution", "welsch", "fair", "l1", "trimmed")


def check_conditions(name, loss, r):
    """The conditions the tests assert on the reference's values: no s within 1e-9 (relative) of a branch threshold; Andrews
    (default scale) and Lp(3) have ten edges in each arm; Tukey and the trimmed mean have an edge with rho' = 0."""
    ss = squared_norms(r)
    assert nl.threshold_margin(loss, ss) > 1e-9, (name, nl.threshold_margin(loss, ss))
    arms = np.array([nl.corrector(loss, s)[3] for s in ss])
    rho1 = np.array([float(nl.evaluate(loss, s)[1]) for s in ss])
    if name in ("andrews", "lp3"):
        assert (arms == 1).sum() >= 10 and (arms == 2).sum() >= 10, (name, (arms == 1).sum(), (arms == 2).sum())
    if name in ("tukey", "trimmed"):
        assert (rho1 == 0.0).sum() >= 1 and (rho1 > 0.0).sum() >= 1, name
    return arms, rho1
