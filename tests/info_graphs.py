"""The graphs and edge information matrices the information tests share (tests/test_info_device_math_host.py and
tests/test_info_api_host.py on the CPU, tests/test_gpu_pg_information.py on the device) -- TEST INFRASTRUCTURE ONLY.

graph(manifold, n, jitter): loss_graphs.graph with every seventh edge turned round (from and to exchanged, the measurement
inverted: the same constraint), so that the caller's edge list has edges with from < to, edges with
from > to and the self-loop -- the three cases of the cross block.

information(d): one Omega per edge of such a graph, Q diag(sigma) Q^T with a random rotation Q per edge and sigma
log-uniform in [0.25, 4]: dense, different from edge to edge, nowhere near a multiple of I -- a cross block assembled as
J_lo^T Omega J_hi instead of J_hi^T Omega J_lo is then wrong in its leading digits, not in its last ones."""
from __future__ import annotations

import numpy as np

import apex_solver_amd as pkg
import loss_graphs as lg

# The range was [0.25, 16] at first.  With it the Lp(3) system of the SE3 graph (rho' grows like sqrt(s): the outliers weigh most) is
# conditioned so that numpy's own fp64 solve is 2e-11 from the long-double solve at lambda = 1e-3, above the 1e-11 that the device
# tests' 1e-10 step bound presumes (tests/test_info_device_math_host.py checks it); [0.25, 4] gives 4e-12.
SIGMA_LO, SIGMA_HI = 0.25, 4.0


def _inverse(m):
    """the inverse of measurements in stored form: (n, 3) [x, y, theta] | (n, 7) [t, qw, qx, qy, qz]"""
    m = np.asarray(m, dtype=np.float64)
    o = m.copy()
    if m.shape[1] == 3:
        c, s = np.cos(m[:, 2]), np.sin(m[:, 2])
        o[:, 0] = -(c * m[:, 0] + s * m[:, 1]); o[:, 1] = -(-s * m[:, 0] + c * m[:, 1]); o[:, 2] = -m[:, 2]
        return o
    w, v, t = m[:, 3:4], -m[:, 4:7], m[:, :3]          # conjugate quaternion; R^T t = t + 2 w (v x t) + 2 v x (v x t)
    vt = np.cross(v, t)
    o[:, :3] = -(t + 2.0 * w * vt + 2.0 * np.cross(v, vt))
    o[:, 4:7] = v
    return o


def graph(manifold: str, n: int | None = None, jitter: bool = False):
    d = lg.graph(manifold, n, jitter=jitter)
    ef, et, meas = d.e_from.copy(), d.e_to.copy(), d.meas.copy()
    turn = np.arange(3, d.n_e - 1, 7)   # (the last edge is the self-loop)
    turn = turn[turn % 5 != 2]          # not loss_graphs' gross outliers: Log of the inverted constraint of one is several times longer
    ef[turn], et[turn] = d.e_to[turn], d.e_from[turn]
    meas[turn] = _inverse(d.meas[turn])
    return pkg.synthetic.PoseGraphData(ids=d.ids, poses=d.poses, e_from=ef, e_to=et, meas=meas, name=d.name)


def information(d, seed: int = 11) -> np.ndarray:
    D = 3 if d.manifold == "se2" else 6
    rng = np.random.default_rng(seed)
    out = np.zeros((d.n_e, D, D))
    for e in range(d.n_e):
        Q, R = np.linalg.qr(rng.standard_normal((D, D)))
        Q = Q * np.sign(np.diag(R))[None, :]
        if np.linalg.det(Q) < 0:
            Q[:, 0] = -Q[:, 0]
        sigma = np.exp(rng.uniform(np.log(SIGMA_LO), np.log(SIGMA_HI), D))
        W = (Q * sigma[None, :]) @ Q.T
        out[e] = 0.5 * (W + W.T)   # exactly symmetric: what a handle stores (the upper triangle) is what it was given
    ef, et = d.e_from.astype(np.int64), d.e_to.astype(np.int64)
    # the three cases of the cross block: row vertex = to, row vertex = from, the self-loop
    assert (ef < et).any() and (ef > et).any() and (ef == et).sum() == 1
    mean = np.trace(out, axis1=1, axis2=2) / D
    off = np.abs(out - mean[:, None, None] * np.eye(D)[None]).max(axis=(1, 2)) / mean
    assert off.min() > 1e-3, off.min()
    assert np.array_equal(out, out.transpose(0, 2, 1)) and np.linalg.eigvalsh(out).min() > 0.9 * SIGMA_LO
    out.setflags(write=False)
    return out
