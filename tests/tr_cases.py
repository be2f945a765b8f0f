"""Inputs shared by tests/test_trust_region_np_ref.py (CPU: the premises, on the numpy loops alone) and
tests/test_gpu_trust_region.py (device): ~60-vertex SE2 and SE3 pose graphs with a prior gauge and a noisy start, and the numpy
Dog-Leg / Gauss-Newton runs on them, computed once per process."""
import functools

import numpy as np
from scipy.spatial.transform import Rotation

import apex_solver_amd as pkg
import np_ref_pg
import np_ref_se2 as ref2
import np_ref_trust_region as tr
from apex_solver_amd.pose_graph import PoseGraphProblem

# (noise, seed) chosen by running the numpy loop alone: the unscaled run from half the Cauchy radius shows all three step types, a
# rejection followed by a reuse and a good-step growth of the radius, with every decision >= 1e-2 relative from its threshold
START = {"se2": (1.5, 6), "se3": (0.1, 2)}
DL_ITERS = 25


def noisy_start(d, noise, seed):
    rng = np.random.default_rng(seed)
    p = d.poses.copy()
    if p.shape[1] == 3:
        return p + noise * rng.normal(size=p.shape)
    p[:, :3] += noise * rng.normal(size=(p.shape[0], 3))
    q = p[:, 3:7] + 0.2 * noise * rng.normal(size=(p.shape[0], 4))
    p[:, 3:7] = q / np.linalg.norm(q, axis=1, keepdims=True)
    return p


def graph(man):
    return pkg.synthetic.make_manhattan(60) if man == "se2" else pkg.synthetic.make_sphere(6, 10)


def problem(man, fix=None):
    """(PoseGraphProblem with a prior on the first vertex as its gauge, noisy start)"""
    d = graph(man)
    prob = PoseGraphProblem(d).add_prior(f"x{int(d.ids[0])}")
    if fix is not None:
        prob.fix[:] = fix
    return prob, noisy_start(d, *START[man])


def numpy_problem(prob, poses):
    return (ref2.Problem if prob.manifold == "se2" else tr.Se3Problem).from_problem(prob, poses)


def first_linearisation(prob, poses, scaling, mu):
    """H, g (scaled variables), D (or None), h, alpha, p_c at the start"""
    P = numpy_problem(prob, poses)
    tr._init_scaling(P, scaling)
    H, g = P.normal_equations()
    h = tr.solve_damped(H, g, mu)
    alpha, p_c = tr.cauchy_point(H, g)
    return P, H, g, P.scaling, h, alpha, p_c


@functools.lru_cache(maxsize=None)
def dogleg_reference(man, scaling):
    prob, p0 = problem(man)
    _, _, _, _, _, _, p_c = first_linearisation(prob, p0, scaling, 1e-4)
    radius0 = 0.5 * float(np.linalg.norm(p_c))
    out = tr.dog_leg(numpy_problem(prob, p0), trust_region_radius=radius0, use_jacobi_scaling=scaling, max_iterations=DL_ITERS)
    out["radius0"] = radius0
    return out


@functools.lru_cache(maxsize=None)
def gauss_newton_reference(man, scaling):
    prob, _ = problem(man)
    p0 = noisy_start(prob.data, 0.05, 3)   # (Gauss-Newton has no globalisation: a start it converges from)
    # (six iterations: on SE3 the undamped iteration with the reference's Jacobians, as coded, stops descending near the minimum and then
    # climbs by a factor of 3 to 4 per step, which would amplify any rounding difference with it)
    out = tr.gauss_newton(numpy_problem(prob, p0), use_jacobi_scaling=scaling, max_iterations=6)
    out["start"] = p0
    return out


# ---- the applied step, read back from two parameter sets: new = old (+) step ---------------------------------------------------
def applied_step(prob, old, new):
    n_v, dof = old.shape[0], prob.dof
    out = np.zeros(dof * n_v)
    for v in range(n_v):
        if dof == 3:
            t = ref2.minus(new[v], old[v])
        else:
            R0, t0 = np_ref_pg.to_Rt(old[v]); R1, t1 = np_ref_pg.to_Rt(new[v])
            th = Rotation.from_matrix(R0.T @ R1).as_rotvec()
            t = np.concatenate([np.linalg.solve(np_ref_pg.so3_left_jacobian(th), R0.T @ (t1 - t0)), th])
        out[prob.pose_col[v]:prob.pose_col[v] + dof] = t
    return out


def mask_vector(prob):
    m = np.zeros(prob.dof * prob.data.n_v, bool)
    for v in range(prob.data.n_v):
        m[prob.pose_col[v]:prob.pose_col[v] + prob.dof] = prob.fix[v].astype(bool)
    return m
