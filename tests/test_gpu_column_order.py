"""The permutation between the caller's global column order and the device's internal order (csrc/column_map.h): every problem
is solved twice, once with the standard column layout and once with a scrambled one -- the cameras' pose blocks, their intrinsic
blocks and the landmarks' blocks shuffled among themselves (camera columns stay below 9 n_cam, which get_schur requires); a pose
graph's vertex blocks shuffled.  The device computes the same numbers in the same order both times and only the host scatter at
the boundary differs, so every export is EXACTLY equal after the shuffle is undone: step and gradient of solve_augmented, step
and gradient under a column scaling (a given vector), get_schur / get_hessian, jv_gram, the covariance blocks, a pose graph's
column norms.  Six-column cameras (plain bundle adjustment): their intrinsic columns of step, gradient and norms are exactly 0.

One export is not reproducible from run to run on ANY layout, so it cannot be bitwise equal between two handles: the column norms
of bundle adjustment.  k_column_norms_sq (ba_kernels.hip) sums the observations of a column with floating-point atomicAdd, in
whatever order the hardware serves them (measured on the commit before the column map, 6 cameras / 60 points: the same layout
solved twice differs in 16 to 31 of the 234 norms by up to 4.4e-16 relative, and so do the two layouts; every other export of
this file, and all of a pose graph's, came out bit for bit the same in every repetition).  A sum of k non-negative terms in two orders differs by at most 2 (k - 1) u relative (u = 2^-53), its square
root by half of that plus one rounding each: |a - b| <= k eps |a| with eps = 2^-52, and k <= n_obs.  That is the bound here -- it
comes from the number format, not from a run; a norm in a wrong column would miss it by orders of magnitude (the test also
holds the norms pairwise further apart than the bound) -- and the zero columns of six-column cameras stay exact.

set_jacobi_scaling is reachable through the C ABI only from inside lm_optimize (use_jacobi_scaling), which switches it off again
before it returns and exports nothing in the caller's columns on the way: the LM tests of the suite run it."""
import numpy as np
import pytest

import apex_solver_amd as pkg
from apex_solver_amd.layout import ColumnLayout
from apex_solver_amd.pose_graph import GpuSparseCholeskySolver, PoseGraphProblem
from apex_solver_amd.solver import GpuSchurComplementSolver, OptimizationType, Problem

pytestmark = pytest.mark.gpu
LAM = 1e-1
N_CAM, N_PT, N_V = 6, 60, 12


def shuffled(n, seed):
    p = np.random.default_rng(seed).permutation(n)
    assert not np.array_equal(p, np.arange(n))
    return p.astype(np.int64)


# ---- bundle adjustment ---------------------------------------------------------------------------------------------------
def ba_problem(mode, scramble):
    d = pkg.synthetic.make_problem(N_CAM, N_PT, 3, 6, config_id=3)
    prob = Problem.bundle_adjustment(d, mode, 1.0)
    if scramble:
        prob.layout = ColumnLayout(intr_col=3 * shuffled(N_CAM, 11), pose_col=3 * N_CAM + 6 * shuffled(N_CAM, 12),
                                   pt_col=9 * N_CAM + 3 * shuffled(N_PT, 13), cam_dof=9 * N_CAM, total_dof=9 * N_CAM + 3 * N_PT)
    return d, prob


def ba_index(lay):
    """idx with v_standard = v_layout[idx], the standard layout being [intrinsics | poses | landmarks] in the caller's numbering"""
    blocks = [(lay.intr_col, 3), (lay.pose_col, 6), (lay.pt_col, 3)]
    return np.concatenate([(np.asarray(col)[:, None] + np.arange(w)[None, :]).ravel() for col, w in blocks])


def ba_capture(mode, scramble):
    d, prob = ba_problem(mode, scramble)
    idx = ba_index(prob.layout)
    assert np.array_equal(np.sort(idx), np.arange(prob.total_dof))   # a permutation of the columns
    idc = idx[:9 * N_CAM]
    assert idc.max() < 9 * N_CAM
    given = 0.5 + np.random.default_rng(5).random(prob.total_dof)    # in the standard layout
    to_layout = np.empty_like(given)
    s = GpuSchurComplementSolver(0).initialize_structure(prob)
    s.set_parameters(d.poses, d.intr, d.points)
    out = {}
    out["step"] = s.solve_augmented_equation(LAM)[idx]
    out["grad"] = s.get_gradient()[idx]
    out["cam_cov"] = s.camera_covariance_blocks()
    out["norms"] = s.compute_column_norms()[idx]
    S, g = s.get_schur()
    out["S"], out["g_red"] = S[np.ix_(idc, idc)], g[idc]
    to_layout[idx] = given
    s.apply_column_scaling(to_layout)
    out["step_given"] = s.solve_augmented_equation(LAM)[idx]
    out["grad_given"] = s.get_gradient()[idx]
    out["cam_cov_given"] = s.camera_covariance_blocks()
    S, g = s.get_schur()
    out["S_given"], out["g_red_given"] = S[np.ix_(idc, idc)], g[idc]
    out["n_obs"] = np.array(d.n_obs)
    s.close()
    return out


@pytest.fixture(scope="module", params=[OptimizationType.SelfCalibration, OptimizationType.BundleAdjustment], ids=["selfcal_dc9", "ba_dc6"])
def ba_pair(request):
    return request.param, ba_capture(request.param, False), ba_capture(request.param, True)


def test_ba_exports_do_not_depend_on_the_column_layout(ba_pair):
    _, std, scr = ba_pair
    assert std.keys() == scr.keys()
    for k in std:
        if k != "norms":
            assert std[k].shape == scr[k].shape and np.array_equal(std[k], scr[k]), k
    # the atomically summed norms (module docstring): the bound of a re-ordered sum, and far enough apart to tell the columns
    a, b = std["norms"], scr["norms"]
    bound = int(std["n_obs"]) * np.finfo(np.float64).eps * np.abs(a)
    print("column norms, standard vs scrambled: max |a - b| / |a| =", float(np.max(np.abs(a - b) / np.maximum(np.abs(a), 1e-300))))
    assert a.shape == b.shape and np.all(np.abs(a - b) <= bound)
    nz = np.sort(a[a != 0.0])
    assert np.all(np.diff(nz) > 4 * bound.max())
    assert np.all(np.isfinite(std["step"])) and np.linalg.norm(std["step"][9 * N_CAM:]) > 0 and np.linalg.norm(std["norms"]) > 0
    assert not np.array_equal(std["step"], std["step_given"])   # the scaling took effect


def test_six_column_cameras_leave_the_intrinsic_columns_zero(ba_pair):
    mode, std, scr = ba_pair
    intr = slice(0, 3 * N_CAM)   # ba_index: the intrinsics come first in the standard layout
    for out in (std, scr):
        for k in ("step", "grad", "norms", "step_given", "grad_given"):
            if mode == OptimizationType.BundleAdjustment:
                assert np.all(out[k][intr] == 0.0), k
            else:
                assert np.any(out[k][intr] != 0.0), k


# ---- pose graphs -----------------------------------------------------------------------------------------------------------
def pg_capture(kind, scramble):
    g = pkg.synthetic.make_sphere(3, 4) if kind == "se3" else pkg.synthetic.make_manhattan(N_V, min_gap=3)
    assert g.n_v == N_V
    prob = PoseGraphProblem.pose_graph(g)
    dof = prob.dof
    if scramble:
        prob.pose_col = dof * shuffled(N_V, 21)
    idx = (np.asarray(prob.pose_col)[:, None] + np.arange(dof)[None, :]).ravel()   # v_standard = v_layout[idx]
    assert np.array_equal(np.sort(idx), np.arange(dof * N_V))
    given = 0.5 + np.random.default_rng(6).random(dof * N_V)
    to_layout = np.empty_like(given)
    s = GpuSparseCholeskySolver(0).initialize_structure(prob)
    s.set_parameters(g.poses)
    out = {}
    out["step"] = s.solve_augmented_equation(LAM)[idx]
    out["grad"] = s.get_gradient()[idx]
    out["cov"] = s.pose_covariance_blocks()
    out["norms"] = s.compute_column_norms()[idx]
    H, gh = s.get_hessian(LAM)
    out["H"], out["g"] = H[np.ix_(idx, idx)], gh[idx]
    a, b = np.empty_like(given), np.empty_like(given)
    a[idx], b[idx] = given, given[::-1]
    out["jv_gram"] = np.array(s.jv_gram(a, b))
    to_layout[idx] = given
    s.apply_column_scaling(to_layout)
    out["step_given"] = s.solve_augmented_equation(LAM)[idx]
    out["grad_given"] = s.get_gradient()[idx]
    out["cov_given"] = s.pose_covariance_blocks()
    H, gh = s.get_hessian(LAM)
    out["H_given"], out["g_given"] = H[np.ix_(idx, idx)], gh[idx]
    s.close()
    return out


@pytest.mark.parametrize("kind", ["se3", "se2"])
def test_pose_graph_exports_do_not_depend_on_the_column_layout(kind):
    std, scr = pg_capture(kind, False), pg_capture(kind, True)
    assert std.keys() == scr.keys()
    for k in std:
        assert std[k].shape == scr[k].shape and np.array_equal(std[k], scr[k]), k
    assert np.all(np.isfinite(std["step"])) and np.linalg.norm(std["step"]) > 0 and np.all(std["norms"] > 0)
    assert not np.array_equal(std["step"], std["step_given"])
