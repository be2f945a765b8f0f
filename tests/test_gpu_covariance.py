"""Marginal covariances by selected inversion of the tile factor (SelectedInverse::blocks): the diagonal blocks of the
inverse of the matrix the last direct solve factorised, against dense numpy inverses of the matrices the exports return.
Tolerances per 6 x 6 / 9 x 9 block (relative Frobenius): 1e-10 at lambda = 1e4, 1e-7 at lambda = 1e-3 -- the step-parity
bounds of the suite."""
import os

import numpy as np
import pytest

import apex_solver_amd as pkg
from apex_solver_amd.capi import LinAlgError
from apex_solver_amd.pose_graph import GpuSparseCholeskySolver, PoseGraphProblem
from apex_solver_amd.solver import (GpuSchurComplementSolver, LevenbergMarquardt, LevenbergMarquardtConfig, LinearSolverType,
                                    OptimizationType, Problem, SchurVariant)

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
TOL = {1e4: 1e-10, 1e-3: 1e-7}


def block_err(a, b):
    return float(np.linalg.norm(a - b) / max(np.linalg.norm(b), 1e-300))


def pg_fixture(name, prior):
    g = np.load(os.path.join(HERE, "golden", name + ".npz"))
    d = pkg.synthetic.PoseGraphData(ids=g["ids"], poses=g["poses0"], e_from=g["e_from"], e_to=g["e_to"], meas=g["meas"])
    hub = None if float(g["huber_delta"]) <= 0 else float(g["huber_delta"])
    p = PoseGraphProblem(d, hub, fix=g["fix"].copy())
    if prior:
        p.add_prior(f"x{int(d.ids[0])}", huber_delta=1.0)
    return p


def ba_fixture(name):
    g = np.load(os.path.join(HERE, "golden", name + ".npz"))
    d = pkg.synthetic.BAProblemData(poses=g["poses0"], intr=g["intr0"], points=g["points0"], cam_idx=g["cam_idx"],
                                    pt_idx=g["pt_idx"], obs_uv=g["obs_uv"], name="golden")
    ot = OptimizationType.SelfCalibration if str(g["mode"]) == "selfcal" else OptimizationType.BundleAdjustment
    return d, Problem.bundle_adjustment(d, ot, 1.0)


def pg_blocks_of(Hinv, pose_col):
    return np.stack([Hinv[c:c + 6, c:c + 6] for c in pose_col])


def cam_blocks_of(M, lay, n_cam):
    out = np.zeros((n_cam, 9, 9))
    for c in range(n_cam):
        idx = np.r_[lay.pose_col[c]:lay.pose_col[c] + 6, lay.intr_col[c]:lay.intr_col[c] + 3]
        out[c] = M[np.ix_(idx, idx)]
    return out


def check_pg(s, prob, lam):
    s.solve_augmented_equation(lam)
    cov = s.pose_covariance_blocks()
    H, _ = s.get_hessian(lam)   # re-assembles the matrix of the same point: after the covariance call
    ref = pg_blocks_of(np.linalg.inv(H), prob.pose_col)
    errs = [block_err(cov[v], ref[v]) for v in range(len(ref))]
    assert max(errs) <= TOL[lam], (lam, max(errs))
    return cov


def check_ba(s, prob, lam, n_cam):
    s.solve_augmented_equation(lam)
    assert s.info()["last_reg"] == 0.0           # no ladder regularisation: the factor is of S itself
    cov = s.camera_covariance_blocks()
    S, _ = s.get_schur()
    ref = cam_blocks_of(np.linalg.inv(S), prob.layout, n_cam)
    errs = [block_err(cov[c], ref[c]) for c in range(n_cam)]
    assert max(errs) <= TOL[lam], (lam, max(errs))
    return cov


@pytest.mark.parametrize("scaled", [False, True], ids=["plain", "jacobi"])
@pytest.mark.parametrize("name,prior", [("pg_sphere_8x12", False), ("pg_sphere_10x10_huber", True)])
def test_pg_fixtures(name, prior, scaled):
    prob = pg_fixture(name, prior)
    s = GpuSparseCholeskySolver().initialize_structure(prob)
    s.set_parameters(prob.data.poses)
    if scaled:
        s.apply_column_scaling(1.0 / (1.0 + s.compute_column_norms()))
    for lam in (1e4, 1e-3):
        check_pg(s, prob, lam)
    s.close()


@pytest.mark.parametrize("scaled", [False, True], ids=["plain", "jacobi"])
@pytest.mark.parametrize("name", ["ba6x40_ba", "ba9x120_selfcal_behind"])
def test_ba_fixtures(name, scaled):
    d, prob = ba_fixture(name)
    s = GpuSchurComplementSolver(0).initialize_structure(prob)
    s.set_parameters(d.poses, d.intr, d.points)
    if scaled:
        s.apply_column_scaling(1.0 / (1.0 + s.compute_column_norms()))
    for lam in (1e4, 1e-3):
        check_ba(s, prob, lam, d.n_cam)
    if not scaled:
        # the Schur identity end to end: the camera blocks of (H + lambda I)^-1 over cameras AND landmarks
        lam = 1e4
        s.solve_augmented_equation(lam)
        cov = s.camera_covariance_blocks()
        H = s.get_hessian().toarray()
        ref = cam_blocks_of(np.linalg.inv(H + lam * np.eye(H.shape[0])), prob.layout, d.n_cam)
        assert max(block_err(cov[c], ref[c]) for c in range(d.n_cam)) <= TOL[lam]
    s.close()


def test_ba_recurrence_plan():
    """Several hundred cameras with long-range landmarks: a deep elimination tree with fill tiles."""
    d = pkg.synthetic.make_problem(480, 24000, 3, 8, config_id=7, window=48, long_range_prob=0.002)
    prob = Problem.bundle_adjustment(d, OptimizationType.SelfCalibration, 1.0)
    s = GpuSchurComplementSolver(0).initialize_structure(prob)
    s.set_parameters(d.poses, d.intr, d.points)
    info = s.info()
    print("BA plan:", info)
    assert info["etree_levels"] >= 4 and info["tiles"] > info["touched_tiles"]
    check_ba(s, prob, 1e4, d.n_cam)
    st = s.covariance_stats()
    assert st["extra_bytes"] >= info["tiles"] * 144 * 144 * 8 and st["zoff_products"] > 0
    s.close()


def test_pg_recurrence_plan():
    d = pkg.synthetic.make_sphere(25, 40)      # 1,000 vertices, loop closures between neighbouring rings
    prob = PoseGraphProblem.pose_graph(d)
    s = GpuSparseCholeskySolver().initialize_structure(prob)
    s.set_parameters(d.poses)
    info = s.info()
    print("PG plan:", info)
    assert info["etree_levels"] >= 4 and info["tiles"] > info["touched_tiles"]
    check_pg(s, prob, 1e-3)
    s.close()


def test_refusals():
    prob = pg_fixture("pg_sphere_8x12", False)
    s = GpuSparseCholeskySolver().initialize_structure(prob)
    s.set_parameters(prob.data.poses)
    with pytest.raises(LinAlgError) as e:
        s.pose_covariance_blocks()                       # before any solve
    assert e.value.kind == "InvalidState"
    s.solve_augmented_equation(1e-3)
    s.get_hessian(1e-3)
    with pytest.raises(LinAlgError) as e:
        s.pose_covariance_blocks()                       # the export re-assembled the tiles
    assert e.value.kind == "InvalidState"
    s.close()

    d, bprob = ba_fixture("ba9x120_selfcal_behind")
    b = GpuSchurComplementSolver(0).initialize_structure(bprob)
    b.set_parameters(d.poses, d.intr, d.points)
    with pytest.raises(LinAlgError) as e:
        b.camera_covariance_blocks()
    assert e.value.kind == "InvalidState"
    b.solve_augmented_equation(1e-3)
    b.get_schur()
    with pytest.raises(LinAlgError) as e:
        b.camera_covariance_blocks()
    assert e.value.kind == "InvalidState"
    for v in (SchurVariant.Iterative, SchurVariant.Implicit):
        b.with_variant(SchurVariant.Sparse).solve_augmented_equation(1e-3)
        b.camera_covariance_blocks()                     # (a factor is held ...)
        b.with_variant(v).solve_augmented_equation(1e-3)
        with pytest.raises(LinAlgError) as e:            # ... and gone after a PCG / matrix-free solve
            b.camera_covariance_blocks()
        assert e.value.kind == "InvalidState"
    b.close()

    m = GpuSchurComplementSolver(0).with_option("matrix_free_only", 1).initialize_structure(bprob)
    m.set_parameters(d.poses, d.intr, d.points)
    m.with_variant(SchurVariant.Implicit).solve_augmented_equation(1e-3)
    with pytest.raises(LinAlgError) as e:
        m.camera_covariance_blocks()
    assert e.value.kind == "InvalidState"
    m.close()

    sh = GpuSchurComplementSolver(0).with_shard(0, 2).initialize_structure(bprob)
    with pytest.raises(LinAlgError) as e:
        sh.camera_covariance_blocks()
    assert e.value.kind == "InvalidState" and "rank" in str(e.value)
    sh.close()


def test_no_interference_and_determinism():
    """A covariance call leaves the factor and the step path alone, and repeats bit for bit.  (The pose-graph assembly adds
    its edge blocks with fp64 atomics, so two of its solves agree to rounding only, with or without a covariance call in
    between; the BA assembly is deterministic, and there the step after a covariance call is the same bits.)"""
    prob = pg_fixture("pg_sphere_10x10_huber", True)
    steps, covs = [], []
    for with_cov in (True, False):
        s = GpuSparseCholeskySolver().initialize_structure(prob)
        s.set_parameters(prob.data.poses)
        s.solve_augmented_equation(1e-3)
        if with_cov:
            covs.append(s.pose_covariance_blocks())
            covs.append(s.pose_covariance_blocks())
        steps.append(s.solve_augmented_equation(1e-3))
        s.close()
    assert block_err(steps[0], steps[1]) <= 1e-12
    assert np.array_equal(covs[0], covs[1])

    d, bprob = ba_fixture("ba9x120_selfcal_behind")
    steps, covs = [], []
    for with_cov in (True, False):
        b = GpuSchurComplementSolver(0).initialize_structure(bprob)
        b.set_parameters(d.poses, d.intr, d.points)
        b.solve_augmented_equation(1e-3)
        if with_cov:
            covs.append(b.camera_covariance_blocks())
            covs.append(b.camera_covariance_blocks())
        steps.append(b.solve_augmented_equation(1e-3))
        b.close()
    assert np.array_equal(steps[0], steps[1])
    assert np.array_equal(covs[0], covs[1])


def test_lm_surface_pose_graph():
    # The loop tests "iteration >= max_iterations" after an iteration (lm_loop.cpp, as the reference): max_iterations = 0 runs
    # exactly one, whose factorised solve is at the initial values with lambda = cfg.damping
    prob = pg_fixture("pg_sphere_8x12", False)
    cfg = (LevenbergMarquardtConfig.new().with_linear_solver_type(LinearSolverType.SparseCholesky)
           .with_max_iterations(0).with_compute_covariances(True))
    res = LevenbergMarquardt.with_config(cfg).optimize(prob)
    assert res.iterations == 1 and res.history.shape[0] == 1
    assert res.covariances is not None and set(res.covariances) == {f"x{int(i)}" for i in prob.data.ids}
    s2 = GpuSparseCholeskySolver().initialize_structure(prob)
    s2.set_parameters(prob.data.poses)
    H, _ = s2.get_hessian(cfg.damping)
    s2.close()
    ref = pg_blocks_of(np.linalg.inv(H), prob.pose_col)
    for k, i in enumerate(prob.data.ids):
        c = res.covariances[f"x{int(i)}"]
        assert np.array_equal(c, c.T) and np.all(np.linalg.eigvalsh(c) > 0)
        assert block_err(c, ref[k]) <= TOL[1e-3]
    # flag off: no covariances, the same loop (to the rounding of the atomic assembly; bit for bit on the BA arm below)
    on = LevenbergMarquardt.with_config(cfg.with_max_iterations(5)).optimize(prob)
    off = LevenbergMarquardt.with_config(cfg.with_max_iterations(5).with_compute_covariances(False)).optimize(prob)
    assert off.covariances is None and on.covariances is not None
    assert np.array_equal(on.history[:, 3], off.history[:, 3]) and np.allclose(on.history, off.history, rtol=1e-9, atol=0)


def test_lm_surface_bundle_adjustment():
    d, prob = ba_fixture("ba6x40_ba")
    cfg = LevenbergMarquardtConfig().with_max_iterations(3).with_compute_covariances(True)
    res = LevenbergMarquardt.with_config(cfg).optimize(prob)
    keys = {f"pose_{i:04}" for i in range(d.n_cam)} | {f"intr_{i:04}" for i in range(d.n_cam)}
    assert set(res.covariances) == keys
    assert all(res.covariances[f"pose_{i:04}"].shape == (6, 6) and res.covariances[f"intr_{i:04}"].shape == (3, 3) for i in range(d.n_cam))
    off = LevenbergMarquardt.with_config(cfg.with_compute_covariances(False)).optimize(prob)
    assert off.covariances is None and np.array_equal(res.history, off.history)
    with pytest.warns(RuntimeWarning, match="covariances not computed"):
        it = LevenbergMarquardt.with_config(cfg.with_schur_variant(SchurVariant.Iterative)).optimize(prob)
    assert it.covariances is None
