"""Marginal landmark covariances from the selected inverse of S (Solver::landmark_covariance, cov_kernels.hip): the 3 x 3
landmark blocks of the inverse of the matrix the last direct solve factorised, against dense numpy inverses.  The reference
matrix is D H D + lambda I with every landmark's diagonal block replaced by the one the factor used (D inv(hinv_l) D: the
eigenvalue gate included).  Tolerances per block (relative Frobenius) as test_gpu_covariance.py: 1e-10 at lambda = 1e4, 1e-7
at lambda = 1e-3.  The covariance calls come before any export: exports re-assemble."""
import os

import numpy as np
import pytest

import apex_solver_amd as pkg
from apex_solver_amd.capi import LinAlgError
from apex_solver_amd.solver import (GpuSchurComplementSolver, LevenbergMarquardt, LevenbergMarquardtConfig, OptimizationType,
                                    Problem, SchurVariant)

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
TOL = {1e4: 1e-10, 1e-3: 1e-7}


def block_err(a, b):
    return float(np.linalg.norm(a - b) / max(np.linalg.norm(b), 1e-300))


def load_fixture(name):
    g = np.load(os.path.join(HERE, "golden", name + ".npz"))
    d = pkg.synthetic.BAProblemData(poses=g["poses0"], intr=g["intr0"], points=g["points0"], cam_idx=g["cam_idx"],
                                    pt_idx=g["pt_idx"], obs_uv=g["obs_uv"], name="golden")
    ot = OptimizationType.SelfCalibration if str(g["mode"]) == "selfcal" else OptimizationType.BundleAdjustment
    return d, ot


def quat_rot(q):
    w, x, y, z = q / np.linalg.norm(q)
    return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y)],
                     [2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x)],
                     [2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)]])


def with_close_landmark(d, frac):
    """d plus one landmark seen by ONE camera, on the ray of an observation in front of its camera but `frac` of the way
    from the camera centre: the same measurement, a 1 / frac^2 larger Hll of rank 2 -- at a small lambda the eigenvalue gate
    regularises it."""
    for i in range(d.n_obs):
        c, p = int(d.cam_idx[i]), int(d.pt_idx[i])
        R = quat_rot(d.poses[c, 3:7])
        if (R @ d.points[p] + d.poses[c, 0:3])[2] < -0.5:     # in front (the camera looks down -z)
            break
    centre = -R.T @ d.poses[c, 0:3]
    newp = centre + frac * (d.points[p] - centre)
    return pkg.synthetic.BAProblemData(
        poses=d.poses, intr=d.intr, points=np.vstack([d.points, newp[None]]),
        cam_idx=np.append(d.cam_idx, d.cam_idx[i]).astype(d.cam_idx.dtype),
        pt_idx=np.append(d.pt_idx, d.n_pt).astype(d.pt_idx.dtype),
        obs_uv=np.vstack([d.obs_uv, d.obs_uv[i][None]]), name=d.name)


def cam_blocks_of(M, lay, n_cam):
    out = np.zeros((n_cam, 9, 9))
    for c in range(n_cam):
        idx = np.r_[lay.pose_col[c]:lay.pose_col[c] + 6, lay.intr_col[c]:lay.intr_col[c] + 3]
        out[c] = M[np.ix_(idx, idx)]
    return out


def dense_reference(H, lay, hinv, lam, scale):
    """inverse of D H D + lambda I with the landmark blocks the factor used; scale: the column scaling or None"""
    n = H.shape[0]
    D = np.ones(n) if scale is None else np.asarray(scale)
    M = D[:, None] * H * D[None, :] + lam * np.eye(n)
    for l, c in enumerate(lay.pt_col):
        dl = D[c:c + 3]
        M[c:c + 3, c:c + 3] = dl[:, None] * np.linalg.inv(hinv[l]) * dl[None, :]
    return np.linalg.inv(M)


def check_against_dense(s, prob, n_cam, lam, scale, tol=None):
    """solve at lam, then camera and landmark blocks against the dense inverse; returns (landmark blocks, hinv, H)"""
    tol = TOL[lam] if tol is None else tol
    s.solve_augmented_equation(lam)
    assert s.info()["last_reg"] == 0.0
    cam = s.camera_covariance_blocks()
    lmk = s.landmark_covariance_blocks()
    hinv, _ = s.get_landmark_blocks()
    H = s.get_hessian().toarray()     # (re-assembles: after the covariance calls)
    Minv = dense_reference(H, prob.layout, hinv, lam, scale)
    ref_c = cam_blocks_of(Minv, prob.layout, n_cam)
    assert max(block_err(cam[c], ref_c[c]) for c in range(n_cam)) <= tol     # the convention, anchored on the camera blocks
    errs = [block_err(lmk[l], Minv[c:c + 3, c:c + 3]) for l, c in enumerate(prob.layout.pt_col)]
    assert max(errs) <= tol, (lam, max(errs), int(np.argmax(errs)))
    assert np.array_equal(lmk, np.transpose(lmk, (0, 2, 1)))
    return lmk, hinv, H


@pytest.mark.parametrize("scaled", [False, True], ids=["plain", "jacobi"])
@pytest.mark.parametrize("name", ["ba6x40_ba", "ba9x120_selfcal_behind"])
def test_golden_fixtures(name, scaled):
    d, ot = load_fixture(name)
    prob = Problem.bundle_adjustment(d, ot, 1.0)
    s = GpuSchurComplementSolver(0).initialize_structure(prob)
    s.set_parameters(d.poses, d.intr, d.points)
    scale = None
    if scaled:
        scale = 1.0 / (1.0 + s.compute_column_norms())
        s.apply_column_scaling(scale)
    for lam in (1e4, 1e-3):
        check_against_dense(s, prob, d.n_cam, lam, scale)
    s.close()


@pytest.mark.parametrize("name", ["ba6x40_ba", "ba9x120_selfcal_behind"])
def test_gate_and_fixed_landmark(name):
    d0, ot = load_fixture(name)
    lam = 1e-3
    # the farthest that fires: max_ev / min_ev of the damped block passes 1e10 (the closer, the worse cond(M))
    for frac in (0.2, 0.1, 0.05, 0.02, 0.01, 5e-3, 2e-3, 1e-3, 1e-4):
        d = with_close_landmark(d0, frac)
        prob = Problem.bundle_adjustment(d, ot, 1.0)
        prob.fix_variable(f"pt_{3:05}", 0)
        prob.fix_variable(f"pt_{3:05}", 2)
        s = GpuSchurComplementSolver(0).initialize_structure(prob)
        s.set_parameters(d.poses, d.intr, d.points)
        s.solve_augmented_equation(lam)
        hinv, _ = s.get_landmark_blocks()
        H = s.get_hessian().toarray()
        c = int(prob.layout.pt_col[d.n_pt - 1])
        plain = np.linalg.inv(H[c:c + 3, c:c + 3] + lam * np.eye(3))
        if block_err(hinv[d.n_pt - 1], plain) > 1e-3:   # the gate fired on the close landmark
            break
        s.close()
    else:
        pytest.fail("the eigenvalue gate did not fire")
    # The gated block's max_ev raises cond(M) far above the fixture's: the dense inverse loses a digit on every landmark
    # (2e-7 .. 4e-7 at lambda = 1e-3), so the dense comparison takes ten times the bound, and the gated landmark itself, whose
    # block the dense inverse resolves worst, is checked against the Schur formula in numpy at the plain bound.
    s.solve_augmented_equation(lam)
    cam = s.camera_covariance_blocks()
    lmk = s.landmark_covariance_blocks()
    hinv, _ = s.get_landmark_blocks()
    S, _ = s.get_schur()
    H = s.get_hessian().toarray()
    Minv = dense_reference(H, prob.layout, hinv, lam, None)
    ref_c = cam_blocks_of(Minv, prob.layout, d.n_cam)
    assert max(block_err(cam[i], ref_c[i]) for i in range(d.n_cam)) <= 10 * TOL[lam]
    g = d.n_pt - 1
    errs = [block_err(lmk[l], Minv[c:c + 3, c:c + 3]) for l, c in enumerate(prob.layout.pt_col) if l != g]
    assert max(errs) <= 10 * TOL[lam], max(errs)
    c = int(prob.layout.pt_col[g])
    U = H[:prob.layout.cam_dof, c:c + 3] @ hinv[g]
    assert block_err(lmk[g], hinv[g] + U.T @ np.linalg.solve(S, U)) <= TOL[lam]
    assert np.array_equal(lmk, np.transpose(lmk, (0, 2, 1)))
    assert np.all(np.linalg.eigvalsh(lmk[g]) > 0)
    print("gate fired at frac", frac)
    s.close()


def test_large_landmarks():
    """Landmarks seen by 80 to 150 cameras: the workgroup-wide path, several observation chunks per landmark."""
    d = pkg.synthetic.make_problem(160, 400, 80, 150, window=160)
    prob = Problem.bundle_adjustment(d, OptimizationType.SelfCalibration, 1.0)
    s = GpuSchurComplementSolver(0).initialize_structure(prob)
    s.set_parameters(d.poses, d.intr, d.points)
    check_against_dense(s, prob, d.n_cam, 1e4, None)
    k = np.bincount(d.pt_idx, minlength=d.n_pt)
    assert k.max() > 2 * 32 and s.landmark_covariance_stats()["pairs"] == int((k * (k + 1) // 2).sum())
    s.close()


def test_deep_plan_schur_restatement():
    d = pkg.synthetic.make_problem(480, 24000, 3, 8, config_id=7, window=48, long_range_prob=0.002)
    prob = Problem.bundle_adjustment(d, OptimizationType.SelfCalibration, 1.0)
    s = GpuSchurComplementSolver(0).initialize_structure(prob)
    s.set_parameters(d.poses, d.intr, d.points)
    info = s.info()
    assert info["etree_levels"] >= 4 and info["tiles"] > info["touched_tiles"]
    lam = 1e4
    s.solve_augmented_equation(lam)
    lmk = s.landmark_covariance_blocks()
    hinv, _ = s.get_landmark_blocks()
    S, _ = s.get_schur()                 # the camera-side column order of the global layout
    Z = np.linalg.inv(S)
    H = s.get_hessian().tocsc()
    ncd = prob.layout.cam_dof
    rng = np.random.default_rng(3)
    sample = rng.choice(d.n_pt, 600, replace=False)
    errs = []
    for l in sample:
        c = int(prob.layout.pt_col[l])
        B = H[:ncd, c:c + 3].toarray()   # W_l: camera rows of landmark l's columns
        U = B @ hinv[l]
        errs.append(block_err(lmk[l], hinv[l] + U.T @ Z @ U))
    assert max(errs) <= TOL[lam], max(errs)
    s.close()


def test_linearisation_point_after_commit_and_discard():
    d, ot = load_fixture("ba9x120_selfcal_behind")
    prob = Problem.bundle_adjustment(d, ot, 1.0)
    for lam, after in ((1e4, "commit"), (1e-3, "discard")):
        fresh = GpuSchurComplementSolver(0).initialize_structure(prob)
        fresh.set_parameters(d.poses, d.intr, d.points)
        fresh.solve_augmented_equation(lam)
        ref = fresh.landmark_covariance_blocks()
        fresh.close()
        s = GpuSchurComplementSolver(0).initialize_structure(prob)
        s.set_parameters(d.poses, d.intr, d.points)
        s.solve_augmented_equation(lam)
        s.eval_step()
        if after == "commit":
            s.commit_step()              # the factorised cameras are in the other parameter set now
            tol = 1e-12
        else:
            s.discard_step()             # the reverted cameras: the factorised ones up to rounding
            tol = TOL[lam]
        got = s.landmark_covariance_blocks()
        errs = [block_err(got[l], ref[l]) for l in range(d.n_pt)]
        assert max(errs) <= tol, (after, max(errs))
        s.close()


def test_reuse_determinism_and_no_interference():
    d, ot = load_fixture("ba9x120_selfcal_behind")
    prob = Problem.bundle_adjustment(d, ot, 1.0)
    steps, first = [], None
    for with_cov in (True, False):
        s = GpuSchurComplementSolver(0).initialize_structure(prob)
        s.set_parameters(d.poses, d.intr, d.points)
        s.solve_augmented_equation(1e-3)
        if with_cov:
            a = s.landmark_covariance_blocks()
            st = s.landmark_covariance_stats()
            assert st["recomputed_z"] and st["pairs"] > 0 and st["extra_bytes"] > 0
            b = s.landmark_covariance_blocks()
            assert np.array_equal(a, b)
            assert not s.landmark_covariance_stats()["recomputed_z"]   # (Z of this factor is still current)
            s.camera_covariance_blocks()
            c = s.landmark_covariance_blocks()
            assert not s.landmark_covariance_stats()["recomputed_z"]
            assert np.array_equal(a, c)
            assert np.array_equal(a, np.transpose(a, (0, 2, 1)))
            assert np.all(np.linalg.eigvalsh(a) > 0)
            first = a
        steps.append(s.solve_augmented_equation(1e-3))
        s.close()
    assert np.array_equal(steps[0], steps[1])
    # after a camera call on a fresh handle: reused, same bits
    s = GpuSchurComplementSolver(0).initialize_structure(prob)
    s.set_parameters(d.poses, d.intr, d.points)
    s.solve_augmented_equation(1e-3)
    s.camera_covariance_blocks()
    got = s.landmark_covariance_blocks()
    assert s.landmark_covariance_stats()["recomputed_z"] is False
    assert np.array_equal(got, first)
    s.close()


def test_refusals():
    d, ot = load_fixture("ba9x120_selfcal_behind")
    prob = Problem.bundle_adjustment(d, ot, 1.0)
    b = GpuSchurComplementSolver(0).initialize_structure(prob)
    b.set_parameters(d.poses, d.intr, d.points)
    with pytest.raises(LinAlgError) as e:
        b.landmark_covariance_blocks()                   # before any solve
    assert e.value.kind == "InvalidState"
    b.solve_augmented_equation(1e-3)
    b.get_schur()
    with pytest.raises(LinAlgError) as e:
        b.landmark_covariance_blocks()                   # the export re-assembled the tiles
    assert e.value.kind == "InvalidState"
    b.solve_augmented_equation(1e-3)
    b.set_parameters(d.poses, d.intr, d.points)
    with pytest.raises(LinAlgError) as e:
        b.landmark_covariance_blocks()                   # the factor's linearisation point was overwritten
    assert e.value.kind == "InvalidState" and "linearisation" in str(e.value)
    for v in (SchurVariant.Iterative, SchurVariant.Implicit):
        b.with_variant(SchurVariant.Sparse).solve_augmented_equation(1e-3)
        b.landmark_covariance_blocks()
        b.with_variant(v).solve_augmented_equation(1e-3)
        with pytest.raises(LinAlgError) as e:
            b.landmark_covariance_blocks()
        assert e.value.kind == "InvalidState"
    b.close()

    m = GpuSchurComplementSolver(0).with_option("matrix_free_only", 1).initialize_structure(prob)
    m.set_parameters(d.poses, d.intr, d.points)
    m.with_variant(SchurVariant.Implicit).solve_augmented_equation(1e-3)
    with pytest.raises(LinAlgError) as e:
        m.landmark_covariance_blocks()
    assert e.value.kind == "InvalidState"
    m.close()

    sh = GpuSchurComplementSolver(0).with_shard(0, 2).initialize_structure(prob)
    with pytest.raises(LinAlgError) as e:
        sh.landmark_covariance_blocks()
    assert e.value.kind == "InvalidState" and "rank" in str(e.value)
    sh.close()


def test_lm_surface():
    d, ot = load_fixture("ba6x40_ba")
    prob = Problem.bundle_adjustment(d, ot, 1.0)
    cfg = (LevenbergMarquardtConfig().with_max_iterations(0).with_compute_covariances(True)
           .with_compute_landmark_covariances(True))
    res = LevenbergMarquardt.with_config(cfg).optimize(prob)
    assert res.iterations == 1
    cam_keys = {f"pose_{i:04}" for i in range(d.n_cam)} | {f"intr_{i:04}" for i in range(d.n_cam)}
    pt_keys = {f"pt_{l:05}" for l in range(d.n_pt)}
    assert set(res.covariances) == cam_keys | pt_keys
    # the factorised solve of that one iteration: the initial values at lambda = cfg.damping
    s = GpuSchurComplementSolver(0).initialize_structure(prob)
    s.set_parameters(d.poses, d.intr, d.points)
    s.solve_augmented_equation(cfg.damping)
    hinv, _ = s.get_landmark_blocks()
    H = s.get_hessian().toarray()
    s.close()
    Minv = dense_reference(H, prob.layout, hinv, cfg.damping, None)
    tol = TOL[1e-3] if cfg.damping < 1.0 else TOL[1e4]
    for l, c in enumerate(prob.layout.pt_col):
        blk = res.covariances[f"pt_{l:05}"]
        assert np.array_equal(blk, blk.T) and block_err(blk, Minv[c:c + 3, c:c + 3]) <= tol
    # only compute_covariances: exactly the camera keys, and the loop is the same bits with or without landmarks
    cfg3 = cfg.with_max_iterations(3)
    cams = LevenbergMarquardt.with_config(cfg3.with_compute_landmark_covariances(False)).optimize(prob)
    both = LevenbergMarquardt.with_config(cfg3).optimize(prob)
    assert set(cams.covariances) == cam_keys
    assert set(both.covariances) == cam_keys | pt_keys
    assert np.array_equal(cams.history, both.history)
