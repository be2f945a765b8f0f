"""The robust loss family on the bundle-adjustment device path (apexgpu_set_loss) against the numpy reference
tests/np_ref_ba_loss.py.  Bounds: those of tests/test_gpu_parity.py for Huber (r, J, g, S 1e-12; g_red 1e-10; backward error
1e-13; step STEP_FORWARD_BOUND at lambda = 1e-3, 1e-10 at 1e4), the cost at test_gpu_pg_loss.py's 1e-12."""
import functools

import numpy as np
import pytest

import apex_solver_amd as pkg
import ba_loss_cases as bc
import np_ref_ba_loss as nb
import referee
from apex_solver_amd import capi
from ba_custom import custom_problem
from apex_solver_amd.loss import Loss, create_loss_function
from apex_solver_amd.solver import (GpuSchurComplementSolver, LevenbergMarquardtConfig, OptimizationType, Problem, SchurVariant)

pytestmark = pytest.mark.gpu
STEP_FORWARD_BOUND = 1e-7   # (tests/test_gpu_parity.py)
MODES = {"selfcal": OptimizationType.SelfCalibration, "ba": OptimizationType.BundleAdjustment, "pose_intr": OptimizationType.PoseAndIntrinsics,
         "only_pose": OptimizationType.OnlyPose}


def rel(a, b):
    a = np.ravel(a); b = np.ravel(b)
    return float(np.linalg.norm(a - b) / max(np.linalg.norm(b), 1e-300))


def gpu_solver(d, mode, loss=None, huber=None, variant=SchurVariant.Sparse, shard=None, set_params=True):
    prob = Problem.bundle_adjustment(d, MODES[mode], huber, loss=loss)
    s = GpuSchurComplementSolver(0).with_variant(variant)
    if shard:
        s.with_shard(*shard)
    s.initialize_structure(prob)
    if set_params:
        s.set_parameters(d.poses, d.intr, d.points)
    return prob, s


@functools.lru_cache(maxsize=None)
def sweep_data():
    d = bc.problem()
    return d, bc.sweep_losses(bc.raw_residuals(d))


@functools.lru_cache(maxsize=None)
def sweep_reference(name, mode):
    """computed once per (loss, mode), shared, never modified"""
    d, losses = sweep_data()
    lay = Problem.bundle_adjustment(d, MODES[mode]).layout
    flags = MODES[mode].flags
    return nb.System(d, lay, losses[name], selfcal=bool(flags[2]), flags=flags)


def check_assembly_and_steps(d, prob, s, P, dc, label, lambdas=(1e-3, 1e4)):
    """the bounds of the module docstring, on one handle against one reference System"""
    cost = s.compute_cost()
    r = s.get_residual().reshape(-1, 2)
    jc, jl = s.get_jacobian_blocks()
    Jc_ref = np.concatenate([P.Jp, P.Ji], axis=2)[:, :, :dc]
    errs = dict(cost=abs(cost - P.cost) / P.cost, r=rel(r, P.r), jc=rel(jc, Jc_ref), jl=rel(jl, P.Jl) if P.Jl.any() else float(np.abs(jl).max()))
    cut = P.w == 0.0
    if cut.any():   # exactly zero where rho' = 0
        assert not r[cut].any() and not jc[cut].any() and not jl[cut].any()
    nc = P.nc
    for lam in lambdas:
        step = s.solve_augmented_equation(lam)
        S, gred = s.get_schur()
        oS, ogred = P.schur(lam)
        ostep = P.step(lam)
        bwd = np.linalg.norm(oS @ step[:nc] - ogred) / (referee.sym_norm2(oS) * np.linalg.norm(step[:nc]) + np.linalg.norm(ogred))
        e = dict(g=rel(s.get_gradient(), P.g), S=rel(S, oS), gred=rel(gred, ogred), bwd=bwd, step=rel(step, ostep))
        print(label, f"lambda {lam:g}", {k: f"{v:.1e}" for k, v in {**errs, **e}.items()})
        assert errs["cost"] < 1e-12 and errs["r"] < 1e-12 and errs["jc"] < 1e-12 and errs["jl"] < 1e-12, errs
        assert e["g"] < 1e-12 and e["S"] < 1e-12 and e["gred"] < 1e-10, e
        assert e["bwd"] < 1e-13 and e["step"] < (STEP_FORWARD_BOUND if lam == 1e-3 else 1e-10), e
    return step


@pytest.mark.parametrize("mode", ["selfcal", "ba"])
@pytest.mark.parametrize("name", bc.SWEEP)
def test_parity_sweep(name, mode):
    d, losses = sweep_data()
    bc.check_conditions(name, losses[name], d)
    prob, s = gpu_solver(d, mode, loss=losses[name])
    assert s.get_loss() == losses[name]
    check_assembly_and_steps(d, prob, s, sweep_reference(name, mode), 9 if mode == "selfcal" else 6, f"{name} {mode}")
    s.close()


def test_masked_mode_under_cauchy():
    d, losses = sweep_data()
    prob, s = gpu_solver(d, "pose_intr", loss=losses["cauchy"])
    check_assembly_and_steps(d, prob, s, sweep_reference("cauchy", "pose_intr"), 9, "cauchy pose_intr")
    s.close()


def test_six_column_masked_mode_under_cauchy():
    """OnlyPose: six camera columns and the landmark group masked, so the solve's back-substitution has no record form to take
    and runs the general-loss instantiation at d_c = 6 (launch_back_substitute), which no other test reaches"""
    d, losses = sweep_data()
    prob, s = gpu_solver(d, "only_pose", loss=losses["cauchy"])
    check_assembly_and_steps(d, prob, s, sweep_reference("cauchy", "only_pose"), 6, "cauchy only_pose")
    s.close()


def _everything(s, lam=1e-3):
    out = [s.get_residual(), *s.get_jacobian_blocks(), np.array([s.compute_cost()])]
    s.solve_augmented_equation(lam)
    out += list(s.get_schur())
    # (six iterations: the loop runs max_iterations + 1)
    res, hist, _ = s.lm_optimize(LevenbergMarquardtConfig(max_iterations=5, cost_tolerance=0.0, parameter_tolerance=0.0, gradient_tolerance=0.0))
    return out + [hist, *s.get_parameters()]


@pytest.mark.parametrize("mode", ["selfcal", "ba"])
@pytest.mark.parametrize("case", ["huber", "l2", "none"])
def test_legacy_kinds_through_set_loss_are_the_huber_delta_kernels_bit_for_bit(case, mode):
    d, losses = sweep_data()
    delta = losses["huber"].p0
    loss, huber = {"huber": (Loss(capi.LOSS_HUBER, delta), delta), "l2": (Loss(capi.LOSS_L2), None), "none": (Loss(capi.LOSS_NONE), None)}[case]
    _, a = gpu_solver(d, mode, huber=huber)
    _, b = gpu_solver(d, mode, huber=3.0, loss=loss)    # (set_structure's own delta is replaced)
    assert b.get_loss() == loss
    for x, y in zip(_everything(a), _everything(b)):
        assert np.array_equal(x, y)
    a.close(); b.close()


def _custom(n_cam, cam_lists, seed=5):
    """tests/ba_custom.py: explicit per-landmark camera lists (duplicates allowed), shuffled, every fifth factor an outlier"""
    return custom_problem(n_cam, cam_lists, seed=seed, outlier_every=5)


@pytest.mark.parametrize("mode", ["selfcal", "ba"])
def test_ragged_landmarks_under_cauchy(mode):
    n_cam = 210
    rng = np.random.default_rng(9)
    lists = [[], [3], [5, 5, 9], list(range(64)), list(range(65)), list(range(40, 169)), list(range(200))]
    lists += [sorted(rng.choice(n_cam, size=int(rng.integers(2, 12)), replace=False).tolist()) for _ in range(50)]
    d = _custom(n_cam, lists)
    loss = create_loss_function("cauchy", 2.0)
    prob, s = gpu_solver(d, mode, loss=loss)
    P = nb.System(d, prob.layout, loss, selfcal=mode == "selfcal", flags=MODES[mode].flags)
    check_assembly_and_steps(d, prob, s, P, 9 if mode == "selfcal" else 6, f"ragged {mode}")
    s.close()


def test_a_landmark_all_of_whose_observations_are_cut():
    d0, losses = sweep_data()
    L = 17
    uv = d0.obs_uv.copy()
    uv[d0.pt_idx == L] += 500.0
    d = pkg.synthetic.BAProblemData(d0.poses, d0.intr, d0.points, d0.cam_idx, d0.pt_idx, uv)
    loss = losses["tukey"]
    prob, s = gpu_solver(d, "selfcal", loss=loss)
    P = nb.System(d, prob.layout, loss, selfcal=True)
    assert (P.w[d.pt_idx == L] == 0.0).all() and (d.pt_idx == L).sum() >= 3
    lam = 1e-3
    step = check_assembly_and_steps(d, prob, s, P, 9, "all cut", lambdas=(1e4, lam))
    c = prob.layout.pt_col[L]
    assert not step[c:c + 3].any()
    hinv, gl = s.get_landmark_blocks()
    # (lambda^2 / lambda^3 of the 3 x 3 inverse is 1 / lambda to a rounding; the off-diagonal entries are exact zeros)
    assert np.allclose(np.diag(hinv[L]), 1.0 / lam, rtol=4e-16, atol=0) and not (hinv[L] - np.diag(np.diag(hinv[L]))).any() and not gl[L].any()
    s.close()


@pytest.mark.parametrize("variant", [SchurVariant.Iterative, SchurVariant.Implicit])
def test_pcg_variants_under_cauchy(variant):
    d = pkg.synthetic.make_problem(30, 1500, 3, 7, config_id=77)
    loss = create_loss_function("cauchy", 1.0)
    prob, s = gpu_solver(d, "selfcal", loss=loss, variant=variant)
    P = nb.System(d, prob.layout, loss, selfcal=True)
    s.with_cg_params(5000, 1e-13)
    step = s.solve_augmented_equation(1e4)
    assert rel(s.get_gradient(), P.g) < 1e-12
    e = rel(step, P.step(1e4))
    print(variant, "pcg iterations", s.info()["pcg_iterations"], "step", e)
    assert e < 1e-10
    x = np.random.default_rng(0).normal(size=prob.layout.cam_dof)
    ye, yi = s.schur_matvec(1e-2, x)
    ref = P.schur(1e-2)[0] @ x
    assert rel(ye, ref) < 1e-12 and rel(yi, ref) < 1e-12
    s.close()


@pytest.mark.parametrize("name", ["cauchy", "tukey"])
def test_lm_history_against_the_numpy_loop(name):
    d, losses = sweep_data()
    prob, s = gpu_solver(d, "selfcal", loss=losses[name])
    hist_ref, params_ref = nb.lm(d, prob.layout, losses[name], True, prob.fix_pose, 8)
    # the reference's accept / reject decisions (cost before > trial cost) away from their threshold: two costs that agree to
    # the 1e-7 asserted below move the difference by at most 2e-7 of the cost; five times that is asked
    before = np.r_[nb.System(d, prob.layout, losses[name], True).cost, hist_ref[:-1, 0]]
    assert (np.abs(before - hist_ref[:, 7]) > 1e-6 * before).all()
    # (max_iterations = 7 is eight iterations: the loop tests `iteration >= max_iterations` after the step, like the reference)
    res, hist, _ = s.lm_optimize(LevenbergMarquardtConfig(max_iterations=7, cost_tolerance=0.0, parameter_tolerance=0.0, gradient_tolerance=0.0))
    print(name, "accepted", hist[:, 3], "costs", hist[:, 0])
    assert len(hist) == 8 and np.array_equal(hist[:, 3], hist_ref[:, 3])
    assert np.allclose(hist[:, 0], hist_ref[:, 0], rtol=1e-7, atol=0) and np.allclose(hist[:, 7], hist_ref[:, 7], rtol=1e-7, atol=0)
    s.close()


def test_jacobi_column_norms_under_cauchy():
    d, losses = sweep_data()
    prob, s = gpu_solver(d, "selfcal", loss=losses["cauchy"])
    assert rel(s.compute_column_norms(), sweep_reference("cauchy", "selfcal").column_norms()) < 1e-12
    s.close()


def test_covariances_after_a_cauchy_solve():
    d, losses = sweep_data()
    prob, s = gpu_solver(d, "selfcal", loss=losses["cauchy"])
    P = sweep_reference("cauchy", "selfcal")
    lam = 1e4
    s.solve_augmented_equation(lam)
    cam = s.camera_covariance_blocks()
    lmk = s.landmark_covariance_blocks()
    Minv = np.linalg.inv(P.H + lam * np.eye(P.H.shape[0]))
    lay = prob.layout
    for c in range(d.n_cam):
        idx = np.r_[lay.pose_col[c]:lay.pose_col[c] + 6, lay.intr_col[c]:lay.intr_col[c] + 3]
        assert rel(cam[c], Minv[np.ix_(idx, idx)]) <= 1e-10
    worst = max(rel(lmk[l], Minv[c:c + 3, c:c + 3]) for l, c in enumerate(lay.pt_col))
    assert worst <= 1e-10, worst
    s.set_loss(losses["tukey"])     # the factor was linearised under the old loss: its landmark covariances are gone
    with pytest.raises(capi.LinAlgError) as e:
        s.landmark_covariance_blocks()
    assert e.value.code == -6
    s.close()


def test_shard_partials_sum_to_the_whole_under_cauchy():
    d, losses = sweep_data()
    _, s = gpu_solver(d, "selfcal", loss=losses["cauchy"])
    s.assemble(1e-3)
    S, gred = s.get_schur()
    parts = []
    for r in range(2):
        _, sr = gpu_solver(d, "selfcal", loss=losses["cauchy"], shard=(r, 2))
        sr.assemble(1e-3)
        parts.append(sr.get_schur())
        sr.close()
    assert rel(parts[0][0] + parts[1][0], S) < 1e-12 and rel(parts[0][1] + parts[1][1], gred) < 1e-11
    s.close()


def test_api_edges():
    d, losses = sweep_data()
    h = capi.Handle(d.n_cam, d.n_pt, d.n_obs, 1, 0)
    assert h.L.apexgpu_set_loss(h.h, capi.LOSS_CAUCHY, 1.0, 0.0) == -6      # before set_structure
    h.close()
    prob, s = gpu_solver(d, "selfcal", huber=1.5)
    assert s.get_loss() == Loss(capi.LOSS_HUBER, 1.5)
    s.set_loss(losses["cauchy"])
    for bad, word in ((Loss(capi.LOSS_CAUCHY, -1.0), "parameter"), (Loss(99, 1.0), "unknown"), (bc.REFUSED["andrews"], "Andrews"),
                      (bc.REFUSED["lp3"], "LpNorm"), (bc.REFUSED["barron3"], "Barron")):
        with pytest.raises(capi.LinAlgError) as e:
            s.set_loss(bad)
        assert e.value.code == -5 and word in str(e.value), str(e.value)
        assert s.get_loss() == losses["cauchy"]
    s.solve_augmented_equation(1e-3)
    s.eval_step()
    s.set_loss(losses["welsch"])        # voids the trial point
    with pytest.raises(capi.LinAlgError) as e:
        s.commit_step()
    assert e.value.code == -6
    s.set_loss(None)
    assert s.get_loss() == Loss(capi.LOSS_NONE)
    s.reinitialize_structure(Problem.bundle_adjustment(d, MODES["selfcal"], 2.0))   # the next set_structure: huber_delta again
    assert s.get_loss() == Loss(capi.LOSS_HUBER, 2.0)
    s.close()
