"""Both device conjugate-gradient loops through the C ABI -- TilePcg::solve (csrc/tile_pcg.hip) behind SchurVariant.Iterative and
Solver::implicit_pcg_solve behind SchurVariant.Implicit -- capped before convergence, at it and past it, against the oracle
under the same cap (tests/test_gpu_pcg.py runs the explicit loop on crafted tiles; tests/test_pcg_ref_host.py pins the
oracle's two loops to a plain long double restatement).

Problem, damping and tolerances are those of the existing comparisons of the converged PCG steps with the oracle
(tests/test_gpu_parity.py, lambda = 1e4: 1e-10 for the explicit loop, 1e-9 for the matrix-free one)."""
import numpy as np
import pytest

import apex_solver_amd as pkg
from apex_solver_amd.solver import GpuSchurComplementSolver, OptimizationType, Problem, SchurVariant

pytestmark = pytest.mark.gpu

LAM = 1e4
TOL = 1e-13
STEP_TOL = {SchurVariant.Iterative: 1e-10, SchurVariant.Implicit: 1e-9}
ORACLE_VARIANT = {SchurVariant.Iterative: 1, SchurVariant.Implicit: 2}


def rel(a, b):
    a = np.ravel(a); b = np.ravel(b)
    return float(np.linalg.norm(a - b) / max(np.linalg.norm(b), 1e-300))


def _pair(oracle, mode, variant, scaled, config_id=77):
    d = pkg.synthetic.make_problem(30, 1500, 3, 7, config_id=config_id)
    ot = OptimizationType.SelfCalibration if mode == "selfcal" else OptimizationType.BundleAdjustment
    prob = Problem.bundle_adjustment(d, ot, 1.0)
    s = GpuSchurComplementSolver(0).with_variant(variant)
    s.initialize_structure(prob)
    s.set_parameters(d.poses, d.intr, d.points)
    o = oracle.from_data(d, prob.layout, mode=mode, huber_delta=1.0)
    o.linearize()
    if scaled:
        scal = 1.0 / (1.0 + o.column_norms())
        s.apply_column_scaling(scal); o.set_column_scaling(scal)
    return prob, s, o


def _oracle_capped(o, variant, cap):
    o.set_cg_params(cap, TOL)
    step, _ = o.solve_augmented(LAM, ORACLE_VARIANT[variant])
    return step, o.last_pcg_iters


def _gpu_capped(s, cap):
    s.with_cg_params(cap, TOL)
    step = s.solve_augmented_equation(LAM)
    return step, s.info()["pcg_iterations"]


@pytest.mark.parametrize("scaled", [False, True], ids=["plain", "jacobi_scaled"])
@pytest.mark.parametrize("variant", [SchurVariant.Iterative, SchurVariant.Implicit], ids=["iterative", "implicit"])
@pytest.mark.parametrize("mode", ["selfcal", "ba"])
def test_capped_loops_follow_the_oracle(oracle, mode, variant, scaled):
    """with_cg_params(k, 1e-13) for k = 0, 1, 2, 3, 5, k_conv: pcg_iterations is the oracle's count under the same cap, the whole
    step (camera part and back-substituted landmark part) is the oracle's capped step, and below k_conv the count EQUALS the cap
    while |S x - g_red| is still above the stopping threshold -- what a caller can use to tell an inexact step.  Then the
    speculation claim in bits: caps at, one past and far past the device's own converged count, and a repeat, give the same
    step and count."""
    prob, s, o = _pair(oracle, mode, variant, scaled)
    nc = prob.layout.cam_dof
    _, _, oS, ogred = o.solve_augmented(LAM, 0, want_schur=True)
    abs_tol = TOL * max(np.linalg.norm(ogred), 1.0)
    _, k_conv = _oracle_capped(o, variant, 5000)
    assert 1 < k_conv < 5000
    for k in dict.fromkeys((0, 1, 2, 3, 5, k_conv)):
        ostep, it_o = _oracle_capped(o, variant, k)
        step, it_g = _gpu_capped(s, k)
        res = float(np.linalg.norm(oS @ step[:nc] - ogred))
        err = rel(step, ostep)
        print(f"PCGCASE abi {mode} {variant.name}{' scaled' if scaled else ''} cap {k}: iterations gpu/oracle {it_g}/{it_o} "
              f"step vs oracle {err:.2e} |S x - g_red| {res:.2e} (abs_tol {abs_tol:.2e})")
        assert it_g == it_o, (k, it_g, it_o)
        assert np.isfinite(step).all() and err < STEP_TOL[variant], (k, err)
        if k < k_conv:
            assert it_g == k and res > abs_tol, (k, it_g, res, abs_tol)
        if k == 0:   # no camera step at all: the landmark part is the pure back-substitution Hll^-1 g_l (the oracle's, above)
            assert not step[:nc].any() and np.abs(step[nc:]).max() > 0
    step_inf, k_gpu = _gpu_capped(s, 5000)
    runs = {k: _gpu_capped(s, k) for k in (k_gpu, k_gpu + 1, 5000)}
    same = {k: (v[1] == k_gpu and v[0].tobytes() == step_inf.tobytes()) for k, v in runs.items()}
    print(f"PCGCASE abi {mode} {variant.name}{' scaled' if scaled else ''} bits: converged count {k_gpu} (oracle {k_conv}) caps {sorted(runs)}: {same}")
    assert all(same.values()), same
    s.close()


def test_sparse_request_on_a_refused_structure_runs_the_matrix_free_loop(oracle):
    """auto_variant hand-over: on the structure the plan refuses (tests/test_gpu_configs.py), a Sparse request is answered by
    the matrix-free loop at the reference's defaults (500, 1e-9): the same count and the same bits as an explicit Implicit
    request with those parameters."""
    d = pkg.synthetic.make_named("final-13682-mix:0.05", 0.02)
    prob = Problem.bundle_adjustment(d, OptimizationType.SelfCalibration, 1.0)
    steps = {}
    for variant in (SchurVariant.Sparse, SchurVariant.Implicit):
        s = GpuSchurComplementSolver(0).with_variant(variant)
        s.with_option("max_tile_updates", 50)
        s.initialize_structure(prob)
        s.set_parameters(d.poses, d.intr, d.points)
        if variant == SchurVariant.Implicit:
            s.with_cg_params(500, 1e-9)
        else:
            assert s.variant_info()["variant_used"] == "Implicit"
        step = s.solve_augmented_equation(1e-3)
        steps[variant] = (step, s.info()["pcg_iterations"])
        s.close()
    (a, ia), (b, ib) = steps[SchurVariant.Sparse], steps[SchurVariant.Implicit]
    print(f"PCGCASE abi auto_variant: iterations Sparse request {ia}, Implicit request {ib}, same bits {a.tobytes() == b.tobytes()}")
    assert 0 < ia <= 500 and ia == ib and a.tobytes() == b.tobytes()


@pytest.mark.parametrize("scaled", [False, True], ids=["plain", "jacobi_scaled"])
@pytest.mark.parametrize("variant", [SchurVariant.Iterative, SchurVariant.Implicit], ids=["iterative", "implicit"])
@pytest.mark.parametrize("mode", ["selfcal", "ba"])
def test_noise_free_problem_at_its_ground_truth(mode, variant, scaled):
    """The observations are the exact projections of the ground truth and the parameters ARE the ground truth, so the gradient
    is rounding noise and r.z, p.Ap and |r| of the loops sit next to their absolute thresholds (where 0/0 once reached x
    through the speculative iteration).  Whatever exit the loop takes: the step is finite, at most 1e-6 of the parameter
    norm, and the trial cost evaluates.  No count is asserted: by construction the thresholds are a knife edge here."""
    import np_ref

    d = pkg.synthetic.make_problem(30, 1500, 3, 7, config_id=77)
    uv, valid, _, _ = np_ref.project(d.truth_poses, d.truth_intr, d.truth_points, d.cam_idx.astype(np.int64), d.pt_idx.astype(np.int64))
    assert valid.all()
    d.obs_uv = np.ascontiguousarray(uv)
    d.poses, d.intr, d.points = (np.ascontiguousarray(a) for a in (d.truth_poses, d.truth_intr, d.truth_points))
    ot = OptimizationType.SelfCalibration if mode == "selfcal" else OptimizationType.BundleAdjustment
    prob = Problem.bundle_adjustment(d, ot, 1.0)
    s = GpuSchurComplementSolver(0).with_variant(variant)
    s.initialize_structure(prob)
    s.set_parameters(d.poses, d.intr, d.points)
    cost = s.compute_cost()
    scal = None
    if scaled:
        scal = 1.0 / (1.0 + s.compute_column_norms())
        s.apply_column_scaling(scal)
    x_norm = float(np.sqrt(sum(np.sum(np.square(a)) for a in (d.poses, d.intr, d.points))))
    for cg in ((200, 1e-6), (5000, TOL)):      # the reference's defaults of the explicit loop, and the tight setting of this file
        s.with_cg_params(*cg)
        step = s.solve_augmented_equation(LAM)
        grad = s.get_gradient()
        plain = step * scal if scaled else step   # (a scaled solve returns the step in the scaled variables)
        trial = s.eval_step()
        s.discard_step()
        print(f"PCGCASE abi ground truth {mode} {variant.name}{' scaled' if scaled else ''} cg {cg}: cost {cost:.3e} |grad| {np.linalg.norm(grad):.3e} "
              f"iterations {s.info()['pcg_iterations']} |step| {np.linalg.norm(plain):.3e} (|x| {x_norm:.3e}) trial cost {trial:.3e}")
        assert np.isfinite(step).all() and np.isfinite(grad).all() and np.isfinite(trial)
        assert np.linalg.norm(plain) <= 1e-6 * x_norm
    s.close()


def _two_islands(d, seed):
    """The counts of d with another plan: the landmarks alternate between cameras 0..15 (one tile at d_c = 9) and the rest,
    every landmark keeps its number of observations, drawn inside its island, so S is block diagonal -- two tile rows, no
    off-diagonal tile -- and every list and work array of the plan and of its PCG has another size."""
    import dataclasses

    rng = np.random.default_rng(seed)
    islands = (np.arange(0, 16), np.arange(16, d.n_cam))
    cam = d.cam_idx.copy()
    order = np.argsort(d.pt_idx, kind="stable")
    pts, first = np.unique(d.pt_idx[order], return_index=True)
    for l, a, b in zip(pts, first, list(first[1:]) + [len(order)]):
        cam[order[a:b]] = rng.choice(islands[int(l) % 2], size=b - a, replace=False)
    uv = pkg.synthetic.project_bal(d.truth_poses[cam], d.truth_intr[cam], d.truth_points[d.pt_idx]) + rng.normal(0, 0.7, (len(cam), 2))
    return dataclasses.replace(d, cam_idx=cam.astype(d.cam_idx.dtype), obs_uv=np.ascontiguousarray(uv))


def _both_variants(s, d, tiles):
    """Parameters set, then one solve per PCG variant: (step bytes, pcg_iterations) each."""
    s.set_parameters(d.poses, d.intr, d.points)
    s.with_cg_params(5000, TOL)
    out = []
    for variant in (SchurVariant.Iterative, SchurVariant.Implicit):
        step = s.with_variant(variant).solve_augmented_equation(LAM)
        assert np.isfinite(step).all() and s.info()["pcg_iterations"] > 1
        out.append((step.tobytes(), s.info()["pcg_iterations"]))
    info = s.info()
    assert info["tile_rows"] == 2 and info["tiles"] == tiles, info
    return out


def test_pcg_survives_a_rebuild():
    """A handle that has run both PCG loops is given another structure (reinitialize_structure: the same library handle, the
    plan released and built again over the PCG's lists, work arrays, pinned slots and events) and runs them again: every step
    and every pcg_iterations equal, byte for byte, those of a fresh handle given only the second problem.  A library handle
    keeps the counts it was created with, so the second problem cannot have fewer cameras: it has the first one's counts and a
    smaller plan instead -- two tiles (block diagonal) after three (two tile rows with their off-diagonal tile, which the
    gather needs).  Then back to the first structure on the same handle: the bytes of its first, fresh, run."""
    dA = pkg.synthetic.make_problem(30, 1500, 3, 7, config_id=77)
    dB = _two_islands(dA, 5)
    assert (dB.n_cam, dB.n_pt, dB.n_obs) == (dA.n_cam, dA.n_pt, dA.n_obs)
    problem = lambda d: Problem.bundle_adjustment(d, OptimizationType.SelfCalibration, 1.0)
    f = GpuSchurComplementSolver(0).initialize_structure(problem(dB))
    fresh = _both_variants(f, dB, 2)
    f.close()
    s = GpuSchurComplementSolver(0).initialize_structure(problem(dA))
    first = _both_variants(s, dA, 3)
    s.reinitialize_structure(problem(dB))
    again = _both_variants(s, dB, 2)
    s.reinitialize_structure(problem(dA))
    back = _both_variants(s, dA, 3)
    s.close()
    print(f"PCGCASE abi rebuild: iterations (Iterative, Implicit) three tiles {[i for _, i in first]}, two tiles on the same handle "
          f"{[i for _, i in again]} (fresh handle {[i for _, i in fresh]}), three tiles again {[i for _, i in back]}")
    assert again == fresh
    assert back == first
