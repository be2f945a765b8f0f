"""GPU parity of the SE3 pose-graph backend (BASELINE.json configs[1]) through the C ABI
(apexgpu_pg_*) against the oracle, the committed golden fixtures and size-independent properties at
sphere2500 scale.  Tolerances: r, J, J^T J, J^T r <= 1e-12 relative; the step within
1e-10 (the north star's figure; cond(H + lambda I) <= 1e5 on these graphs, measured 1e-13 .. 1e-12) with backward error <= 1e-13."""
import os

import numpy as np
import pytest

import apex_solver_amd as pkg
from apex_solver_amd.pose_graph import G2oLoader, GpuSparseCholeskySolver, PoseGraphProblem, write_g2o
from apex_solver_amd.solver import LevenbergMarquardt, LevenbergMarquardtConfig, LinearSolverType, OptimizationStatus
from oracle import pg_oracle as po

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
EPS = np.finfo(np.float64).eps
STEP_FORWARD_BOUND = 1e-10   # |step - oracle step| / |oracle step|: the north star's figure, fixed (not scaled by cond)


def rel(a, b):
    return float(np.linalg.norm(np.ravel(a) - np.ravel(b)) / max(np.linalg.norm(np.ravel(b)), 1e-300))


def problem_from_fixture(g):
    d = pkg.synthetic.PoseGraphData(ids=g["ids"], poses=g["poses0"], e_from=g["e_from"], e_to=g["e_to"], meas=g["meas"])
    hub = None if float(g["huber_delta"]) <= 0 else float(g["huber_delta"])
    p = PoseGraphProblem(d, hub, fix=g["fix"].copy())
    assert np.array_equal(p.pose_col, g["pose_col"])
    return p


@pytest.mark.parametrize("name", ["pg_sphere_8x12", "pg_sphere_10x10_huber"])
def test_golden_iterations(name):
    g = np.load(os.path.join(HERE, "golden", name + ".npz"))
    prob = problem_from_fixture(g)
    s = GpuSparseCholeskySolver().initialize_structure(prob)
    s.set_parameters(g["poses0"])
    assert abs(s.compute_cost() - float(g["initial_cost"])) <= 1e-12 * float(g["initial_cost"])
    for it in range(int(g["iters"])):
        s.set_parameters(g[f"it{it}_poses"])
        lam = float(g[f"it{it}_lambda"])
        assert rel(s.get_residual(), g[f"it{it}_r"]) < 1e-12
        assert rel(s.get_jacobian_blocks(), g[f"it{it}_J"]) < 1e-12
        step = s.solve_augmented_equation(lam)
        assert rel(s.get_gradient(), g[f"it{it}_grad"]) < 1e-12
        tol = STEP_FORWARD_BOUND
        assert rel(step, g[f"it{it}_step"]) < tol
        gn, sn, pred = s.step_stats()
        assert abs(pred - float(g[f"it{it}_pred"])) <= 1e-9 * abs(pred)
        assert abs(sn - np.linalg.norm(g[f"it{it}_step"])) <= 1e-9 * sn
        nc = s.eval_step()
        assert abs(nc - float(g[f"it{it}_new_cost"])) <= 1e-9 * nc
        s.discard_step()
    s.close()


@pytest.mark.parametrize("name", ["pg_sphere_8x12", "pg_sphere_10x10_huber"])
def test_golden_lm_history(name):
    g = np.load(os.path.join(HERE, "golden", name + ".npz"))
    prob = problem_from_fixture(g)
    cfg = LevenbergMarquardtConfig.new().with_max_iterations(10).with_linear_solver_type(LinearSolverType.SparseCholesky)
    res = LevenbergMarquardt.with_config(cfg).optimize(prob)
    assert res.status.value == int(g["lm_status"]) and res.iterations == int(g["lm_iterations"])
    H = g["lm_history"]
    assert np.allclose(res.history[:, 3], H[:, 3])                       # accept / reject pattern
    assert np.allclose(res.history[:, 0], H[:, 0], rtol=1e-7)            # cost after each iteration
    assert np.allclose(res.history[:, 1], H[:, 1], rtol=1e-5)            # damping
    assert abs(res.final_cost - float(g["lm_final_cost"])) <= 1e-7 * res.final_cost


@pytest.mark.parametrize("huber", [None, 0.8])
def test_oracle_parity_mid_size(huber):
    d = pkg.synthetic.make_sphere(20, 30, id_stride=3)     # 600 vertices: 25 tiles, nested dissection active
    prob = PoseGraphProblem.pose_graph(d, huber)
    o = po.PgOracle.from_problem(prob)
    s = GpuSparseCholeskySolver().initialize_structure(prob)
    s.set_parameters(d.poses)
    c, r, J = o.linearize()
    assert abs(s.compute_cost() - c) <= 1e-12 * c
    assert rel(s.get_residual(), r) < 1e-12 and rel(s.get_jacobian_blocks(), J) < 1e-12
    lam = 1e-3
    H, g = s.get_hessian(lam)
    Ho, go = o.normal_equations()
    Ho += lam * np.eye(Ho.shape[0])
    assert rel(H, Ho) < 1e-12 and rel(g, go) < 1e-12
    step = s.solve_augmented_equation(lam)
    rc, so, _ = o.solve_augmented(lam)
    assert rc == 0
    cond = np.linalg.cond(Ho)
    assert rel(step, so) < STEP_FORWARD_BOUND, (rel(step, so), cond)
    assert np.linalg.norm(Ho @ step + go) <= 1e-13 * (np.linalg.norm(Ho, 2) * np.linalg.norm(step) + np.linalg.norm(go))
    info = s.info()
    assert info["tile_rows"] == 25 and info["total_dof"] == 3600
    s.close()


def test_sphere2500_normal_equations_property():
    """BASELINE.json configs[1] at full size: (J^T J + lambda I) dx = -J^T r checked with the Jacobian the
    device exports (scipy sparse product), and the oracle's envelope Cholesky on the same input."""
    import scipy.sparse as sp

    d = pkg.synthetic.make_sphere()
    assert (d.n_v, d.n_e) == (2500, 4949)
    prob = PoseGraphProblem.pose_graph(d)
    s = GpuSparseCholeskySolver().initialize_structure(prob)
    s.set_parameters(d.poses)
    lam = 1e-3
    step = s.solve_augmented_equation(lam)
    grad = s.get_gradient()
    J = s.get_jacobian_blocks(); r = s.get_residual()
    rows = (6 * np.arange(d.n_e)[:, None, None] + np.arange(6)[None, :, None] + np.zeros((1, 1, 12), int)).ravel()
    c0 = prob.pose_col[d.e_from][:, None] + np.arange(6)[None, :]
    c1 = prob.pose_col[d.e_to][:, None] + np.arange(6)[None, :]
    cols = np.broadcast_to(np.concatenate([c0, c1], axis=1)[:, None, :], (d.n_e, 6, 12)).ravel()
    Js = sp.csr_matrix((J.ravel(), (rows, cols)), shape=(6 * d.n_e, 6 * d.n_v))
    g = Js.T @ r.ravel()
    assert rel(grad, g) < 1e-12
    resid = Js.T @ (Js @ step) + lam * step + g
    assert np.linalg.norm(resid) <= 1e-12 * np.linalg.norm(g)
    o = po.PgOracle.from_problem(prob)
    o.linearize()
    rc, so, go = o.solve_augmented(lam)
    assert rc == 0 and rel(grad, go) < 1e-12
    assert rel(step, so) < 1e-8
    s.close()


def test_sphere2500_lm_converges_like_the_oracle():
    """integration_tests.rs:293-469 asserts for sphere2500: converged, > 99 % cost reduction, < 20 iterations
    -- with the real dataset; the synthetic sphere is held to the oracle's own trajectory instead."""
    d = pkg.synthetic.make_sphere()
    prob = PoseGraphProblem.pose_graph(d)
    cfg = (LevenbergMarquardtConfig.new().with_max_iterations(100).with_cost_tolerance(1e-4).with_parameter_tolerance(1e-4)
           .with_linear_solver_type(LinearSolverType.SparseCholesky))       # bin/pose_graph_g2o.rs:933-938
    res = LevenbergMarquardt.with_config(cfg).optimize(prob)
    o = po.PgOracle.from_problem(prob)
    ref = o.lm_optimize(po.lm_config(max_iterations=100, cost_tolerance=1e-4, parameter_tolerance=1e-4), hist_rows=128)
    assert res.status.value == ref["status"] and res.iterations == ref["iterations"]
    assert abs(res.initial_cost - ref["initial_cost"]) <= 1e-12 * ref["initial_cost"]
    assert abs(res.final_cost - ref["final_cost"]) <= 1e-6 * ref["final_cost"]
    assert res.final_cost < 0.01 * res.initial_cost
    assert res.status in (OptimizationStatus.CostToleranceReached, OptimizationStatus.ParameterToleranceReached,
                          OptimizationStatus.GradientToleranceReached)


def test_rejected_step_and_fixed_vertex():
    d = pkg.synthetic.make_sphere(10, 12)
    prob = PoseGraphProblem.pose_graph(d)
    s = GpuSparseCholeskySolver().initialize_structure(prob)
    s.set_parameters(d.poses)
    p0 = s.get_parameters()
    step = s.solve_augmented_equation(1e-3)
    assert np.abs(step[prob.pose_col[0]:prob.pose_col[0] + 6]).max() > 0     # the fixed vertex still gets a step ...
    s.eval_step(); s.commit_step()
    p1 = s.get_parameters()
    assert np.array_equal(p1[0, :3], p0[0, :3])                               # ... that is masked when applied
    o = po.PgOracle.from_problem(prob); o.apply_step(step, 1.0)
    assert np.abs(p1 - o.get_params()).max() < 1e-12
    s.solve_augmented_equation(1e-3); s.eval_step(); s.discard_step()        # inverse retraction
    assert np.abs(s.get_parameters() - p1).max() < 1e-9
    s.close()


def test_singular_matrix_is_reported():
    d = pkg.synthetic.make_sphere(4, 6)
    prob = PoseGraphProblem(pkg.synthetic.PoseGraphData(ids=d.ids, poses=d.truth, e_from=d.e_from[:1], e_to=d.e_to[:1], meas=d.meas[:1]))
    s = GpuSparseCholeskySolver().initialize_structure(prob)
    s.set_parameters(d.truth)
    with pytest.raises(pkg.capi.LinAlgError) as e:
        s.solve_augmented_equation(0.0)
    assert e.value.kind == "SingularMatrix" and "Cholesky factorization failed" in str(e.value)
    s.solve_augmented_equation(1e-3)     # the handle stays usable
    s.close()


def test_error_behaviour():
    s = GpuSparseCholeskySolver()
    with pytest.raises(pkg.capi.LinAlgError) as e:
        s.set_parameters(np.zeros((2, 7)))
    assert e.value.kind == "InvalidState"
    d = pkg.synthetic.make_sphere(3, 4)
    bad = pkg.synthetic.PoseGraphData(ids=d.ids, poses=d.poses, e_from=np.array([0], np.uint32), e_to=np.array([99], np.uint32), meas=d.meas[:1])
    with pytest.raises(pkg.capi.LinAlgError) as e:
        GpuSparseCholeskySolver().initialize_structure(PoseGraphProblem(bad))
    assert e.value.kind == "InvalidInput"
    s2 = GpuSparseCholeskySolver().initialize_structure(PoseGraphProblem.pose_graph(d))
    with pytest.raises(pkg.capi.LinAlgError) as e:
        s2.step_stats()
    assert e.value.kind == "InvalidState"


def test_nested_dissection_off_gives_the_same_step():
    d = pkg.synthetic.make_sphere(25, 40)
    prob = PoseGraphProblem.pose_graph(d)
    steps = []
    for nd in (0, 1, 8):
        s = GpuSparseCholeskySolver().with_option("nested_dissection", nd).initialize_structure(prob)
        s.set_parameters(d.poses)
        steps.append(s.solve_augmented_equation(1e-3))
        s.close()
    assert rel(steps[1], steps[0]) < 1e-9 and rel(steps[2], steps[0]) < 1e-9


def test_g2o_end_to_end(tmp_path):
    d = pkg.synthetic.make_sphere(12, 15, id_stride=2)
    path = tmp_path / "sphere.g2o"
    write_g2o(path, d)
    g = G2oLoader.load(path)
    prob = PoseGraphProblem.pose_graph(g.to_problem_data())
    cfg = LevenbergMarquardtConfig.new().with_max_iterations(30).with_linear_solver_type(LinearSolverType.SparseCholesky)
    res = LevenbergMarquardt.with_config(cfg).optimize(prob)
    o = po.PgOracle.from_problem(PoseGraphProblem.pose_graph(d))
    ref = o.lm_optimize(po.lm_config(max_iterations=30))
    assert res.iterations == ref["iterations"] and abs(res.final_cost - ref["final_cost"]) <= 1e-6 * ref["final_cost"]
    assert res.final_cost < res.initial_cost


def test_tiny_and_degenerate_graphs():
    """2 vertices / 1 edge (one tile, no nested dissection), an isolated vertex (kept finite by the damping),
    a multi-edge and a self-loop: the assembled J^T J equals the oracle's."""
    d = pkg.synthetic.make_sphere(3, 4)
    for ef, et, nv in (([0], [1], 2), ([0, 1, 1, 2, 3, 3], [1, 2, 2, 3, 3, 0], 5)):
        data = pkg.synthetic.PoseGraphData(ids=np.arange(nv, dtype=np.int64), poses=d.truth[:nv].copy(),
                                           e_from=np.asarray(ef, np.uint32), e_to=np.asarray(et, np.uint32), meas=d.meas[:len(ef)].copy())
        prob = PoseGraphProblem.pose_graph(data)
        s = GpuSparseCholeskySolver().initialize_structure(prob)
        s.set_parameters(data.poses)
        o = po.PgOracle.from_problem(prob)
        c, r, J = o.linearize()
        assert abs(s.compute_cost() - c) <= 1e-12 * c
        H, g = s.get_hessian(0.5)
        Ho, go = o.normal_equations()
        assert rel(H, Ho + 0.5 * np.eye(Ho.shape[0])) < 1e-12 and rel(g, go) < 1e-12
        step = s.solve_augmented_equation(0.5)
        assert np.linalg.norm((Ho + 0.5 * np.eye(Ho.shape[0])) @ step + go) <= 1e-12 * max(np.linalg.norm(go), 1e-30)
        s.close()


def test_empty_edge_list_is_an_identity_system():
    d = pkg.synthetic.make_sphere(3, 4)
    data = pkg.synthetic.PoseGraphData(ids=d.ids, poses=d.poses, e_from=np.zeros(0, np.uint32), e_to=np.zeros(0, np.uint32), meas=np.zeros((0, 7)))
    s = GpuSparseCholeskySolver().initialize_structure(PoseGraphProblem.pose_graph(data))
    s.set_parameters(d.poses)
    assert s.compute_cost() == 0.0
    step = s.solve_augmented_equation(1e-3)
    assert np.all(step == 0.0)
    s.close()


# ---- Jacobi column scaling (optimizer/mod.rs:749-763; linearizer/mod.rs:229-262) -----------------------------
@pytest.mark.parametrize("huber", [None, 0.8])
def test_jacobi_scaling_vs_oracle(huber):
    d = pkg.synthetic.make_sphere(20, 30, id_stride=3)
    prob = PoseGraphProblem.pose_graph(d, huber)
    o = po.PgOracle.from_problem(prob)
    s = GpuSparseCholeskySolver().initialize_structure(prob)
    s.set_parameters(d.poses)
    o.linearize()
    norms, onorms = s.compute_column_norms(), o.column_norms()
    assert rel(norms, onorms) < 1e-12
    scal = 1.0 / (1.0 + onorms)
    s.apply_column_scaling(scal); o.set_column_scaling(scal)
    lam = 1e-3
    Ho, go = o.normal_equations()
    Hs = Ho * scal[:, None] * scal[None, :] + lam * np.eye(len(go))
    H, g = s.get_hessian(lam)
    assert rel(H, Hs) < 1e-12 and rel(g, scal * go) < 1e-12
    y = s.solve_augmented_equation(lam)
    rc, yo, gso = o.solve_augmented(lam)
    assert rc == 0 and rel(s.get_gradient(), gso) < 1e-12
    assert rel(y, yo) < STEP_FORWARD_BOUND
    assert np.linalg.norm(Hs @ y + scal * go) <= 1e-13 * (np.linalg.norm(Hs, 2) * np.linalg.norm(y) + np.linalg.norm(go))
    step = yo * scal
    gn, sn, pred = s.step_stats()   # compute_step_generic: scaled gradient, unscaled step
    assert abs(gn - np.linalg.norm(gso)) <= 1e-12 * gn and abs(sn - np.linalg.norm(step)) <= 1e-8 * sn
    assert abs(pred - 0.5 * step @ (lam * step - gso)) <= 1e-7 * abs(pred)
    o.apply_step(step, 1.0)
    assert abs(s.eval_step() - o.residuals()[0]) <= 1e-9 * o.residuals()[0]
    s.discard_step()
    s.apply_column_scaling(None)
    o.apply_step(step, -1.0); o.set_column_scaling(None); o.linearize()
    rc, so, _ = o.solve_augmented(lam)
    assert rel(s.solve_augmented_equation(lam), so) < 1e-7
    s.close()


def test_jacobi_scaling_lm_history_vs_oracle():
    d = pkg.synthetic.make_sphere(12, 16)
    prob = PoseGraphProblem.pose_graph(d)
    cfg = (LevenbergMarquardtConfig.new().with_max_iterations(15).with_jacobi_scaling(True)
           .with_linear_solver_type(LinearSolverType.SparseCholesky))
    res = LevenbergMarquardt.with_config(cfg).optimize(prob)
    o = po.PgOracle.from_problem(prob)
    ref = o.lm_optimize(po.lm_config(max_iterations=15, use_jacobi_scaling=True))
    assert res.status.value == ref["status"] and res.iterations == ref["iterations"]
    H = ref["history"]
    assert np.allclose(res.history[:, 3], H[:, 3])
    assert np.allclose(res.history[:, 0], H[:, 0], rtol=1e-7) and np.allclose(res.history[:, 4], H[:, 4], rtol=1e-6)
    assert np.allclose(res.history[:, 1], H[:, 1], rtol=1e-4)
    assert res.final_cost < 0.05 * res.initial_cost


@pytest.mark.parametrize("delta", [None, 1.0, 0.05])
def test_prior_factor_blocks_vs_oracle(delta):
    """PriorFactor blocks (prior_factor.rs:96-108; the gauge of tests/integration_tests.rs:98-118) through
    apexgpu_pg_set_priors: cost, prior residuals, J^T J, J^T r and the step against the oracle (which
    tests/test_pg_prior_factor.py pins against a dense restatement), nothing fixed, loss active and inactive."""
    from apex_solver_amd.pose_graph import se3_as_vector

    d = pkg.synthetic.make_sphere(12, 20, id_stride=2)
    rng = np.random.default_rng(4)
    prob = PoseGraphProblem(d, huber_delta=0.7)
    x0 = se3_as_vector(d.poses[0]); x0[:3] += 0.2 * rng.standard_normal(3); x0[3:] += 0.05 * rng.standard_normal(4)
    prob.add_prior(f"x{int(d.ids[0])}", data=x0, huber_delta=delta)
    prob.add_prior(f"x{int(d.ids[77])}", huber_delta=delta)
    o = po.PgOracle.from_problem(prob)
    s = GpuSparseCholeskySolver().initialize_structure(prob)
    s.set_parameters(d.poses)
    c, r, J = o.linearize()
    assert abs(s.compute_cost() - c) <= 1e-12 * c
    assert rel(s.get_prior_residual(), o.prior_residuals()) < 1e-13
    assert rel(s.get_residual(), r) < 1e-12
    lam = 1e-4
    H, g = s.get_hessian(lam)
    Ho, go = o.normal_equations()
    Ho += lam * np.eye(Ho.shape[0])
    assert rel(H, Ho) < 1e-12 and rel(g, go) < 1e-12
    assert rel(s.compute_column_norms(), o.column_norms()) < 1e-12
    step = s.solve_augmented_equation(lam)
    rc, so, _ = o.solve_augmented(lam)
    assert rc == 0 and rel(step, so) < 1e-9, rel(step, so)
    # trial cost includes the priors at the trial point
    nc = s.eval_step()
    o.apply_step(so, 1.0)
    assert abs(nc - o.residuals()[0]) <= 1e-8 * nc
    s.discard_step()
    # without damping the priors alone must hold the gauge
    assert np.all(np.isfinite(s.solve_augmented_equation(0.0)))
    s.close()


def test_lm_with_prior_gauge_matches_the_oracle_loop():
    d = pkg.synthetic.make_sphere(10, 12, config_id=9)
    prob = PoseGraphProblem(d).add_prior(f"x{int(d.ids[0])}", huber_delta=1.0)
    o = po.PgOracle.from_problem(prob)
    ref = o.lm_optimize(po.lm_config(max_iterations=30))
    cfg = LevenbergMarquardtConfig.new().with_max_iterations(30).with_linear_solver_type(LinearSolverType.SparseCholesky)
    res = LevenbergMarquardt.with_config(cfg).optimize(prob)
    assert res.iterations == ref["iterations"]
    assert abs(res.initial_cost - ref["initial_cost"]) <= 1e-12 * ref["initial_cost"]
    assert abs(res.final_cost - ref["final_cost"]) <= 1e-7 * ref["final_cost"]
    assert res.final_cost < 0.5 * res.initial_cost


# ---- the grid-stride pass of the cost kernel ------------------------------------------------------------------
def _random_path_graph(manifold, n_v, seed):
    """Vertices 0 .. n_v - 1 in a path (edge i: i -> i + 1; block-tridiagonal, no fill), random poses and measurements."""
    rng = np.random.default_rng(seed)

    def poses(n):
        if manifold == "se2":
            return np.column_stack([10.0 * rng.standard_normal((n, 2)), rng.uniform(-np.pi, np.pi, n)])
        q = rng.standard_normal((n, 4))
        return np.column_stack([10.0 * rng.standard_normal((n, 3)), q / np.linalg.norm(q, axis=1, keepdims=True)])

    e = np.arange(n_v - 1, dtype=np.uint32)
    return pkg.synthetic.PoseGraphData(ids=np.arange(n_v, dtype=np.int64), poses=poses(n_v), e_from=e, e_to=e + 1, meas=poses(n_v - 1))


def _path_slice(d, v0, v1):
    """The sub-path on vertices v0 .. v1 inclusive: edges v0 .. v1 - 1 of d with their poses and measurements."""
    e = np.arange(v1 - v0, dtype=np.uint32)
    return pkg.synthetic.PoseGraphData(ids=d.ids[v0:v1 + 1], poses=d.poses[v0:v1 + 1], e_from=e, e_to=e + 1, meas=d.meas[v0:v1])


def _device_cost(d):
    s = GpuSparseCholeskySolver().initialize_structure(PoseGraphProblem(d))
    s.set_parameters(d.poses)
    c = s.compute_cost()
    s.close()
    return c


@pytest.mark.parametrize("manifold", ["se3", "se2"])
def test_cost_grid_stride_pass_equals_the_sum_of_single_pass_parts(manifold):
    """The cost kernel runs 256 blocks of 256 threads, so only a graph above 65,536 edges sends a thread round its
    grid-stride loop a second time -- every other graph of the suite stays below.  A path of 66,000 vertices (65,999
    edges) against the device's own cost of the same edges in two handles of 33,000 and 32,999 edges, each one pass (the
    path the numpy references and the oracle pin): equal to rel 1e-13, a few ulp over 66,000 non-negative terms summed by
    two different fixed trees.  No solve: set_structure, set_params, cost."""
    n_v = 66000
    d = _random_path_graph(manifold, n_v, seed=11)
    assert d.n_e == 65999 > 256 * 256
    mid = 33000
    parts = [_device_cost(_path_slice(d, 0, mid)), _device_cost(_path_slice(d, mid, n_v - 1))]
    whole = _device_cost(d)
    print(f"{manifold}: whole {whole!r}  parts {parts!r}  rel {abs(whole - sum(parts)) / sum(parts):.3e}")
    assert parts[0] > 0.0 and parts[1] > 0.0
    assert abs(whole - sum(parts)) <= 1e-13 * sum(parts)
