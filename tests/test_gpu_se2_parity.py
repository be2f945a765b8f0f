"""SE2 pose graphs on the device, through the C ABI, against the numpy reference tests/np_ref_se2.py (needs a real MI355X:
`pytest -m gpu`).  Tolerances are the ones tests/test_gpu_pg_parity.py applies to the same quantities for SE3:
r, J, J^T J, J^T r <= 1e-12 relative; the step rel < 1e-10 where cond(H + lambda I) <= 1e5 (asserted on the numpy matrix)."""
import ctypes as C

import numpy as np
import pytest

import apex_solver_amd as pkg
import fixed_masks as fm
import np_ref_se2 as ref
from apex_solver_amd import capi
from apex_solver_amd.pose_graph import G2oLoader, GpuSparseCholeskySolver, PoseGraphProblem, write_g2o
from apex_solver_amd.solver import LevenbergMarquardt, LevenbergMarquardtConfig, LinearSolverType

pytestmark = pytest.mark.gpu


def rel(a, b):
    a = np.asarray(a, dtype=np.float64); b = np.asarray(b, dtype=np.float64)
    return float(np.linalg.norm(a - b) / max(np.linalg.norm(b), 1e-300))


def solver(prob, poses=None, **opts):
    s = GpuSparseCholeskySolver(0)
    for k, v in opts.items():
        s.with_option(k, v)
    s.initialize_structure(prob)
    s.set_parameters(prob.data.poses if poses is None else poses)
    return s


def lm_cfg(**kw):
    c = LevenbergMarquardtConfig.new().with_linear_solver_type(LinearSolverType.SparseCholesky)
    for k, v in kw.items():
        c = getattr(c, "with_" + k)(v)
    return c


INTEL = dict(max_iterations=100, cost_tolerance=1e-4, parameter_tolerance=1e-4, damping=1e-3)   # integration_tests.rs:243-247


def test_handle_reports_its_manifold():
    d = pkg.synthetic.make_manhattan(40)
    s = solver(PoseGraphProblem.pose_graph(d))
    out = (C.c_int * 3)()
    assert s._h.L.apexgpu_pg_manifold(s._h.h, C.byref(out)) == 0 and list(out) == [capi.MANIFOLD_SE2, 3, 3]
    assert s.info()["total_dof"] == 120
    s.close()
    g = pkg.synthetic.make_sphere(3, 4)
    s = solver(PoseGraphProblem.pose_graph(g))
    assert s._h.L.apexgpu_pg_manifold(s._h.h, C.byref(out)) == 0 and list(out) == [capi.MANIFOLD_SE3, 7, 6]
    s.close()


@pytest.mark.parametrize("huber", [None, 0.05], ids=["no-loss", "huber"])
@pytest.mark.parametrize("n", [40, 600])
def test_parity_with_numpy_reference(n, huber):
    d = pkg.synthetic.make_manhattan(n, id_stride=3)
    prob = PoseGraphProblem.pose_graph(d, huber)
    s = solver(prob)
    o = ref.Problem.from_problem(prob)
    r, J = o.edge_blocks()
    if huber:
        assert (np.einsum("ei,ei->e", *[ref.between_linearize(d.poses[d.e_from], d.poses[d.e_to], d.meas)[0]] * 2) > huber ** 2).any()
    gr, gJ = s.get_residual(), s.get_jacobian_blocks()
    print("r", rel(gr, r), "J", rel(gJ, J))
    assert rel(gr, r) < 1e-12 and rel(gJ, J) < 1e-12
    Ho, go = o.normal_equations()
    H, g = s.get_hessian(0.0)
    print("H", rel(H, Ho), "g", rel(g, go), "cost", abs(s.compute_cost() - o.cost()) / o.cost())
    assert rel(H, Ho) < 1e-12 and rel(g, go) < 1e-12
    assert s.compute_cost() == pytest.approx(o.cost(), rel=1e-12)
    for lam in (1e4, 1.0):
        cond = np.linalg.cond(Ho + lam * np.eye(o.n))
        assert cond <= 1e5, cond                      # the premise of the 1e-10 step bound, on the reference's matrix
        step = s.solve_augmented_equation(lam)
        so, _ = o.solve(lam)
        print(n, huber, lam, "cond", cond, "step", rel(step, so))
        assert rel(step, so) < 1e-10
        assert rel(s.get_gradient(), go) < 1e-12
    s.close()


@pytest.mark.parametrize("gauge", ["fixed-first-vertex", "huber-prior"])
def test_manhattan_3500_property_and_convergence(gauge):
    """Full size.  (J^T J + lambda I) dx = -J^T r with the Jacobian blocks the device exports (scipy sparse product; the
    prior rows from the numpy reference), held to the bound test_sphere2500_normal_equations_property uses, 1e-12 |g| --
    nothing of k_pg2_assemble enters the reference side.  Then the LM run as the reference's intel test asserts it
    (tests/integration_tests.rs:293-345) with its config."""
    import scipy.sparse as sp

    d = pkg.synthetic.make_manhattan(3500)
    assert (d.n_v, d.n_e) == (3500, 9378)
    if gauge == "huber-prior":
        prob = PoseGraphProblem(d).add_prior(f"x{int(d.ids[0])}", huber_delta=1.0)
    else:
        prob = PoseGraphProblem.pose_graph(d)
    s = solver(prob)
    lam = 1e-3
    step = s.solve_augmented_equation(lam)
    grad = s.get_gradient()
    J = s.get_jacobian_blocks(); r = s.get_residual()
    rows = (3 * np.arange(d.n_e)[:, None, None] + np.arange(3)[None, :, None] + np.zeros((1, 1, 6), int)).ravel()
    c0 = prob.pose_col[d.e_from][:, None] + np.arange(3)[None, :]
    c1 = prob.pose_col[d.e_to][:, None] + np.arange(3)[None, :]
    cols = np.broadcast_to(np.concatenate([c0, c1], axis=1)[:, None, :], (d.n_e, 3, 6)).ravel()
    Js = sp.csr_matrix((J.ravel(), (rows, cols)), shape=(3 * d.n_e, 3 * d.n_v))
    rv = r.ravel()
    if prob.priors:                                   # prior rows: sc I3 on the vertex's columns, corrected residual
        pr, psc = ref.Problem.from_problem(prob).prior_blocks()
        assert np.abs(s.get_prior_residual() - pr).max() <= 1e-13 * max(1.0, np.abs(pr).max())
        pi, pj, pv = [], [], []
        for k, (vtx, _, _) in enumerate(prob.priors):
            for a in range(3):
                pi.append(3 * k + a); pj.append(int(prob.pose_col[vtx]) + a); pv.append(psc[k])
        Jp = sp.csr_matrix((pv, (pi, pj)), shape=(3 * len(prob.priors), 3 * d.n_v))
        Js = sp.vstack([Js, Jp]).tocsr(); rv = np.concatenate([rv, pr.ravel()])
    g = Js.T @ rv
    print(gauge, "gradient rel", rel(grad, g))
    assert rel(grad, g) < 1e-12
    resid = Js.T @ (Js @ step) + lam * step + g
    print(gauge, "|J^T J dx + lambda dx + g| / |g|", np.linalg.norm(resid) / np.linalg.norm(g), s.info())
    assert np.linalg.norm(resid) <= 1e-12 * np.linalg.norm(g)
    s.close()
    res = LevenbergMarquardt.with_config(lm_cfg(**INTEL)).optimize(prob)
    imp = 100.0 * (res.initial_cost - res.final_cost) / res.initial_cost
    print(gauge, res.status, res.iterations, res.initial_cost, res.final_cost, imp)
    assert res.status.name in ("Converged", "CostToleranceReached", "ParameterToleranceReached", "GradientToleranceReached")
    assert imp > 85.0 and res.iterations < 100 and np.isfinite(res.final_cost)


@pytest.mark.parametrize("scaling", [False, True], ids=["plain", "jacobi-scaling"])
def test_lm_history_against_the_numpy_loop(scaling):
    d = pkg.synthetic.make_manhattan(600)
    prob = PoseGraphProblem.pose_graph(d)
    res = LevenbergMarquardt.with_config(lm_cfg(**INTEL).with_jacobi_scaling(scaling)).optimize(prob)
    o = ref.Problem.from_problem(prob).lm_optimize(use_jacobi_scaling=scaling, **INTEL)
    Hh = o["history"]
    print(res.status, res.iterations, o["status"], o["iterations"])
    assert res.status.value == o["status"] and res.iterations == o["iterations"]
    assert np.array_equal(res.history[:, 3], Hh[:, 3])
    assert np.allclose(res.history[:, 0], Hh[:, 0], rtol=1e-7) and np.allclose(res.history[:, 1], Hh[:, 1], rtol=1e-5 if not scaling else 1e-4)


def test_bit_reproducibility():
    d = pkg.synthetic.make_manhattan(600)
    prob = PoseGraphProblem.pose_graph(d, 0.05)
    s = solver(prob)
    H1, g1 = s.get_hessian(0.5); H2, g2 = s.get_hessian(0.5)
    assert np.array_equal(H1, H2) and np.array_equal(g1, g2)
    s.close()
    runs = []
    for _ in range(2):
        r = LevenbergMarquardt.with_config(lm_cfg(**INTEL)).optimize(prob)
        runs.append(r)
    assert np.array_equal(runs[0].history, runs[1].history) and np.array_equal(runs[0].parameters[0], runs[1].parameters[0])
    assert runs[0].iterations == runs[1].iterations and runs[0].final_cost == runs[1].final_cost


def test_switches_give_the_same_step():
    d = pkg.synthetic.make_manhattan(600)
    prob = PoseGraphProblem.pose_graph(d)
    steps = []
    for opts in ({}, {"graphs": 0}, {"tri_dataflow": 0}, {"nested_dissection": 0}):
        s = solver(prob, **opts)
        steps.append(s.solve_augmented_equation(1e-3).copy())
        s.close()
    for k in (1, 2, 3):
        print(k, rel(steps[k], steps[0]))
        assert rel(steps[k], steps[0]) < 1e-9            # test_nested_dissection_off_gives_the_same_step


SE2_MASKS = {"x-only": lambda n: _single(n, 0), "y-only": lambda n: _single(n, 1), "theta-only": lambda n: _single(n, 2),
             "mixed": lambda n: _mixed(n)}


def _single(n, dof):
    m = np.zeros((n, 3), np.uint8); m[n // 2 + 1, dof] = 1; m[n - 1, dof] = 1
    return m


def _mixed(n):
    rng = np.random.default_rng(61)
    m = np.zeros((n, 3), np.uint8)
    for k, v in enumerate(np.unique(np.concatenate([[1, n - 1], rng.choice(np.arange(2, n - 1), size=9, replace=False)]))):
        m[v] = fm._subset(k, 3)
    m[5, :] = 1
    return m


@pytest.mark.parametrize("scaled", [False, True], ids=["plain", "scaled"])
@pytest.mark.parametrize("pattern", sorted(SE2_MASKS))
def test_fixed_dofs_on_every_path_that_applies_a_step(pattern, scaled):
    d = pkg.synthetic.make_manhattan(600, id_stride=3)
    fix = SE2_MASKS[pattern](d.n_v)
    prob = fm.pg_apply_to_problem(PoseGraphProblem(d), fix)
    assert np.array_equal(prob.fix, fix)
    full = fix.astype(bool).all(axis=1)
    for eager in (1, 0):
        s = solver(prob, eager_step_eval=eager)
        s0 = solver(PoseGraphProblem(d), eager_step_eval=eager)
        scal = None
        if scaled:
            scal = 1.0 / (1.0 + s.compute_column_norms()); s.apply_column_scaling(scal); s0.apply_column_scaling(scal)
        p0 = s.get_parameters()
        y = s.solve_augmented_equation(1e-3).copy()
        y0 = s0.solve_augmented_equation(1e-3).copy()
        s0.close()
        # the mask acts when the step is applied, not in the solve; the row-owned assembly has a fixed order of
        # summation, so the step under the mask is the unmasked step bit for bit (SE3 holds this to its atomic bound)
        assert np.array_equal(y, y0)
        step = y if scal is None else s.apply_inverse_scaling(y)
        trial = s.eval_step(); s.discard_step()
        p1 = s.get_parameters()
        assert np.abs(p1 - p0).max() < 1e-9 and np.array_equal(p1[full], p0[full])
        y2 = s.solve_augmented_equation(1e-3).copy()
        step2 = y2 if scal is None else s.apply_inverse_scaling(y2)
        trial = s.eval_step(); s.commit_step()
        got = s.get_parameters()
        o = ref.Problem.from_problem(prob, poses=p1)
        o.apply_step(step2, 1.0)
        print(pattern, scaled, eager, "worst |gpu - numpy|", np.abs(got - o.poses).max())
        assert np.allclose(got, o.poses, rtol=1e-13, atol=1e-13)
        # all three DOF fixed: the vertex keeps its bits.  A vertex with theta alone fixed does not (theta (+) 0 still
        # goes through atan2(sin, cos) when x or y move, as t' = t + R V rho moves a fixed translation DOF for SE3):
        # those follow the numpy retraction above.
        assert np.array_equal(got[full], p0[full])
        assert trial == pytest.approx(o.cost(), rel=1e-13)
        s.close()
    res = LevenbergMarquardt.with_config(lm_cfg(max_iterations=8).with_jacobi_scaling(scaled)).optimize(prob)
    assert np.array_equal(res.parameters[0][full], ref.Problem.from_problem(prob).poses[full])
    oo = ref.Problem.from_problem(prob).lm_optimize(max_iterations=8, use_jacobi_scaling=scaled)
    assert res.iterations == oo["iterations"] and np.array_equal(res.history[:, 3], oo["history"][:, 3])
    assert np.allclose(res.history[:, 0], oo["history"][:, 0], rtol=1e-7)


@pytest.mark.parametrize("delta", [None, 0.3])
def test_priors_and_their_residual_export(delta):
    d = pkg.synthetic.make_manhattan(200)
    prob = PoseGraphProblem(d, huber_delta=0.05)
    prob.add_prior("x0", huber_delta=delta)
    prob.add_prior("x77", data=d.poses[77] + np.array([0.5, -0.4, 0.2]), huber_delta=delta)
    prob.add_prior("x77", data=d.poses[77] + np.array([0.0, 0.1, -0.1]), huber_delta=None)      # two blocks on one vertex
    s = solver(prob)
    o = ref.Problem.from_problem(prob)
    pr, _ = o.prior_blocks()
    assert rel(s.get_prior_residual(), pr) < 1e-13
    Ho, go = o.normal_equations()
    H, g = s.get_hessian(0.0)
    assert rel(H, Ho) < 1e-12 and rel(g, go) < 1e-12
    assert s.compute_cost() == pytest.approx(o.cost(), rel=1e-12)
    assert np.linalg.cond(Ho + 1.0 * np.eye(o.n)) <= 1e5
    assert rel(s.solve_augmented_equation(1.0), o.solve(1.0)[0]) < 1e-10
    s.close()


def test_rejected_step_singular_matrix_and_wrong_state_calls():
    d = pkg.synthetic.make_manhattan(200)
    prob = PoseGraphProblem.pose_graph(d)
    s = GpuSparseCholeskySolver(0).initialize_structure(prob)
    with pytest.raises(capi.LinAlgError) as e:
        s.compute_cost()
    assert e.value.kind == "InvalidState"
    s.set_parameters(d.poses)
    with pytest.raises(capi.LinAlgError) as e:
        s.eval_step()
    assert e.value.kind == "InvalidState"
    with pytest.raises(capi.LinAlgError) as e:
        s.commit_step()
    assert e.value.kind == "InvalidState"
    p0 = s.get_parameters()
    s.solve_augmented_equation(1e-3); s.eval_step(); s.discard_step()
    assert np.abs(s.get_parameters() - p0).max() < 1e-9
    s.close()
    # no gauge, lambda = 0, and vertices no edge touches: exact zero pivots (the graph of test_singular_matrix_is_reported)
    from apex_solver_amd.synthetic import PoseGraphData
    free = PoseGraphProblem(PoseGraphData(ids=d.ids, poses=d.truth, e_from=d.e_from[:1], e_to=d.e_to[:1], meas=d.meas[:1]))
    s = solver(free)
    with pytest.raises(capi.LinAlgError) as e:
        s.solve_augmented_equation(0.0)
    assert e.value.kind == "SingularMatrix" and "Cholesky factorization failed" in str(e.value)
    s.solve_augmented_equation(1e-3)                             # the handle stays usable
    s.close()


def test_tiny_and_degenerate_graphs():
    z = np.zeros((0,), np.uint32)
    from apex_solver_amd.synthetic import PoseGraphData
    # empty edge list: H = lambda I, g = 0
    d = PoseGraphData(ids=np.arange(5), poses=np.random.default_rng(0).uniform(-1, 1, (5, 3)), e_from=z, e_to=z, meas=np.zeros((0, 3)))
    s = solver(PoseGraphProblem(d))
    H, g = s.get_hessian(0.5)
    assert np.array_equal(H, 0.5 * np.eye(15)) and np.array_equal(g, np.zeros(15)) and s.compute_cost() == 0.0
    assert np.array_equal(s.solve_augmented_equation(0.5), np.zeros(15))
    s.close()
    # two vertices; a self-loop and duplicate edges (both directions)
    rng = np.random.default_rng(3)
    for ef, et, nv in (([0], [1], 2), ([0, 1, 0, 2, 2, 1], [1, 0, 1, 2, 3, 3], 4)):
        d = PoseGraphData(ids=np.arange(nv) * 2, poses=rng.uniform(-2, 2, (nv, 3)), e_from=np.array(ef, np.uint32), e_to=np.array(et, np.uint32),
                          meas=rng.uniform(-1, 1, (len(ef), 3)))
        prob = PoseGraphProblem(d)
        s = solver(prob); o = ref.Problem.from_problem(prob)
        Ho, go = o.normal_equations()
        H, g = s.get_hessian(0.5)
        assert rel(H, Ho + 0.5 * np.eye(o.n)) < 1e-12 and rel(g, go) < 1e-12
        assert rel(s.get_residual(), o.edge_blocks()[0]) < 1e-12
        assert rel(s.solve_augmented_equation(0.5), o.solve(0.5)[0]) < 1e-10
        s.close()


def test_theta_comes_back_in_range_after_a_step_across_pi():
    from apex_solver_amd.synthetic import PoseGraphData
    poses = np.array([[0.0, 0.0, np.pi - 0.02], [1.0, 0.0, -np.pi + 0.03], [2.0, 0.5, 3.0 * np.pi + 0.1]])
    meas = np.array([[1.0, 0.0, 0.2], [1.0, 0.5, -0.3], [2.0, 0.4, 0.1]])
    d = PoseGraphData(ids=np.arange(3), poses=poses, e_from=np.array([0, 1, 0], np.uint32), e_to=np.array([1, 2, 2], np.uint32), meas=meas)
    prob = PoseGraphProblem(d)
    s = solver(prob)
    p = s.get_parameters()
    assert np.array_equal(p[:2], poses[:2]) and abs(p[2, 2] - (np.pi + 0.1 - 2 * np.pi)) < 1e-14     # held as SE2 -> DVector gives it
    o = ref.Problem.from_problem(prob)
    step = s.solve_augmented_equation(1e-2); s.eval_step(); s.commit_step()
    got = s.get_parameters()
    o.apply_step(step, 1.0)
    assert ((got[:, 2] > -np.pi) & (got[:, 2] <= np.pi)).all() and np.allclose(got, o.poses, rtol=1e-13, atol=1e-13)
    assert (np.sign(got[:, 2]) != np.sign(p[:, 2])).any()                                             # one of them crossed
    s.close()


def test_g2o_end_to_end(tmp_path):
    d = pkg.synthetic.make_manhattan(200, id_stride=5)
    path = tmp_path / "m200.g2o"
    write_g2o(path, d)
    q = G2oLoader.load(path).to_problem_data()
    out = []
    for data in (d, q):
        res = LevenbergMarquardt.with_config(lm_cfg(**INTEL)).optimize(PoseGraphProblem.pose_graph(data))
        out.append(res)
    assert np.array_equal(out[0].history, out[1].history) and np.array_equal(out[0].parameters[0], out[1].parameters[0])
    assert out[0].final_cost < 0.15 * out[0].initial_cost


def test_se3_handles_around_an_se2_one_still_reproduce_the_golden():
    """The shared class does not leak state between manifolds: tests/golden/pg_sphere_8x12.npz before and after an SE2 handle."""
    import os
    from test_gpu_pg_parity import problem_from_fixture

    g = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "pg_sphere_8x12.npz"))

    def se3_once():
        s = GpuSparseCholeskySolver().initialize_structure(problem_from_fixture(g))
        s.set_parameters(g["it0_poses"])
        assert rel(s.get_residual(), g["it0_r"]) < 1e-12 and rel(s.get_jacobian_blocks(), g["it0_J"]) < 1e-12
        step = s.solve_augmented_equation(float(g["it0_lambda"])).copy()
        assert rel(s.get_gradient(), g["it0_grad"]) < 1e-12
        s.close()
        return step

    s1 = se3_once()
    d = pkg.synthetic.make_manhattan(100)
    s = solver(PoseGraphProblem.pose_graph(d)); s.solve_augmented_equation(1e-3); s.eval_step(); s.commit_step(); s.close()
    s2 = se3_once()
    assert rel(s2, s1) < 1e-9
