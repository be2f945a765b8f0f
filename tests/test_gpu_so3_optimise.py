"""SO3 pose graphs on the device: the three optimiser loops, the loss family, information matrices, the Dog-Leg products and
marginal covariances, against tests/so3_ref.py (needs a real MI355X: `pytest -m gpu`).

The loops are held to a float64 numpy restatement of the same loop over so3_ref (np_ref_se2.Problem.lm_optimize,
np_ref_trust_region.gauss_newton / dog_leg on so3_ref.So3Problem) at the tolerances the SE2 loop tests use: the same status,
iteration count and accept / reject decisions, cost rtol 1e-7, LM damping rtol 1e-5, Dog-Leg radius rtol 1e-7.  The gauge is
fixed as the SE2 tests of the same loop fix theirs: LM with the three DOF of the first vertex fixed (PoseGraphProblem.pose_graph,
tests/test_gpu_se2_parity.py), Gauss-Newton and Dog-Leg with a prior on the first vertex (tests/tr_cases.py: a fixed DOF stays
in the linear system, so without a prior J^T J is singular and Gauss-Newton has nothing to factorise)."""
import numpy as np
import pytest

import apex_solver_amd as pkg
import np_ref_trust_region as tr
import so3_ref as sr
from apex_solver_amd.pose_graph import (DogLegConfig, GaussNewtonConfig, GpuSparseCholeskySolver, PoseGraphProblem,
                                        create_loss_function)
from apex_solver_amd.solver import LevenbergMarquardt, LevenbergMarquardtConfig, LinearSolverType

pytestmark = pytest.mark.gpu
SEED = 4


def rel(a, b):
    a = np.asarray(a, dtype=np.float64); b = np.asarray(b, dtype=np.float64)
    return float(np.linalg.norm(a - b) / max(np.linalg.norm(b), 1e-300))


def solver(prob, poses=None):
    s = GpuSparseCholeskySolver(0).initialize_structure(prob)
    s.set_parameters(prob.data.poses if poses is None else poses)
    return s


def graph(sigma=0.05):
    return pkg.synthetic.make_rotation_graph(200, 6, sigma, SEED)


def with_prior_gauge(d):
    return PoseGraphProblem(d, manifold="so3").add_prior(f"x{int(d.ids[0])}")


def test_lm_history_against_the_numpy_loop():
    prob = PoseGraphProblem.pose_graph(graph())
    kw = dict(max_iterations=20, cost_tolerance=1e-6, parameter_tolerance=1e-8, damping=1e-3)
    cfg = LevenbergMarquardtConfig.new().with_linear_solver_type(LinearSolverType.SparseCholesky)
    for k, v in kw.items():
        cfg = getattr(cfg, "with_" + k)(v)
    res = LevenbergMarquardt.with_config(cfg).optimize(prob)
    o = sr.So3Problem.from_problem(prob).lm_optimize(**kw)
    Hh = o["history"]
    print(res.status, res.iterations, o["status"], o["iterations"], res.history[:, 0], Hh[:, 0])
    assert res.status.value == o["status"] and res.iterations == o["iterations"]
    assert np.array_equal(res.history[:, 3], Hh[:, 3])                  # accepted
    assert np.allclose(res.history[:, 0], Hh[:, 0], rtol=1e-7) and np.allclose(res.history[:, 1], Hh[:, 1], rtol=1e-5)
    assert res.final_cost < 0.2 * res.initial_cost


def test_gauss_newton_history_against_the_numpy_loop():
    prob = with_prior_gauge(graph())
    s = solver(prob)
    res, H, _ = s.gn_optimize(GaussNewtonConfig(max_iterations=6))
    R = tr.gauss_newton(sr.So3Problem.from_problem(prob), max_iterations=6)
    print(res.status, res.iterations, R["status"], R["iterations"], H[:, 0], R["history"][:, 0])
    assert (res.status, res.iterations) == (R["status"], R["iterations"])
    np.testing.assert_allclose(H[:, 0], R["history"][:, 0], rtol=1e-7)
    assert (H[:, 3] == 1).all()
    s.close()


def test_dogleg_history_against_the_numpy_loop():
    prob = with_prior_gauge(graph())
    kw = dict(max_iterations=12, trust_region_radius=3.0)               # a radius the first steps reach: steepest-descent and dog-leg steps run
    R = tr.dog_leg(sr.So3Problem.from_problem(prob), **kw)
    assert R["margins"].min() > 1e-6                                    # no decision sits on its threshold
    s = solver(prob)
    res, H, c = s.dogleg_optimize(DogLegConfig(**kw))
    Rh = R["history"]
    print(res.status, res.iterations, R["status"], R["iterations"], "types", Rh[:, 9], "reused", Rh[:, 11])
    assert (res.status, res.iterations) == (R["status"], R["iterations"])
    assert np.array_equal(H[:, [4, 9, 11]], Rh[:, [4, 9, 11]]) and np.array_equal(H[:, 2], Rh[:, 2])
    np.testing.assert_allclose(H[:, 0], Rh[:, 0], rtol=1e-7)
    np.testing.assert_allclose(H[:, 1], Rh[:, 1], rtol=1e-7)
    s.close()


def test_noise_free_graph_is_recovered_up_to_the_gauge():
    d = graph(0.0)
    rng = np.random.default_rng(1)
    start = sr.f64(sr.so3_plus(d.truth, 0.2 * rng.standard_normal((d.n_v, 3))))
    start[0] = d.truth[0]                                               # the prior holds the first vertex at its true value: the gauge
    prob = with_prior_gauge(d)
    s = solver(prob, start)
    res, H, _ = s.gn_optimize(GaussNewtonConfig(max_iterations=15))
    got = s.get_parameters()
    got = got / np.linalg.norm(got, axis=1, keepdims=True)
    sign = np.sign((got * d.truth).sum(-1))[:, None]                    # q and -q are one rotation
    print("cost", H[:, 0], "worst |q - truth|", np.abs(got * sign - d.truth).max())
    assert s.compute_cost() < 1e-20 and np.abs(got * sign - d.truth).max() < 1e-10
    s.close()


# ---- loss, information, priors ---------------------------------------------------------------------------------------------------
CASES = [("huber", 0.4, False), ("cauchy", 1.0, False), ("andrews", 1.2, False), ("tukey", 1.5, False), (None, None, True),
         ("cauchy", 1.0, True)]


@pytest.mark.parametrize("name,scale,weighted", CASES, ids=[f"{n}-{'info' if w else 'plain'}" for n, _, w in CASES])
def test_loss_and_information(name, scale, weighted):
    d = sr.crafted("nv97")
    loss = None if name is None else create_loss_function(name, scale)
    info = sr.random_information(d.n_e) if weighted else None
    prob = PoseGraphProblem(d, loss=loss, information=info, manifold="so3").add_prior("x0").add_prior("x50", huber_delta=0.01)
    s = solver(prob)
    P = sr.So3Problem.from_problem(prob)
    r, J = P.edge_blocks()
    if name == "tukey":                                                 # an edge cut to rho' = 0 contributes nothing
        cut = np.nonzero(~r.any(axis=1))[0]
        assert len(cut) > 0 and not J[cut].any()
    if name == "andrews":
        assert (P.arms == 2).any()
    assert rel(s.get_residual(), r) < 1e-12 and rel(s.get_jacobian_blocks(), J) < 1e-12
    Hr, gr, cost = P.dense(0.5)
    H, g = s.get_hessian(0.5)
    H2, g2 = s.get_hessian(0.5)
    print(name, weighted, "H", rel(H, sr.f64(Hr)), "g", rel(g, sr.f64(gr)))
    assert np.array_equal(H, H2) and np.array_equal(g, g2)
    assert rel(H, sr.f64(Hr)) < 1e-12 and rel(g, sr.f64(gr)) < 1e-12
    assert s.compute_cost() == pytest.approx(float(cost), rel=1e-12)
    if name == "tukey":
        for e in cut:                                                   # the pair's block holds the other edges only: here none
            a, b = int(d.e_from[e]), int(d.e_to[e])
            others = ((d.e_from == a) & (d.e_to == b)) | ((d.e_from == b) & (d.e_to == a))
            if others.sum() == 1:
                ca, cb = prob.pose_col[a], prob.pose_col[b]
                assert not H[ca:ca + 3, cb:cb + 3].any()
    # the Dog-Leg products |J a|^2, (J a).(J b), |J b|^2 against the reference's dense J
    rng = np.random.default_rng(2)
    a, b = rng.standard_normal(P.n), rng.standard_normal(P.n)
    _, Jd = P.jacobian()
    want = np.array([(Jd @ a) @ (Jd @ a), (Jd @ a) @ (Jd @ b), (Jd @ b) @ (Jd @ b)])
    got = np.array(s.jv_gram(a, b))
    print("jv_gram", np.abs(got / want - 1).max())
    assert np.allclose(got, want, rtol=1e-12)
    s.close()


def test_marginal_covariances():
    d = sr.crafted("nv97")
    prob = PoseGraphProblem(d, manifold="so3").add_prior("x0")
    s = solver(prob)
    lam = 1e-3
    H, _ = s.get_hessian(lam)
    s.solve_augmented_equation(lam)
    cov = s.pose_covariance_blocks()
    assert cov.shape == (97, 3, 3)
    Hr, _, _ = sr.So3Problem.from_problem(prob).dense(lam)
    Z = np.linalg.inv(sr.f64(Hr))
    errs = [float(np.abs(cov[v] - Z[c:c + 3, c:c + 3]).max() / np.abs(Z[c:c + 3, c:c + 3]).max()) for v, c in enumerate(prob.pose_col)]
    print("worst covariance block error", max(errs), "cond", np.linalg.cond(sr.f64(Hr)))
    assert max(errs) <= 1e-7                                            # tests/test_gpu_se2_covariance.py at lambda = 1e-3
    s.close()
