"""The robust loss family on the device (apexgpu_pg_set_loss): every per-edge kernel's general-loss instantiation against
tests/np_ref_loss.py, on make_sphere(8, 12) (SE3) and make_manhattan(120) (SE2) with a fifth of the edges gross outliers
and one self-loop (tests/loss_graphs.py).

Bounds are those of the Huber cases of tests/test_gpu_pg_parity.py::test_oracle_parity_mid_size and tests/test_gpu_se2_parity.py
(r, J, H, g, cost 1e-12 relative; step 1e-10 at lambda = 1e-3 and 1e4, plus the backward residual 1e-13), of tests/test_gpu_trust_region.py for histories (cost 1e-7) and jv_gram (1e-12),
and of tests/test_gpu_covariance.py for the covariance (1e-10 at lambda = 1e4)."""
import ctypes as C

import numpy as np
import pytest

import apex_solver_amd as pkg
import loss_graphs as lg
import np_ref_loss as nl
import np_ref_trust_region as tr
from apex_solver_amd import capi
from apex_solver_amd.pose_graph import (DogLegConfig, GaussNewtonConfig, GpuSparseCholeskySolver, Loss, PoseGraphProblem,
                                        create_loss_function)
from apex_solver_amd.solver import LevenbergMarquardtConfig

pytestmark = pytest.mark.gpu
MANIFOLDS = ["se3", "se2"]
_cache = {}


def rel(a, b):
    a = np.asarray(a, dtype=np.float64); b = np.asarray(b, dtype=np.float64)
    return float(np.linalg.norm(a - b) / max(np.linalg.norm(b), 1e-300))


def case(man, jitter=False):
    """the graph, its uncorrected linearisation and the sweep's losses: computed once, never changed"""
    key = (man, jitter)
    if key not in _cache:
        d = lg.graph(man, 120, jitter=jitter)
        r, J = lg.linearize(d)
        r.setflags(write=False); J.setflags(write=False)
        _cache[key] = (d, r, J, lg.sweep_losses(r))
    return _cache[key]


def numpy_problem(prob):
    return (nl.Se2LossProblem if prob.manifold == "se2" else nl.Se3LossProblem).from_problem(prob)


def solver(prob, poses=None):
    s = GpuSparseCholeskySolver().initialize_structure(prob)
    s.set_parameters(prob.data.poses if poses is None else poses)
    return s


# ---- parity sweep --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", lg.SWEEP)
@pytest.mark.parametrize("man", MANIFOLDS)
def test_parity_sweep(man, name):
    d, r0, J0, losses = case(man, lg.needs_jitter(name))
    loss = losses[name]
    arms, rho1 = lg.check_conditions(name, loss, r0)
    prob = PoseGraphProblem.pose_graph(d, loss=loss)
    P = numpy_problem(prob)
    s = solver(prob)
    assert s.get_loss() == loss
    rt, Jt = P.edge_blocks()
    gr, gJ = s.get_residual(), s.get_jacobian_blocks()
    print(man, name, "arms", (arms == 1).sum(), (arms == 2).sum(), "rho'=0:", (rho1 == 0).sum(), "r", rel(gr, rt), "J", rel(gJ, Jt))
    assert rel(gr, rt) < 1e-12 and rel(gJ, Jt) < 1e-12
    zero = rho1 == 0.0
    assert not gr[zero].any() and not gJ[zero].any()
    Ho, go = P.normal_equations()
    c = P.cost()
    gc = s.compute_cost()
    print("  cost", abs(gc - c) / c)
    assert abs(gc - c) <= 1e-12 * c
    for lam in (1e-3, 1e4):
        H, g = s.get_hessian(lam)
        A = Ho + lam * np.eye(P.n)
        step = s.solve_augmented_equation(lam)
        so = tr.solve_damped(Ho, go, lam)
        cond = np.linalg.cond(A)
        print(f"  lambda {lam:g}: H {rel(H, A):.2e} g {rel(g, go):.2e} step {rel(step, so):.2e} cond {cond:.2e}")
        assert rel(H, A) < 1e-12 and rel(g, go) < 1e-12
        assert rel(s.get_gradient(), go) < 1e-12
        assert rel(step, so) < 1e-10, (rel(step, so), cond)   # at both lambdas, as test_oracle_parity_mid_size has it
        assert np.linalg.norm(A @ step + go) <= 1e-13 * (np.linalg.norm(A, 2) * np.linalg.norm(step) + np.linalg.norm(go))
    s.close()


# ---- legacy equivalence ----------------------------------------------------------------------------------------------------
def _lm_history(s, iters=6):
    _, H, _ = s.lm_optimize(LevenbergMarquardtConfig(max_iterations=iters))
    return H


@pytest.mark.parametrize("man", MANIFOLDS)
def test_huber_through_set_loss_is_huber_delta(man):
    d, r0, _, _ = case(man)
    delta = float(lg.scale_between(r0, 0.6))
    ss = lg.squared_norms(r0)
    assert (ss > delta * delta).any() and (ss < delta * delta).any()
    a = solver(PoseGraphProblem.pose_graph(d, delta))
    b = solver(PoseGraphProblem.pose_graph(d, loss=Loss(capi.LOSS_HUBER, delta)))
    assert a.get_loss() == Loss(capi.LOSS_HUBER, delta) and b.get_loss() == Loss(capi.LOSS_HUBER, delta)
    assert np.array_equal(a.get_residual(), b.get_residual()) and np.array_equal(a.get_jacobian_blocks(), b.get_jacobian_blocks())
    Ha, ga = a.get_hessian(1e-3); Hb, gb = b.get_hessian(1e-3)
    ha, hb = _lm_history(a), _lm_history(b)
    if man == "se2":   # row-owned assembly, no atomics: the same bits
        assert np.array_equal(Ha, Hb) and np.array_equal(ga, gb) and a.compute_cost() == b.compute_cost()
        assert np.array_equal(ha, hb)
    else:              # SE3 assembles with fp64 atomics
        assert rel(Hb, Ha) < 1e-12 and rel(gb, ga) < 1e-12
        assert ha.shape == hb.shape and np.array_equal(ha[:, 3], hb[:, 3])
        np.testing.assert_allclose(hb[:, 0], ha[:, 0], rtol=1e-7)
    a.close(); b.close()


@pytest.mark.parametrize("man", MANIFOLDS)
def test_l2_and_none_through_set_loss_are_no_loss(man):
    d, _, _, _ = case(man)
    a = solver(PoseGraphProblem.pose_graph(d))
    ra, Ja, ca = a.get_residual(), a.get_jacobian_blocks(), a.compute_cost()
    Ha, ga = a.get_hessian(1e-3)
    for kind in (capi.LOSS_L2, capi.LOSS_NONE):
        b = solver(PoseGraphProblem.pose_graph(d, 0.01))   # (a Huber delta that set_loss must replace)
        b.set_loss(Loss(kind))
        assert b.get_loss().kind == kind
        assert np.array_equal(b.get_residual(), ra) and np.array_equal(b.get_jacobian_blocks(), Ja)
        Hb, gb = b.get_hessian(1e-3)
        assert rel(Hb, Ha) < 1e-12 and rel(gb, ga) < 1e-12 and abs(b.compute_cost() - ca) <= 1e-12 * ca
        if man == "se2":
            assert np.array_equal(Hb, Ha) and np.array_equal(gb, ga)
        b.close()
    a.close()


def test_se2_cauchy_history_is_bit_reproducible():
    d, _, _, losses = case("se2")
    runs = []
    for _ in range(2):
        s = solver(PoseGraphProblem.pose_graph(d, loss=losses["cauchy"]))
        runs.append((_lm_history(s), s.get_parameters()))
        s.close()
    assert np.array_equal(runs[0][0], runs[1][0]) and np.array_equal(runs[0][1], runs[1][1])


# ---- loops ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["cauchy", "andrews"])
@pytest.mark.parametrize("man", MANIFOLDS)
def test_loops_against_the_numpy_loops(man, name):
    d, _, _, losses = case(man, lg.needs_jitter(name))
    # (a prior on the first vertex: without it H is singular along the gauge and Gauss-Newton's undamped Cholesky is decided by rounding)
    prob = PoseGraphProblem.pose_graph(d, loss=losses[name]).add_prior(f"x{int(d.ids[0])}")
    # jv_gram against a^T H b of the dense J~^T J~
    P = numpy_problem(prob)
    _, J = P.jacobian()
    s = solver(prob)
    rng = np.random.default_rng(7)
    a, b = rng.normal(size=P.n), rng.normal(size=P.n)
    u, w = J @ a, J @ b
    got = s.jv_gram(a, b)
    print(man, name, "jv_gram", got, (u @ u, u @ w, w @ w))
    assert got[0] == pytest.approx(u @ u, rel=1e-12) and got[2] == pytest.approx(w @ w, rel=1e-12)
    assert abs(got[1] - u @ w) <= 1e-12 * np.linalg.norm(u) * np.linalg.norm(w)
    assert s.jv_gram(a, b) == got
    # LM
    ref = nl.lm(numpy_problem(prob), 8)
    res, H, _ = s.lm_optimize(LevenbergMarquardtConfig(max_iterations=8))
    print("LM", res.iterations, ref["iterations"], H[:, 0], ref["history"][:, 0])
    assert res.iterations == ref["iterations"] and np.array_equal(H[:, 3], ref["history"][:, 3])
    np.testing.assert_allclose(H[:, 0], ref["history"][:, 0], rtol=1e-7)
    # Gauss-Newton
    s.set_parameters(d.poses)
    ref = tr.gauss_newton(numpy_problem(prob), max_iterations=8)
    res, H, _ = s.gn_optimize(GaussNewtonConfig(max_iterations=8))
    print("GN", res.status, ref["status"], res.iterations, ref["iterations"], H[:, 0], ref["history"][:, 0])
    assert res.status == ref["status"] and res.iterations == ref["iterations"]
    np.testing.assert_allclose(H[:, 0], ref["history"][:, 0], rtol=1e-7)
    # Dog-Leg, step reuse on
    s.set_parameters(d.poses)
    ref = tr.dog_leg(numpy_problem(prob), max_iterations=8, enable_step_reuse=True)
    res, H, _ = s.dogleg_optimize(DogLegConfig(max_iterations=8, enable_step_reuse=True))
    print("DL", res.status, ref["status"], res.iterations, ref["iterations"], H[:, 0], ref["history"][:, 0], "reused", H[:, 11],
          "margins", ref["margins"].min())
    assert ref["margins"].min() > 1e-6       # no decision of the reference loop sits on its threshold
    assert ref["history"][:, 11].any()       # the reused path runs under the general loss
    assert (res.status, res.iterations) == (ref["status"], ref["iterations"])
    assert np.array_equal(H[:, [4, 9, 11]], ref["history"][:, [4, 9, 11]])   # accepted, step type, reused
    assert np.array_equal(H[:, 2], ref["history"][:, 2])                     # mu
    np.testing.assert_allclose(H[:, 0], ref["history"][:, 0], rtol=1e-7)
    np.testing.assert_allclose(H[:, 1], ref["history"][:, 1], rtol=1e-7)
    s.close()


# ---- edges of the API ------------------------------------------------------------------------------------------------------
def test_set_loss_before_set_structure_is_invalid_state():
    h = capi.PgHandle(4, 3, 0, capi.MANIFOLD_SE3)
    assert h.L.apexgpu_pg_set_loss(h.h, capi.LOSS_CAUCHY, 1.0, 0.0) == -6
    k = C.c_int(-1); p = (C.c_double * 2)()
    assert h.L.apexgpu_pg_get_loss(h.h, C.byref(k), C.byref(p)) == 0 and k.value == capi.LOSS_NONE
    h.close()


@pytest.mark.parametrize("man", MANIFOLDS)
def test_set_loss_refusals_and_the_dogleg_cache(man):
    d, _, _, losses = case(man)
    s = solver(PoseGraphProblem.pose_graph(d, loss=losses["cauchy"]))
    for bad in (Loss(capi.LOSS_TUKEY, 0.0), Loss(capi.LOSS_LP_NORM, -1.0), Loss(capi.LOSS_BARRON, 1.0, 0.0), Loss(15, 1.0), Loss(-1, 1.0)):
        with pytest.raises(capi.LinAlgError) as e:
            s.set_loss(bad)
        assert e.value.kind == "InvalidInput"
    assert s.get_loss() == losses["cauchy"]   # a refused call changes nothing
    s.dogleg_step(1e-4, 1.0)
    s.eval_step(); s.discard_step()
    assert s.dogleg_step(1e-4, 0.5, reuse=True)["reused"]
    s.eval_step(); s.discard_step()
    s.set_loss(losses["welsch"])
    with pytest.raises(capi.LinAlgError) as e:
        s.dogleg_step(1e-4, 0.25, reuse=True)
    assert e.value.kind == "InvalidState"
    with pytest.raises(capi.LinAlgError) as e:
        s.eval_step()
    assert e.value.kind == "InvalidState"
    s.close()


@pytest.mark.parametrize("man", MANIFOLDS)
def test_covariance_after_a_cauchy_solve(man):
    d, _, _, losses = case(man)
    prob = PoseGraphProblem.pose_graph(d, loss=losses["cauchy"])
    s = solver(prob)
    lam = 1e4
    s.solve_augmented_equation(lam)
    cov = s.pose_covariance_blocks()
    H, _ = s.get_hessian(lam)
    Hinv = np.linalg.inv(H)
    D = prob.dof
    errs = [rel(cov[v], Hinv[c:c + D, c:c + D]) for v, c in enumerate(prob.pose_col)]
    print(man, "covariance", max(errs))
    assert max(errs) <= 1e-10
    s.close()


@pytest.mark.parametrize("man", MANIFOLDS)
def test_tukey_below_every_residual_leaves_a_singular_system(man):
    d, r0, _, _ = case(man, jitter=True)   # (no residual of rounding size: every edge is beyond the scale)
    scale = 0.5 * float(np.sqrt(lg.squared_norms(r0).min()))
    assert scale > 0.0
    s = solver(PoseGraphProblem.pose_graph(d, loss=create_loss_function("tukey", scale)))
    H, g = s.get_hessian(0.0)
    assert not H.any() and not g.any()
    assert s.compute_cost() == 0.0
    res, _, _ = s.gn_optimize(GaussNewtonConfig(max_iterations=3))
    ref = tr.gauss_newton(numpy_problem(PoseGraphProblem.pose_graph(d, loss=create_loss_function("tukey", scale))), max_iterations=3)
    assert ref["status"] == 100 and res.status == 100   # LinearSolveFailed: the solve's SingularMatrix
    with pytest.raises(capi.LinAlgError) as e:
        s.solve_augmented_equation(0.0)
    assert e.value.kind == "SingularMatrix"
    s.close()


# ---- the grid-stride pass of the cost and Gram kernels in the general instantiation ------------------------------------------
def _random_path_graph(manifold, n_v, seed):
    """the construction of test_gpu_pg_parity.py::test_cost_grid_stride_pass_equals_the_sum_of_single_pass_parts"""
    rng = np.random.default_rng(seed)

    def poses(n):
        if manifold == "se2":
            return np.column_stack([10.0 * rng.standard_normal((n, 2)), rng.uniform(-np.pi, np.pi, n)])
        q = rng.standard_normal((n, 4))
        return np.column_stack([10.0 * rng.standard_normal((n, 3)), q / np.linalg.norm(q, axis=1, keepdims=True)])

    e = np.arange(n_v - 1, dtype=np.uint32)
    return pkg.synthetic.PoseGraphData(ids=np.arange(n_v, dtype=np.int64), poses=poses(n_v), e_from=e, e_to=e + 1, meas=poses(n_v - 1))


def _path_slice(d, v0, v1):
    e = np.arange(v1 - v0, dtype=np.uint32)
    return pkg.synthetic.PoseGraphData(ids=d.ids[v0:v1 + 1], poses=d.poses[v0:v1 + 1], e_from=e, e_to=e + 1, meas=d.meas[v0:v1])


def _cost_and_gram(d, loss, a, b, v0):
    """cost and jv_gram of a (sub-)path; a, b are given per vertex of the whole path ([n_v][dof]) and v0 is the slice's first"""
    prob = PoseGraphProblem(d, loss=loss)
    s = solver(prob)
    D = prob.dof
    x = np.zeros(D * d.n_v); y = np.zeros(D * d.n_v)
    idx = prob.pose_col[:, None] + np.arange(D)[None]
    x[idx] = a[v0:v0 + d.n_v]; y[idx] = b[v0:v0 + d.n_v]
    out = (s.compute_cost(), np.array(s.jv_gram(x, y)))
    s.close()
    return out


@pytest.mark.parametrize("man", MANIFOLDS)
def test_grid_stride_pass_of_cost_and_gram_with_a_loss(man):
    """256 blocks of 256 threads: only a graph above 65,536 edges sends a thread round the loop of k_pg_cost_partial and
    k_pg_jv_gram a second time.  The whole path against the device's own single-pass results on its two halves, which the
    numpy references pin at small sizes: equal to rel 1e-13 (cost) and 1e-12 (Gram), as the legacy test has it."""
    n_v, mid = 66000, 33000
    d = _random_path_graph(man, n_v, seed=12)
    assert d.n_e > 256 * 256
    loss = create_loss_function("cauchy")
    D = 3 if man == "se2" else 6
    rng = np.random.default_rng(2)
    a, b = rng.standard_normal((n_v, D)), rng.standard_normal((n_v, D))
    c0, g0 = _cost_and_gram(_path_slice(d, 0, mid), loss, a, b, 0)
    c1, g1 = _cost_and_gram(_path_slice(d, mid, n_v - 1), loss, a, b, mid)
    cw, gw = _cost_and_gram(d, loss, a, b, 0)
    print(man, cw, c0 + c1, gw, g0 + g1)
    assert c0 > 0.0 and c1 > 0.0 and abs(cw - (c0 + c1)) <= 1e-13 * (c0 + c1)
    assert abs(gw[0] - (g0 + g1)[0]) <= 1e-12 * gw[0] and abs(gw[2] - (g0 + g1)[2]) <= 1e-12 * gw[2]
    assert abs(gw[1] - (g0 + g1)[1]) <= 1e-12 * np.sqrt(gw[0] * gw[2])
