"""Edge information matrices on the device (apexgpu_pg_set_information): the LossWeighted instantiation of every
per-edge kernel against tests/np_ref_info.py, on info_graphs.graph("se3") -- make_sphere(8, 12), four 144-row tiles -- and
info_graphs.graph("se2", 120) -- make_manhattan(120) --, both with outliers, one self-loop, edges of either direction and a
dense random Omega per edge (tests/info_graphs.py).

Bounds are those of tests/test_gpu_pg_loss.py (r, J, H, g, cost 1e-12 relative; step 1e-10 at lambda = 1e-3 and 1e4 plus the
backward residual 1e-13; jv_gram 1e-12; histories: cost 1e-7, decisions equal) and of tests/test_gpu_covariance.py (1e-10 at
lambda = 1e4).  tests/test_info_device_math_host.py checks on the CPU that the fixture is conditioned well enough for the
step bound."""
import ctypes as C
from types import SimpleNamespace

import numpy as np
import pytest

import info_graphs as ig
import loss_graphs as lg
import np_ref_info as ni
import np_ref_loss as nl
import np_ref_trust_region as tr
from apex_solver_amd import capi
from apex_solver_amd.pose_graph import (DogLegConfig, GaussNewtonConfig, G2oLoader, GpuSparseCholeskySolver, PoseGraphProblem,
                                        create_loss_function, write_g2o)
from apex_solver_amd.solver import LevenbergMarquardtConfig

pytestmark = pytest.mark.gpu
MANIFOLDS = ["se3", "se2"]
SWEEP = ("none", "huber", "cauchy", "tukey", "andrews", "lp3")
_cache, _refs = {}, {}


def rel(a, b):
    a = np.asarray(a, dtype=np.float64); b = np.asarray(b, dtype=np.float64)
    return float(np.linalg.norm(a - b) / max(np.linalg.norm(b), 1e-300))


def case(man, jitter=False):
    """the graph, its information matrices, its whitened uncorrected linearisation and the sweep's losses: once, read-only"""
    key = (man, jitter)
    if key not in _cache:
        d = ig.graph(man, 120, jitter=jitter)
        W = ig.information(d)
        r, J = lg.linearize(d)
        rw, Jw = ni.whiten(r, J, W)
        rw.setflags(write=False); Jw.setflags(write=False)
        losses = {"none": None, "huber": create_loss_function("huber", float(lg.scale_between(rw, 0.6))),
                  "cauchy": create_loss_function("cauchy"), "tukey": create_loss_function("tukey", lg.scale_between(rw, 0.8)),
                  "andrews": create_loss_function("andrews"), "lp3": create_loss_function("lp", 3.0)}
        _cache[key] = SimpleNamespace(d=d, W=W, rw=rw, Jw=Jw, losses=losses)
    return _cache[key]


def reference(man, name):
    """the numpy problem of (graph, Omega, loss) with its corrected blocks, H, g and cost: computed once, shared"""
    key = (man, name)
    if key not in _refs:
        c = case(man, lg.needs_jitter(name))
        prob = PoseGraphProblem.pose_graph(c.d, loss=c.losses[name], information=c.W)
        P = ni.numpy_problem(prob)
        rt, Jt = P.edge_blocks()
        H, g = P.normal_equations()
        for a in (rt, Jt, H, g):
            a.setflags(write=False)
        _refs[key] = SimpleNamespace(prob=prob, P=P, rt=rt, Jt=Jt, H=H, g=g, cost=P.cost(), arms=P.arms.copy(), s=P.s.copy())
    return _refs[key]


def solver(prob, poses=None):
    s = GpuSparseCholeskySolver().initialize_structure(prob)
    s.set_parameters(prob.data.poses if poses is None else poses)
    return s


def check_conditions(name, loss, R):
    if loss is None:
        return np.ones(len(R.s))
    assert nl.threshold_margin(loss, R.s) > 1e-9
    rho1 = np.array([float(nl.evaluate(loss, s)[1]) for s in R.s])
    if name in ("andrews", "lp3"):
        assert (R.arms == 1).sum() >= 10 and (R.arms == 2).sum() >= 10, (name, (R.arms == 1).sum(), (R.arms == 2).sum())
    if name == "tukey":
        assert (rho1 == 0.0).sum() >= 1 and (rho1 > 0.0).sum() >= 1
    if name == "huber":
        assert (R.s > loss.p0 ** 2).any() and (R.s < loss.p0 ** 2).any()
    return rho1


# ---- 1. parity sweep ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", SWEEP)
@pytest.mark.parametrize("man", MANIFOLDS)
def test_parity_sweep(man, name):
    R = reference(man, name)
    loss = case(man, lg.needs_jitter(name)).losses[name]
    rho1 = check_conditions(name, loss, R)
    s = solver(R.prob)
    assert np.array_equal(s.get_information(), R.prob.information)
    gr, gJ = s.get_residual(), s.get_jacobian_blocks()
    print(man, name, "arms", (R.arms == 1).sum(), (R.arms == 2).sum(), "rho'=0:", (rho1 == 0).sum(), "r", rel(gr, R.rt), "J", rel(gJ, R.Jt))
    assert rel(gr, R.rt) < 1e-12 and rel(gJ, R.Jt) < 1e-12
    zero = rho1 == 0.0
    assert not gr[zero].any() and not gJ[zero].any()
    gc = s.compute_cost()
    print("  cost", abs(gc - R.cost) / R.cost)
    assert abs(gc - R.cost) <= 1e-12 * R.cost
    n = R.P.n
    for lam in (1e-3, 1e4):
        H, g = s.get_hessian(lam)
        A = R.H + lam * np.eye(n)
        step = s.solve_augmented_equation(lam)
        so = tr.solve_damped(R.H, R.g, lam)
        print(f"  lambda {lam:g}: H {rel(H, A):.2e} g {rel(g, R.g):.2e} step {rel(step, so):.2e}")
        assert rel(H, A) < 1e-12 and rel(g, R.g) < 1e-12
        assert rel(s.get_gradient(), R.g) < 1e-12
        assert rel(step, so) < 1e-10
        assert np.linalg.norm(A @ step + R.g) <= 1e-13 * (np.linalg.norm(A, 2) * np.linalg.norm(step) + np.linalg.norm(R.g))
    s.close()


# ---- 2. jv_gram --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["cauchy", "lp3"])
@pytest.mark.parametrize("man", MANIFOLDS)
def test_jv_gram(man, name):
    R = reference(man, name)
    _, J = R.P.jacobian()
    s = solver(R.prob)
    rng = np.random.default_rng(7)
    a, b = rng.normal(size=R.P.n), rng.normal(size=R.P.n)
    u, w = J @ a, J @ b
    got = s.jv_gram(a, b)
    print(man, name, got, (u @ u, u @ w, w @ w))
    assert got[0] == pytest.approx(u @ u, rel=1e-12) and got[2] == pytest.approx(w @ w, rel=1e-12)
    assert abs(got[1] - u @ w) <= 1e-12 * np.linalg.norm(u) * np.linalg.norm(w)
    assert s.jv_gram(a, b) == got
    s.close()


# ---- 3. scaling laws, no loss ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("man", MANIFOLDS)
def test_scaling_laws(man):
    c = case(man)
    D = c.W.shape[1]
    eye = np.broadcast_to(np.eye(D), c.W.shape).copy()
    plain = solver(PoseGraphProblem.pose_graph(c.d))
    H0, g0 = plain.get_hessian(0.0)
    c0 = plain.compute_cost()
    for k in (1.0, 4.0):   # Omega = I: another instantiation, the same numbers; Omega = 4 I: four times them
        s = solver(PoseGraphProblem.pose_graph(c.d, information=k * eye))
        H, g = s.get_hessian(0.0)
        print(man, k, rel(H, k * H0), rel(g, k * g0), abs(s.compute_cost() - k * c0) / (k * c0))
        assert rel(H, k * H0) < 1e-12 and rel(g, k * g0) < 1e-12 and abs(s.compute_cost() - k * c0) <= 1e-12 * k * c0
        s.close()
    plain.close()
    # (k Omega: H -> k H, so (k H + k lambda I)^-1 = (H + lambda I)^-1 / k: the damping scales along)
    lam, k = 1e4, 4.0
    a = solver(PoseGraphProblem.pose_graph(c.d, information=c.W))
    b = solver(PoseGraphProblem.pose_graph(c.d, information=k * c.W))
    a.solve_augmented_equation(lam); b.solve_augmented_equation(k * lam)
    ca, cb = a.pose_covariance_blocks(), b.pose_covariance_blocks()
    errs = [rel(cb[v], ca[v] / k) for v in range(c.d.n_v)]
    print(man, "covariance", max(errs))
    assert max(errs) <= 1e-10
    a.close(); b.close()


# ---- 4. clearing restores the old path ---------------------------------------------------------------------------------------
def _lm_history(s, iters=6):
    _, H, _ = s.lm_optimize(LevenbergMarquardtConfig(max_iterations=iters))
    return H


@pytest.mark.parametrize("man", MANIFOLDS)
def test_clearing_restores_the_unweighted_path(man):
    c = case(man)
    plain = solver(PoseGraphProblem.pose_graph(c.d))
    s = solver(PoseGraphProblem.pose_graph(c.d, information=c.W))
    s.solve_augmented_equation(1e-3)
    s.set_information(None)
    assert s.get_information() is None
    assert np.array_equal(s.get_residual(), plain.get_residual()) and np.array_equal(s.get_jacobian_blocks(), plain.get_jacobian_blocks())
    assert s.compute_cost() == plain.compute_cost()
    Hs, gs = s.get_hessian(1e-3); Hp, gp = plain.get_hessian(1e-3)
    if man == "se2":
        assert np.array_equal(Hs, Hp) and np.array_equal(gs, gp)
        assert np.array_equal(_lm_history(s), _lm_history(plain))
    else:   # fp64 atomics
        assert rel(Hs, Hp) < 1e-12 and rel(gs, gp) < 1e-12
    s.close(); plain.close()


# ---- 5. SE2 reproducibility --------------------------------------------------------------------------------------------------
def test_se2_weighted_cauchy_history_is_bit_reproducible():
    c = case("se2")
    runs = []
    for _ in range(2):
        s = solver(PoseGraphProblem.pose_graph(c.d, loss=c.losses["cauchy"], information=c.W))
        Ha, ga = s.get_hessian(1e-3); Hb, gb = s.get_hessian(1e-3)
        assert np.array_equal(Ha, Hb) and np.array_equal(ga, gb)
        runs.append((_lm_history(s), s.get_parameters()))
        s.close()
    assert np.array_equal(runs[0][0], runs[1][0]) and np.array_equal(runs[0][1], runs[1][1])


# ---- 6. optimisers -----------------------------------------------------------------------------------------------------------
def _huber_problem(man):
    c = case(man)
    # (huber_delta, not set_loss: the weighted kernels then take the delta as a Huber PgLoss.  A prior on the first vertex:
    # without it H is singular along the gauge and Gauss-Newton's undamped Cholesky is decided by rounding.)
    prob = PoseGraphProblem.pose_graph(c.d, float(c.losses["huber"].p0), information=c.W).add_prior(f"x{int(c.d.ids[0])}")
    P = ni.numpy_problem(prob)
    P.long_double = False
    return c, prob, P


@pytest.mark.parametrize("man", MANIFOLDS)
def test_lm_against_the_numpy_loop(man):
    c, prob, P = _huber_problem(man)
    s = solver(prob)
    ref = nl.lm(P, 6)
    res, H, _ = s.lm_optimize(LevenbergMarquardtConfig(max_iterations=6))
    print("LM", res.iterations, ref["iterations"], H[:, 0], ref["history"][:, 0])
    assert res.iterations == ref["iterations"] and np.array_equal(H[:, 3], ref["history"][:, 3])
    np.testing.assert_allclose(H[:, 0], ref["history"][:, 0], rtol=1e-7)
    s.close()


@pytest.mark.parametrize("man", MANIFOLDS)
def test_gauss_newton_against_the_numpy_loop(man):
    c, prob, P = _huber_problem(man)
    s = solver(prob)
    ref = tr.gauss_newton(P, max_iterations=6)
    res, H, _ = s.gn_optimize(GaussNewtonConfig(max_iterations=6))
    print("GN", res.status, ref["status"], res.iterations, ref["iterations"], H[:, 0], ref["history"][:, 0])
    assert res.status == ref["status"] and res.iterations == ref["iterations"]
    np.testing.assert_allclose(H[:, 0], ref["history"][:, 0], rtol=1e-7)
    s.close()


@pytest.mark.parametrize("man", MANIFOLDS)
def test_dog_leg_against_the_numpy_loop(man):
    c, prob, P = _huber_problem(man)
    s = solver(prob)
    ref = tr.dog_leg(P, max_iterations=6, enable_step_reuse=True)
    res, H, _ = s.dogleg_optimize(DogLegConfig(max_iterations=6, enable_step_reuse=True))
    print("DL", res.status, ref["status"], res.iterations, ref["iterations"], H[:, 0], ref["history"][:, 0], "margins", ref["margins"].min())
    assert ref["margins"].min() > 1e-6       # no decision of the reference loop sits on its threshold
    assert (res.status, res.iterations) == (ref["status"], ref["iterations"])
    assert np.array_equal(H[:, [4, 9, 11]], ref["history"][:, [4, 9, 11]])   # accepted, step type, reused
    np.testing.assert_allclose(H[:, 0], ref["history"][:, 0], rtol=1e-7)
    np.testing.assert_allclose(H[:, 1], ref["history"][:, 1], rtol=1e-7)
    s.close()


# ---- 7. step protocol --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("man", MANIFOLDS)
def test_set_information_invalidates_a_pending_step_and_the_dogleg_cache(man):
    c = case(man)
    s = solver(PoseGraphProblem.pose_graph(c.d, loss=c.losses["cauchy"]))
    s.solve_augmented_equation(1e-3)
    s.set_information(c.W)
    with pytest.raises(capi.LinAlgError) as e:
        s.eval_step()
    assert e.value.kind == "InvalidState"
    s.dogleg_step(1e-4, 1.0)
    s.eval_step(); s.discard_step()
    assert s.dogleg_step(1e-4, 0.5, reuse=True)["reused"]
    s.eval_step(); s.discard_step()
    s.set_information(None)
    with pytest.raises(capi.LinAlgError) as e:
        s.dogleg_step(1e-4, 0.25, reuse=True)
    assert e.value.kind == "InvalidState"
    s.close()


# ---- 8. refusals -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("man", MANIFOLDS)
def test_refusals_name_the_edge_and_change_nothing(man):
    c = case(man)
    s = solver(PoseGraphProblem.pose_graph(c.d))
    D = c.W.shape[1]
    asym = c.W.copy(); asym[5, 0, 1] += 1e-6
    indef = c.W.copy(); indef[7] = np.eye(D); indef[7, D - 1, D - 1] = -1.0
    nan = c.W.copy(); nan[9, 1, 1] = np.nan
    for held in (None, c.W):
        if held is not None:
            s.set_information(held)
        for bad, edge in ((asym, 5), (indef, 7), (nan, 9)):
            with pytest.raises(capi.LinAlgError) as e:
                s.set_information(bad)
            assert e.value.kind == "InvalidInput" and f"edge {edge}" in str(e.value), str(e.value)
            got = s.get_information()
            assert (got is None) if held is None else np.array_equal(got, held)
    s.close()


def test_set_information_before_set_structure_is_invalid_state():
    h = capi.PgHandle(4, 3, 0, capi.MANIFOLD_SE3)
    W = np.broadcast_to(np.eye(6), (3, 6, 6)).copy()
    assert h.L.apexgpu_pg_set_information(h.h, capi.ptr(W)) == -6
    present = C.c_int(-1)
    assert h.L.apexgpu_pg_get_information(h.h, C.byref(present), None) == 0 and present.value == 0
    h.close()


# ---- 9. G2O end to end -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("man", MANIFOLDS)
def test_g2o_end_to_end(man, tmp_path):
    R = reference(man, "none")
    c = case(man)
    path = tmp_path / "w.g2o"
    write_g2o(path, c.d, information=c.W)
    g = G2oLoader.load(path)
    s = GpuSparseCholeskySolver().initialize_structure(PoseGraphProblem.pose_graph(g.to_problem_data(use_information=True)))
    s.set_parameters(c.d.poses)
    assert np.array_equal(s.get_information(), c.W)
    H, gg = s.get_hessian(0.0)
    print(man, rel(H, R.H), rel(gg, R.g))
    assert rel(H, R.H) < 1e-12 and rel(gg, R.g) < 1e-12
    s.close()
