"""Gauss-Newton and Dog-Leg on the device, through the Python surface of the C ABI, against tests/np_ref_trust_region.py (needs a
real MI355X: `pytest -m gpu`).

Bounds: the Gram sums 1e-12 relative (the tree's bound for J^T J and J^T r; the cross term normwise, against |J a| |J b|, as those
are); the Dog-Leg step 1e-10 relative where cond(H + mu I) <= 1e5 (asserted on the numpy matrix), alpha and the predicted
reduction 1e-9; histories: cost 1e-7 (the LM-history bound), radius 1e-7, mu / type / accepted / reused exactly."""
import ctypes as C

import numpy as np
import pytest

import apex_solver_amd as pkg
import fixed_masks as fm
import np_ref_trust_region as tr
import tr_cases as tc
from apex_solver_amd import capi
from apex_solver_amd.loss import Loss
from apex_solver_amd.pose_graph import DogLegConfig, GaussNewtonConfig, GpuSparseCholeskySolver, PoseGraphProblem
from apex_solver_amd.solver import LevenbergMarquardtConfig
from apex_solver_amd.synthetic import PoseGraphData
from test_trust_region_np_ref import singular_case

pytestmark = pytest.mark.gpu
MANIFOLDS = ["se2", "se3"]


def rel(a, b):
    a = np.asarray(a, dtype=np.float64); b = np.asarray(b, dtype=np.float64)
    return float(np.linalg.norm(a - b) / max(np.linalg.norm(b), 1e-300))


def solver(prob, poses):
    s = GpuSparseCholeskySolver(0).initialize_structure(prob)
    s.set_parameters(poses)
    return s


def kind_of(call, *a, **k):
    with pytest.raises(capi.LinAlgError) as e:
        call(*a, **k)
    return e.value.kind


# ---- jv_gram -------------------------------------------------------------------------------------------------------------------
def random_graph(man, n_v, n_e, seed, self_loop=False):
    rng = np.random.default_rng(seed)

    def poses(n):
        if man == "se2":
            return np.column_stack([rng.uniform(-3, 3, (n, 2)), rng.uniform(-3, 3, n)])
        q = rng.normal(size=(n, 4))
        return np.column_stack([rng.uniform(-3, 3, (n, 3)), q / np.linalg.norm(q, axis=1, keepdims=True)])

    ef = rng.integers(0, n_v, n_e); et = (ef + 1 + rng.integers(0, n_v - 1, n_e)) % n_v   # (no accidental self-loops)
    if self_loop:
        et[-1] = ef[-1]
    return PoseGraphData(ids=3 * np.arange(n_v, dtype=np.int64) + 1, poses=poses(n_v), e_from=ef.astype(np.uint32),
                         e_to=et.astype(np.uint32), meas=poses(n_e), name="random")


def gram_case(man, name):
    if name == "one-edge":
        return PoseGraphProblem(random_graph(man, 2, 1, 1))
    if name == "self-loop":
        return PoseGraphProblem(random_graph(man, 3, 3, 2, self_loop=True))
    d = random_graph(man, 40, 300, 3)   # 300 edges: two workgroups of 256 lanes, the second ragged
    if name == "no-loss":
        return PoseGraphProblem(d)
    # Huber with edges on both sides of delta: the median residual norm; priors: two on one vertex, one of them Huber-scaled
    r = tc.numpy_problem(PoseGraphProblem(d), d.poses).jacobian()[0].reshape(300, -1)
    prob = PoseGraphProblem(d, float(np.median(np.linalg.norm(r, axis=1))))
    far = d.poses[7] + 2.0
    prob.add_prior(f"x{int(d.ids[7])}").add_prior(f"x{int(d.ids[7])}", data=far, huber_delta=0.5).add_prior(f"x{int(d.ids[31])}", data=d.poses[30])
    return prob


@pytest.mark.parametrize("name", ["no-loss", "huber-priors", "one-edge", "self-loop"])
@pytest.mark.parametrize("man", MANIFOLDS)
def test_jv_gram_against_dense_numpy(man, name):
    prob = gram_case(man, name)
    d = prob.data
    P = tc.numpy_problem(prob, d.poses)
    r, J = P.jacobian()
    if name == "huber-priors":
        n2 = np.einsum("ei,ei->e", *[tc.numpy_problem(PoseGraphProblem(d), d.poses).jacobian()[0].reshape(300, -1)] * 2)
        assert (n2 > prob.huber_delta ** 2).any() and (n2 < prob.huber_delta ** 2).any()
        assert P.prior_blocks()[1].min() < 1.0   # the far prior is Huber-scaled
    s = solver(prob, d.poses)
    rng = np.random.default_rng(5)
    a, b = rng.normal(size=P.n), rng.normal(size=P.n)
    for x, y in ((a, b), (a, a)):
        u, w = J @ x, J @ y
        got = s.jv_gram(x, y)
        want = (u @ u, u @ w, w @ w)
        print(man, name, got, want)
        assert got[0] == pytest.approx(want[0], rel=1e-12) and got[2] == pytest.approx(want[2], rel=1e-12)
        assert abs(got[1] - want[1]) <= 1e-12 * np.linalg.norm(u) * np.linalg.norm(w)
        assert s.jv_gram(x, y) == got   # no atomics, one order of summation: the same bits
    s.close()


# ---- dogleg_step ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("scaling", [False, True], ids=["plain", "jacobi-scaling"])
@pytest.mark.parametrize("man", MANIFOLDS)
def test_dogleg_step_of_every_type_against_numpy(man, scaling):
    n_v = tc.graph(man).n_v
    dof = 3 if man == "se2" else 6
    prob, p0 = tc.problem(man, fix=fm.pg_asymmetric(n_v, 4)[:, :dof])
    mu = 1e-2 if scaling else 1.0   # (in the scaled variables mu = 1 damps h below the Cauchy point; both keep cond <= 1e5)
    P, H, g, D, h, alpha, p_c = tc.first_linearisation(prob, p0, scaling, mu)
    cond = np.linalg.cond(H + mu * np.eye(P.n))
    hn, pn = np.linalg.norm(h), np.linalg.norm(p_c)
    assert cond <= 1e5 and pn < hn, (cond, pn, hn)
    mask = tc.mask_vector(prob)
    assert mask.any()
    s = solver(prob, p0)
    if scaling:
        s.apply_column_scaling(D)
    for radius, typ in ((2.0 * hn, tr.GAUSS_NEWTON), (0.5 * pn, tr.STEEPEST_DESCENT), (0.5 * (pn + hn), tr.DOG_LEG)):
        step_s, t, beta = tr.dog_leg_step(-g, p_c, h, radius)
        assert t == typ
        step = step_s * D if scaling else step_s
        o = s.dogleg_step(mu, radius)
        assert o["step_type"] == typ and not o["reused"]
        print(man, scaling, typ, o, "pred", tr.predicted_reduction(step_s, g, H))
        assert o["alpha"] == pytest.approx(alpha, rel=1e-9)
        assert o["predicted_reduction"] == pytest.approx(tr.predicted_reduction(step_s, g, H), rel=1e-9)
        assert o["gradient_norm"] == pytest.approx(np.linalg.norm(g), rel=1e-11)
        assert o["step_norm"] == pytest.approx(np.linalg.norm(step), rel=1e-10)
        assert o["scaled_step_norm"] == pytest.approx(np.linalg.norm(step_s), rel=1e-10)
        if typ == tr.DOG_LEG:
            assert o["beta"] == pytest.approx(beta, rel=1e-9)
        st = s.step_stats()
        assert st == (o["gradient_norm"], o["step_norm"], o["predicted_reduction"])
        trial = s.eval_step()
        s.commit_step()
        new = s.get_parameters()
        assert s.compute_cost() == pytest.approx(trial, rel=1e-12)
        got = tc.applied_step(prob, p0, new)
        want = np.where(mask, 0.0, step)
        print("   applied step", rel(got, want), "masked", np.abs(got[mask]).max())
        assert rel(got, want) < 1e-10
        assert np.abs(got[mask]).max() <= 1e-13   # (read back through Log: a few ulp of the pose coordinates, O(10))
        s.set_parameters(p0)
    s.close()


@pytest.mark.parametrize("man", MANIFOLDS)
def test_reuse_after_a_rejected_step(man):
    """A step far too long is rejected; the reused step at half the radius is the numpy step from the cached h, p_c, g, and
    costs no assembly, factorisation or triangular solve."""
    prob, p0 = tc.problem(man)
    mu = 1e-2
    P, H, g, D, h, alpha, p_c = tc.first_linearisation(prob, p0, True, mu)
    hn, pn = np.linalg.norm(h), np.linalg.norm(p_c)
    s = solver(prob, p0)
    s.apply_column_scaling(D)
    s.enable_stage_timing(True)
    cost0 = s.compute_cost()
    radius = 0.9 * hn   # a dog leg
    o = s.dogleg_step(mu, radius)
    trial = s.eval_step()
    s.discard_step()                       # (whatever rho was: the point of this test is the reuse that follows)
    before = s.stage_times()
    r = s.dogleg_step(mu, 0.5 * radius, reuse=True)
    after = s.stage_times()
    for stage in ("assemble", "factor", "tri_solve"):
        assert after[stage][1] == before[stage][1], (stage, before, after)
    assert after["cost"][1] == before["cost"][1] + 1 and after["retract"][1] == before["retract"][1] + 1
    step_s, typ, beta = tr.dog_leg_step(-g, p_c, h, 0.5 * radius)
    assert r["reused"] and r["step_type"] == typ
    assert r["predicted_reduction"] == pytest.approx(tr.predicted_reduction(step_s, g, H), rel=1e-9)
    assert r["step_norm"] == pytest.approx(np.linalg.norm(step_s * D), rel=1e-10)
    s.eval_step(); s.commit_step()
    # (the rejected step was undone by the inverse retraction: the start is p0 up to its rounding)
    assert rel(tc.applied_step(prob, p0, s.get_parameters()), step_s * D) < 1e-9
    # a second reuse after the commit -- the reference's quirk: the cache outlives an accepted poor step
    r2 = s.dogleg_step(mu, 0.25 * radius, reuse=True)
    assert r2["reused"] and r2["gradient_norm"] == r["gradient_norm"]
    s.close()


@pytest.mark.parametrize("man", MANIFOLDS)
def test_reuse_needs_a_cache_that_is_still_valid(man):
    """What voids the cached solve and what leaves it alone, call by call (the bundle-adjustment test of this name, on a pose graph)."""
    prob, p0 = tc.problem(man)
    n = prob.dof * prob.data.n_v
    s = solver(prob, p0)
    assert kind_of(s.dogleg_step, 1e-2, 1.0, reuse=True) == "InvalidState"     # before any fresh solve
    rng = np.random.default_rng(7)
    a, b = rng.normal(size=n), rng.normal(size=n)
    voids = (lambda: s.set_parameters(p0), lambda: s.set_loss(Loss(capi.LOSS_HUBER, 1.0)), lambda: s.set_priors(prob.priors),
             lambda: s.set_information(None), lambda: s.apply_column_scaling(np.full(n, 0.5)), lambda: s.apply_column_scaling(None),
             lambda: s.solve_augmented_equation(1e-3), lambda: s.get_hessian(0.0), lambda: s.compute_column_norms())
    for void in voids:
        s.dogleg_step(1e-2, 1.0)
        assert s.dogleg_step(1e-2, 0.5, reuse=True)["reused"]          # (the cache is there)
        void()
        assert kind_of(s.dogleg_step, 1e-2, 0.25, reuse=True) == "InvalidState"
    keeps = (lambda: s.jv_gram(a, b), lambda: (s.eval_step(), s.discard_step()), lambda: (s.eval_step(), s.commit_step()))
    for keep in keeps:
        s.set_parameters(p0)
        s.dogleg_step(1e-2, 1.0)
        assert s.dogleg_step(1e-2, 0.5, reuse=True)["reused"]
        keep()
        assert s.dogleg_step(1e-2, 0.25, reuse=True)["reused"]
    s.close()


@pytest.mark.parametrize("man", MANIFOLDS)
def test_dogleg_step_does_not_depend_on_one_wait(man):
    """A fresh blended step and a reused one at half the radius, with the flags waited for where they are raised ("one_wait" 0)
    and with the one wait of the default: SE2 has no atomics on either path and is held to the same bits; SE3 scatters its
    assembly with fp64 atomics and is held to this file's bounds (step 1e-10, scalars 1e-9).  The pose-graph surface has no
    export_step: the step is compared as the parameters it leaves behind a commit."""
    prob, p0 = tc.problem(man)
    mu = 1.0   # (cond(H + mu I) <= 1e5 in the plain variables, as test_dogleg_step_of_every_type_against_numpy has it)
    P, H, g, D, h, alpha, p_c = tc.first_linearisation(prob, p0, False, mu)
    hn, pn = np.linalg.norm(h), np.linalg.norm(p_c)
    assert np.linalg.cond(H + mu * np.eye(P.n)) <= 1e5 and pn < hn, (pn, hn)
    radius = 0.5 * (pn + hn)   # inside the Gauss-Newton norm, outside the Cauchy point: the leg is blended
    runs = []
    for opts in ({"one_wait": 0}, {}):
        s = GpuSparseCholeskySolver(0)
        for k, v in opts.items():
            s.with_option(k, v)
        s.initialize_structure(prob)
        s.set_parameters(p0)
        fresh = s.dogleg_step(mu, radius)
        assert fresh["step_type"] == tr.DOG_LEG and not fresh["reused"]
        stats_f, trial_f = s.step_stats(), s.eval_step()
        s.commit_step()
        after_f = s.get_parameters()
        s.set_parameters(p0)
        s.dogleg_step(mu, radius)
        s.eval_step(); s.discard_step()
        reused = s.dogleg_step(mu, 0.5 * radius, reuse=True)
        assert reused["reused"]
        stats_r, trial_r = s.step_stats(), s.eval_step()
        s.commit_step()
        after_r = s.get_parameters()
        s.close()
        runs.append((fresh, stats_f, trial_f, after_f, reused, stats_r, trial_r, after_r))
    off, on = runs
    print(man, "one_wait 0", off[0], off[4], "\n   default", on[0], on[4])
    if man == "se2":
        for x, y in zip(off, on):
            assert np.array_equal(x, y) if isinstance(x, np.ndarray) else x == y, (x, y)
        return
    for i in (0, 4):      # the step dictionaries
        assert off[i]["step_type"] == on[i]["step_type"] and off[i]["reused"] == on[i]["reused"]
        for k in ("gradient_norm", "step_norm", "predicted_reduction", "alpha", "beta", "scaled_step_norm"):
            assert off[i][k] == pytest.approx(on[i][k], rel=1e-9), (i, k)
    for i in (1, 5):      # step_stats
        assert off[i] == pytest.approx(on[i], rel=1e-9)
    for i in (2, 6):      # eval_step
        assert off[i] == pytest.approx(on[i], rel=1e-9)
    for i in (3, 7):      # the applied step
        assert rel(tc.applied_step(prob, p0, off[i]), tc.applied_step(prob, p0, on[i])) < 1e-10


# ---- histories -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("scaling", [False, True], ids=["plain", "jacobi-scaling"])
@pytest.mark.parametrize("man", MANIFOLDS)
def test_dogleg_history_against_the_numpy_loop(man, scaling):
    ref = tc.dogleg_reference(man, scaling)
    assert ref["margins"].min() > 1e-6
    prob, p0 = tc.problem(man)
    s = solver(prob, p0)
    res, H, c = s.dogleg_optimize(DogLegConfig(max_iterations=tc.DL_ITERS, trust_region_radius=ref["radius0"], use_jacobi_scaling=scaling))
    R = ref["history"]
    print(man, scaling, res.status, res.iterations, ref["status"], ref["iterations"], "types", R[:, 9], "reused", R[:, 11])
    assert (res.status, res.iterations) == (ref["status"], ref["iterations"])
    assert res.jacobian_evaluations == res.iterations and res.cost_evaluations == res.iterations + 1
    assert np.array_equal(H[:, [4, 9, 11]], R[:, [4, 9, 11]])   # accepted, step type, reused
    assert np.array_equal(H[:, 2], R[:, 2])                     # mu
    print("cost", np.abs(H[:, 0] / R[:, 0] - 1).max(), "radius", np.abs(H[:, 1] / R[:, 1] - 1).max())
    np.testing.assert_allclose(H[:, 0], R[:, 0], rtol=1e-7)
    np.testing.assert_allclose(H[:, 1], R[:, 1], rtol=1e-7)
    assert c.trust_region_radius == pytest.approx(ref["radius"], rel=1e-7) and c.mu == ref["mu"]
    assert res.successful_steps == int(R[:, 4].sum()) and res.unsuccessful_steps == int((R[:, 4] == 0).sum())
    s.close()


@pytest.mark.parametrize("scaling", [False, True], ids=["plain", "jacobi-scaling"])
@pytest.mark.parametrize("man", MANIFOLDS)
def test_gauss_newton_history_against_the_numpy_loop(man, scaling):
    ref = tc.gauss_newton_reference(man, scaling)
    prob, _ = tc.problem(man)
    s = solver(prob, ref["start"])
    res, H, _ = s.gn_optimize(GaussNewtonConfig(max_iterations=6, use_jacobi_scaling=scaling))
    R = ref["history"]
    print(man, scaling, res.status, res.iterations, H[:, 0], R[:, 0])
    assert (res.status, res.iterations) == (ref["status"], ref["iterations"])
    assert res.jacobian_evaluations == res.iterations
    np.testing.assert_allclose(H[:, 0], R[:, 0], rtol=1e-7)
    # |g|, |step|: 1e-6 of their own size, and of the first iteration's where the run has converged and they are rounding residue
    np.testing.assert_allclose(H[:, [4, 5]], R[:, [4, 5]], rtol=1e-6, atol=1e-10 * R[0, 4])
    assert (H[:, 3] == 1).all()
    s.close()


@pytest.mark.parametrize("man", MANIFOLDS)
def test_gauss_newton_fails_on_a_gauge_free_graph(man):
    prob, P = singular_case(man)
    Hn, _ = P.normal_equations()
    assert tr.solve_damped(Hn, np.zeros(P.n), 0.0) is None   # numpy's Cholesky meets the zero pivot
    s = solver(prob, prob.data.poses)
    res, H, _ = s.gn_optimize(GaussNewtonConfig())
    err = s._h.L.apexgpu_pg_last_error(s._h.h).decode()
    print(res.status, res.iterations, err)
    assert res.status == 100 and res.iterations == 0
    assert "Cholesky factorization failed" in err
    with pytest.raises(capi.LinAlgError) as e:
        s.dogleg_step(0.0, 1.0)
    assert e.value.kind == "SingularMatrix"
    # Dog-Leg mends it with its mu: the first solve at mu = 1e-4 goes through
    res, _, _ = s.dogleg_optimize(DogLegConfig(max_iterations=3))
    assert res.status != 100
    s.close()


# ---- wrong-state calls ---------------------------------------------------------------------------------------------------------
def test_wrong_state_calls():
    prob, p0 = tc.problem("se2")
    s = GpuSparseCholeskySolver(0).initialize_structure(prob)
    with pytest.raises(capi.LinAlgError) as e:
        s.dogleg_step(1e-4, 1.0)
    assert e.value.kind == "InvalidState"
    with pytest.raises(capi.LinAlgError) as e:
        s.jv_gram(np.zeros(180), np.zeros(180))
    assert e.value.kind == "InvalidState"
    s.set_parameters(p0)
    with pytest.raises(capi.LinAlgError) as e:
        s.dogleg_step(1e-4, 1.0, reuse=True)
    assert e.value.kind == "InvalidState"
    s.dogleg_step(1e-4, 1.0)
    s.get_hessian(0.0)   # an export assembles: the cached gradient is gone
    with pytest.raises(capi.LinAlgError) as e:
        s.dogleg_step(1e-4, 0.5, reuse=True)
    assert e.value.kind == "InvalidState"
    for call, cfg in ((s.gn_optimize, GaussNewtonConfig(variant=1)), (s.dogleg_optimize, DogLegConfig(variant=2))):
        with pytest.raises(capi.LinAlgError) as e:
            call(cfg)
        assert e.value.kind == "InvalidInput"
    with pytest.raises(capi.LinAlgError) as e:
        s.dogleg_step(1e-4, -1.0)
    assert e.value.kind == "InvalidInput"
    s.close()


# ---- LM is what it was ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("man", MANIFOLDS)
def test_lm_before_and_after_a_dogleg_run_on_one_handle(man):
    prob, p0 = tc.problem(man)
    cfg = LevenbergMarquardtConfig(max_iterations=8)
    lone = solver(prob, p0)
    _, H_lone, _ = lone.lm_optimize(cfg)
    lone.close()
    s = solver(prob, p0)
    _, H_before, _ = s.lm_optimize(cfg)
    s.set_parameters(p0)
    s.dogleg_optimize(DogLegConfig(max_iterations=6, trust_region_radius=tc.dogleg_reference(man, False)["radius0"]))
    s.set_parameters(p0)
    _, H_after, _ = s.lm_optimize(cfg)
    s.close()
    assert H_before.shape == H_after.shape == H_lone.shape
    if man == "se2":   # the SE2 assembly has no atomics: bit for bit
        assert np.array_equal(H_before, H_lone) and np.array_equal(H_after, H_lone)
    else:              # SE3 scatters with fp64 atomics: the LM-history bounds (cost 1e-7)
        for H in (H_before, H_after):
            np.testing.assert_allclose(H[:, 0], H_lone[:, 0], rtol=1e-7)
            assert np.array_equal(H[:, 3], H_lone[:, 3])
