"""Dog-Leg on bundle adjustment, on the device, against tests/np_ref_ba_tr.py (needs a real MI355X: `pytest -m gpu`).

Bounds, as tests/test_gpu_trust_region.py holds the pose graphs to: the Gram sums 1e-12 relative (the cross term normwise, against
|J a| |J b|); the Dog-Leg step 1e-10 relative where cond(H_s + mu I) <= 1e5 (asserted on the numpy matrix; mu is the smallest
power of ten that reaches it -- 1e-4 in the scaled variables, 10 to 1e4 in pixels), alpha / beta / predicted reduction 1e-9, norms
1e-10; the trial cost 1e-12; histories: cost and radius 1e-7, mu / type / accepted / reused exactly."""
import ctypes as C

import numpy as np
import pytest

import fixed_masks as fm
import np_ref
import np_ref_ba_tr as bt
import np_ref_trust_region as tr
from apex_solver_amd import capi
from apex_solver_amd.loss import Loss
from apex_solver_amd.pose_graph import DogLegConfig
from apex_solver_amd.solver import (DogLeg, GpuSchurComplementSolver, LevenbergMarquardtConfig, OptimizationType, SchurVariant)

pytestmark = pytest.mark.gpu
NO_WORK = ("cam_reduce", "landmark_reduce", "schur_scatter", "factor", "tri_solve", "back_substitute")


def rel(a, b):
    a = np.asarray(a, dtype=np.float64); b = np.asarray(b, dtype=np.float64)
    return float(np.linalg.norm(a - b) / max(np.linalg.norm(b), 1e-300))


def device(P, options=None, shard=None):
    s = GpuSchurComplementSolver(0)
    for k, v in (options or {}).items():
        s.with_option(k, v)
    if shard:
        s.with_shard(*shard)
    s.initialize_structure(bt.device_problem(P))
    s.set_parameters(*P.params)
    return s


def kind_of(call, *a, **k):
    with pytest.raises(capi.LinAlgError) as e:
        call(*a, **k)
    return e.value.kind


# ---- jv_gram -------------------------------------------------------------------------------------------------------------------
def gram_problem(name):
    if name.startswith("golden:"):
        d, opt, delta, _ = bt.golden_data(name[7:])
        return bt.BaProblem(d, opt, bt.huber(delta), bt.gauge(d))
    if name.startswith("mode:"):   # every OptimizationType on the self-calibration golden's data
        d, _, delta, _ = bt.golden_data("ba6x40_selfcal")
        return bt.BaProblem(d, OptimizationType[name[5:]], bt.huber(delta), bt.gauge(d))
    if name == "custom-noloss":
        return bt.BaProblem(bt.custom_data(), OptimizationType.SelfCalibration, None)
    if name == "custom-ba-noloss":
        return bt.BaProblem(bt.custom_data(), OptimizationType.BundleAdjustment, None)
    d = bt.custom_data(outlier_every=5)
    loss = bt.huber(1.0) if name == "custom-huber-outliers" else Loss(capi.LOSS_CAUCHY, 2.0)   # Cauchy: the general instantiation
    return bt.BaProblem(d, OptimizationType.SelfCalibration if name != "custom-ba-cauchy" else OptimizationType.BundleAdjustment, loss)


GRAM_CASES = (["golden:ba6x40_selfcal", "golden:ba6x40_ba", "golden:ba9x120_selfcal_behind"] + ["mode:" + t.name for t in OptimizationType]
              + ["custom-noloss", "custom-ba-noloss", "custom-huber-outliers", "custom-cauchy", "custom-ba-cauchy"])


@pytest.mark.parametrize("name", GRAM_CASES)
def test_jv_gram_against_dense_numpy(name):
    P = gram_problem(name)
    r, J = P.jacobian()
    J = J.toarray()
    if name.endswith("behind"):
        valid = np_ref.project(*P.params, P.ci, P.pi)[1]
        assert (~valid).any() and not J[np.repeat(~valid, 2)].any()   # zero rows for the points behind their camera
    if name == "custom-huber-outliers":
        s2 = np.sum(np_ref.residuals(*P.params, P.ci, P.pi, P.d.obs_uv, huber_delta=0)[0] ** 2, axis=1)
        assert (s2 > 1.0).sum() >= 20 and (s2 < 1.0).sum() >= 20
    s = device(P)
    rng = np.random.default_rng(5)
    a, b = rng.normal(size=P.n), rng.normal(size=P.n)
    g = J.T @ r
    for x, y in ((a, b), (g, b), (g, g)):
        u, w = J @ x, J @ y
        got = s.jv_gram(x, y)
        want = (u @ u, u @ w, w @ w)
        print(name, got, want)
        assert got[0] == pytest.approx(want[0], rel=1e-12, abs=0.0) and got[2] == pytest.approx(want[2], rel=1e-12, abs=0.0)
        assert abs(got[1] - want[1]) <= 1e-12 * np.linalg.norm(u) * np.linalg.norm(w)
        assert s.jv_gram(x, y) == got   # no atomics, one order of summation: the same bits
    assert s.jv_gram(np.zeros(P.n), np.zeros(P.n)) == (0.0, 0.0, 0.0)
    s.close()


# ---- dogleg_step ---------------------------------------------------------------------------------------------------------------
STEP_CASES = ["golden:ba6x40_selfcal", "golden:ba6x40_ba", "golden:ba9x120_selfcal_behind", "custom-huber-outliers", "custom-ba-cauchy"]


def masked(P, seed=4):
    m = fm.with_gauge(fm.asymmetric(P.d.n_cam, P.d.n_pt, seed))
    return bt.BaProblem(P.d, P.opt, P.loss, m, P.params)


def oracle_applied(ora, P, start, step):
    """the C oracle applying `step` from `start` under P's masks: the storage convention of the device (raw quaternion product)"""
    lay, m = P.lay, P.masks
    o = ora.OracleProblem(P.d.n_cam, P.d.n_pt, P.d.cam_idx, P.d.pt_idx, P.d.obs_uv, lay.intr_col, lay.pose_col, lay.pt_col,
                          mode="selfcal" if P.selfcal else "ba", huber_delta=1.0, fix_pose=m["pose"], fix_intr=m["intr"], fix_pt=m["pt"])
    o.set_params(*start)
    o.apply_step(step, 1.0)
    return o.get_params()


@pytest.mark.parametrize("scaling", [False, True], ids=["plain", "jacobi-scaling"])
@pytest.mark.parametrize("name", STEP_CASES)
def test_dogleg_step_of_every_type_against_numpy(oracle, name, scaling):
    P = masked(gram_problem(name))
    start = P.params
    tr._init_scaling(P, scaling)
    H, g = P.normal_equations()
    D = P.scaling
    mu = bt.mu_for_condition(H)
    h = tr.solve_damped(H, g, mu)
    alpha, p_c = tr.cauchy_point(H, g)
    cond = np.linalg.cond(H + mu * np.eye(P.n))
    hn, pn = np.linalg.norm(h), np.linalg.norm(p_c)
    print(name, scaling, "mu", mu, "cond", cond, "|h|", hn, "|p_c|", pn)
    assert cond <= 1e5 and pn < hn, (cond, pn, hn)
    mask = P.mask_vector()
    fp, fi, fl = (P.masks[k].astype(bool) for k in ("pose", "intr", "pt"))
    assert fp.any() and fi.any() and fl.any()
    s = device(P)
    if scaling:
        s.apply_column_scaling(D)
    for radius, typ in ((2.0 * hn, tr.GAUSS_NEWTON), (0.5 * pn, tr.STEEPEST_DESCENT), (0.5 * (pn + hn), tr.DOG_LEG)):
        step_s, t, beta = tr.dog_leg_step(-g, p_c, h, radius)
        assert t == typ
        step = step_s * D if scaling else step_s
        o = s.dogleg_step(mu, radius)
        pred = tr.predicted_reduction(step_s, g, H)
        print("  ", typ, o, "pred", pred)
        assert o["step_type"] == typ and not o["reused"]
        assert o["alpha"] == pytest.approx(alpha, rel=1e-9)
        assert o["predicted_reduction"] == pytest.approx(pred, rel=1e-9)
        assert o["gradient_norm"] == pytest.approx(np.linalg.norm(g), rel=1e-10)
        assert o["step_norm"] == pytest.approx(np.linalg.norm(step), rel=1e-10)
        assert o["scaled_step_norm"] == pytest.approx(np.linalg.norm(step_s), rel=1e-10)
        if typ == tr.DOG_LEG:
            assert o["beta"] == pytest.approx(beta, rel=1e-9)
        assert s.step_stats() == (o["gradient_norm"], o["step_norm"], o["predicted_reduction"])
        y, _ = s.export_step()                      # the blended step as the solver exports steps: in the scaled variables
        got_step = y * D if scaling else y
        if not P.selfcal:                           # (the intrinsic columns exist for the caller only: zero in both)
            assert not got_step[P.lay.intr_col[:, None] + np.arange(3)[None]].any()
        print("   step", rel(got_step, step))
        assert rel(got_step, step) < 1e-10
        trial = s.eval_step()
        s.commit_step()
        assert s.compute_cost() == pytest.approx(trial, rel=1e-12)
        pg, ig, lg = s.get_parameters()
        # fixed DOF do not move: landmarks and intrinsics bit for bit, a fully fixed pose too; the free ones are the device's own
        # step applied under the masks, poses to the se3_plus bound of tests/test_gpu_fixed_dofs.py
        assert np.array_equal(lg[fl], start[2][fl]) and np.array_equal(ig[fi], start[1][fi])
        full = fp.all(axis=1)
        assert full.any() and np.array_equal(pg[full], start[0][full])
        po, io, lo = oracle_applied(oracle, P, start, got_step)
        assert np.allclose(pg, po, rtol=1e-13, atol=1e-15)
        for got, want, dlt in ((lg, lo, got_step[P.lay.pt_col[:, None] + np.arange(3)[None]]),
                               (ig, io, got_step[P.lay.intr_col[:, None] + np.arange(3)[None]])):
            assert (np.abs(got - want) <= 2.0 ** -52 * (np.abs(dlt) + np.abs(want))).all()   # (y s: two roundings from the device's d)
        s.set_parameters(*start)
        if scaling:
            s.apply_column_scaling(D)
    s.close()


def test_reuse_after_a_rejected_step():
    """The reused step at half the radius is the numpy step from the cached h, p_c, g, and costs no assembly, factorisation, sweep
    or back-substitution."""
    P, _ = bt.history_problem("selfcal-huber-scaled")
    start = P.params
    mu = 1e-4
    H, g, D, h, alpha, p_c = bt.first_linearisation(P, True, mu)
    hn = np.linalg.norm(h)
    s = device(P)
    s.apply_column_scaling(D)
    s.enable_stage_timing(True)
    radius = 0.9 * hn
    s.dogleg_step(mu, radius)
    s.eval_step()
    s.discard_step()                       # (whatever rho was: the point of this test is the reuse that follows)
    before = s.stage_times()
    r = s.dogleg_step(mu, 0.5 * radius, reuse=True)
    after = s.stage_times()
    for stage in NO_WORK:
        assert after[stage][1] == before[stage][1], (stage, before, after)
    assert after["cost"][1] == before["cost"][1] + 1 and after["retract"][1] == before["retract"][1] + 1
    assert after["step_stats"][1] == before["step_stats"][1] + 1
    step_s, typ, beta = tr.dog_leg_step(-g, p_c, h, 0.5 * radius)
    assert r["reused"] and r["step_type"] == typ
    assert r["predicted_reduction"] == pytest.approx(tr.predicted_reduction(step_s, g, H), rel=1e-9)
    assert r["step_norm"] == pytest.approx(np.linalg.norm(step_s * D), rel=1e-10)
    assert r["gradient_norm"] == pytest.approx(np.linalg.norm(g), rel=1e-10)
    y, _ = s.export_step()
    assert rel(y, step_s) < 1e-10
    trial = s.eval_step(); s.commit_step()
    P.apply_step(step_s * D)
    assert trial == pytest.approx(P.cost(), rel=1e-9)
    # a second reuse after the commit -- the reference's quirk: the cache outlives an accepted poor step
    r2 = s.dogleg_step(mu, 0.25 * radius, reuse=True)
    assert r2["reused"] and r2["gradient_norm"] == r["gradient_norm"]
    s.close()


# ---- histories -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", list(bt.HISTORY_CASES))
def test_dogleg_history_against_the_numpy_loop(case):
    ref = bt.dogleg_reference(case)
    assert ref["margins"].min() > 1e-6
    P, scaling = bt.history_problem(case)
    cfg = DogLegConfig(max_iterations=bt.DL_ITERS, trust_region_radius=ref["radius0"], use_jacobi_scaling=scaling, **bt.MU.get(case, {}))
    out = DogLeg.with_config(cfg).optimize(bt.device_problem(P), initial_values=P.params)
    H, R = out.history, ref["history"]
    print(case, out.status, out.iterations, ref["status"], ref["iterations"], "types", R[:, 9], "reused", R[:, 11])
    assert (out.status.value, out.iterations) == (ref["status"], ref["iterations"])
    assert out.jacobian_evaluations == out.iterations and out.cost_evaluations == out.iterations + 1
    assert np.array_equal(H[:, [4, 9, 11]], R[:, [4, 9, 11]])   # accepted, step type, reused
    assert np.array_equal(H[:, 2], R[:, 2])                     # mu
    print("cost", np.abs(H[:, 0] / R[:, 0] - 1).max(), "radius", np.abs(H[:, 1] / R[:, 1] - 1).max())
    np.testing.assert_allclose(H[:, 0], R[:, 0], rtol=1e-7)
    np.testing.assert_allclose(H[:, 1], R[:, 1], rtol=1e-7)
    assert out.final_radius == pytest.approx(ref["radius"], rel=1e-7) and out.final_mu == ref["mu"]   # written back into the config
    assert out.successful_steps == int(R[:, 4].sum()) and out.unsuccessful_steps == int((R[:, 4] == 0).sum())


# ---- state ---------------------------------------------------------------------------------------------------------------------
def test_refusals_leave_a_pending_step_as_it_was():
    P, _ = bt.history_problem("selfcal-huber-plain")
    s = device(P)
    s.solve_augmented_equation(1e-3)
    stats = s.step_stats()
    step = s.export_step()[0]
    assert kind_of(s.dogleg_step, 1e-4, -1.0) == "InvalidInput" and kind_of(s.dogleg_step, 1e-4, 0.0) == "InvalidInput"
    assert kind_of(s.dogleg_step, -1e-4, 1.0) == "InvalidInput"
    assert kind_of(s.dogleg_optimize, DogLegConfig(variant=1)) == "InvalidInput"
    assert kind_of(s.dogleg_optimize, DogLegConfig(trust_region_radius=0.0)) == "InvalidInput"
    assert kind_of(s.dogleg_step, 1e-4, 1.0, reuse=True) == "InvalidState"
    assert s.step_stats() == stats and np.array_equal(s.export_step()[0], step)
    trial = s.eval_step(); s.commit_step()       # the pending step is still there to be evaluated and kept
    assert s.compute_cost() == pytest.approx(trial, rel=1e-12)
    s.close()


def test_matrix_free_and_sharded_handles_refuse():
    P, _ = bt.history_problem("selfcal-huber-plain")
    # "matrix_free_only", the automatic fallback (forced by cost on this small problem), and two ranks
    probe = device(P)
    vi = probe.variant_info()
    probe.close()
    pct = int(np.floor(1000.0 * vi["predicted_direct_ms"] / vi["predicted_matrix_free_ms"]))
    assert pct >= 1, vi
    for opts, shard in (({"matrix_free_only": 1}, None), ({"variant_cost_permille": pct}, None), (None, (0, 2))):
        s = device(P, opts, shard)
        if opts and "variant_cost_permille" in opts:
            assert s.variant_info()["variant_used"] == "Implicit"
        if shard is None:
            s.with_variant(SchurVariant.Implicit).solve_augmented_equation(1e-3)
            stats = s.step_stats()
        assert kind_of(s.dogleg_step, 1e-4, 1.0) == "InvalidState"
        assert kind_of(s.dogleg_optimize, DogLegConfig()) == "InvalidState"
        msg = s._h.L.apexgpu_last_error(s._h.h).decode()
        assert ("single rank only" in msg) == (shard is not None), msg
        if shard is None:
            assert s.step_stats() == stats
        s.close()


def test_reuse_needs_a_cache_that_is_still_valid():
    P, _ = bt.history_problem("selfcal-huber-plain")
    s = device(P)
    assert kind_of(s.dogleg_step, 1e-4, 1.0, reuse=True) == "InvalidState"     # before any fresh solve
    voids = (lambda: s.set_parameters(*P.params), lambda: s.set_loss(bt.huber(2.0)), lambda: s.apply_column_scaling(np.full(P.n, 0.5)),
             lambda: s.apply_column_scaling(None), lambda: s.solve_augmented_equation(1e-3), lambda: s.assemble(1e-3),
             lambda: s.compute_column_norms(), lambda: s.get_schur(want_S=False))
    for void in voids:
        s.dogleg_step(1.0, 1.0)
        s.dogleg_step(1.0, 0.5, reuse=True)          # (the cache is there)
        void()
        assert kind_of(s.dogleg_step, 1.0, 0.25, reuse=True) == "InvalidState"
    s.dogleg_step(1.0, 1.0)
    s.dogleg_step(1.0, 0.5, reuse=True)
    s.jv_gram(np.ones(P.n), np.arange(P.n, dtype=np.float64))   # the parity export prices two vectors of its own: the cache stays
    assert s.dogleg_step(1.0, 0.25, reuse=True)["reused"]
    s.close()
    s = GpuSchurComplementSolver(0).initialize_structure(bt.device_problem(P))
    assert kind_of(s.dogleg_step, 1e-4, 1.0) == "InvalidState" and kind_of(s.jv_gram, np.zeros(P.n), np.zeros(P.n)) == "InvalidState"
    s.close()


def test_failed_factorisation_is_reported_without_the_ladder():
    """Landmarks-only columns and mu = 0: S = 0 on the camera side beyond its padding, the first pivot fails.  solve_augmented
    mends that with its ladder (last_reg > 0); dogleg_step reports it, and the loop's answer is a larger mu."""
    d, _, delta, _ = bt.golden_data("ba6x40_selfcal")
    P = bt.BaProblem(d, OptimizationType.OnlyLandmarks, bt.huber(delta), bt.gauge(d))
    kinds = []
    for opts in (None, {"one_wait": 0}):   # the flags read at the solve's one wait, and right behind the factorisation
        s = device(P, opts)
        kinds.append(kind_of(s.dogleg_step, 0.0, 1.0))
        assert kinds[-1] in ("FactorizationFailed", "SingularMatrix")
        assert s.info()["last_reg"] == 0.0
        assert kind_of(s.step_stats) == "InvalidState"
        s.dogleg_step(1e-4, 1.0)
        s.close()
    assert kinds[0] == kinds[1]


def test_dogleg_step_does_not_depend_on_one_wait():
    """A fresh blended step and a reused one at half the radius, with the flags waited for where they are raised ("one_wait" 0:
    Solver::solve_for_dogleg has a branch of its own for it) and with the one wait of the default.  Neither path has an atomic:
    the step dictionaries, export_step and eval_step are the same bits."""
    P = gram_problem("golden:ba6x40_selfcal")
    tr._init_scaling(P, False)
    H, g = P.normal_equations()
    mu = bt.mu_for_condition(H)
    h = tr.solve_damped(H, g, mu)
    _, p_c = tr.cauchy_point(H, g)
    hn, pn = np.linalg.norm(h), np.linalg.norm(p_c)
    assert pn < hn, (pn, hn)
    radius = 0.5 * (pn + hn)   # inside the Gauss-Newton norm, outside the Cauchy point: the leg is blended
    runs = []
    for opts in ({"one_wait": 0}, None):
        s = device(P, opts)
        fresh = s.dogleg_step(mu, radius)
        assert fresh["step_type"] == tr.DOG_LEG and not fresh["reused"]
        step_f, trial_f = s.export_step(), s.eval_step()
        s.discard_step()
        reused = s.dogleg_step(mu, 0.5 * radius, reuse=True)
        assert reused["reused"]
        step_r, trial_r = s.export_step(), s.eval_step()
        s.close()
        runs.append((fresh, step_f, trial_f, reused, step_r, trial_r))
    off, on = runs
    print("one_wait 0", off[0], off[3], "\n   default", on[0], on[3])
    for i in (0, 2, 3, 5):
        assert off[i] == on[i], (i, off[i], on[i])
    for i in (1, 4):
        assert np.array_equal(off[i][0], on[i][0]) and np.array_equal(off[i][1], on[i][1])


# ---- LM is what it was ---------------------------------------------------------------------------------------------------------
def test_lm_before_and_after_a_dogleg_run_on_one_handle():
    P, _ = bt.history_problem("selfcal-huber-plain")
    cfg = LevenbergMarquardtConfig(max_iterations=8)
    lone = device(P)
    _, H_lone, _ = lone.lm_optimize(cfg)
    lone.close()
    s = device(P)
    _, H_before, _ = s.lm_optimize(cfg)
    s.set_parameters(*P.params)
    s.dogleg_optimize(DogLegConfig(max_iterations=6, trust_region_radius=bt.dogleg_reference("selfcal-huber-plain")["radius0"]))
    s.set_parameters(*P.params)
    _, H_after, _ = s.lm_optimize(cfg)
    s.close()
    assert H_before.shape == H_after.shape == H_lone.shape
    for H in (H_before, H_after):   # (the bounds for atomically scattered sums: cost 1e-7, the same decisions)
        print("LM cost vs a fresh handle", np.abs(H[:, 0] / H_lone[:, 0] - 1).max(), "bitwise", np.array_equal(H, H_lone))
        np.testing.assert_allclose(H[:, 0], H_lone[:, 0], rtol=1e-7)
        assert np.array_equal(H[:, 3], H_lone[:, 3])


# ---- the raw ABI -----------------------------------------------------------------------------------------------------------------
def test_raw_abi_through_ctypes():
    """apexgpu_jv_gram, apexgpu_dogleg_step and apexgpu_dogleg_optimize called on a bare apexgpu_solver*, without solver.py."""
    P, _ = bt.history_problem("ba-noloss-plain")
    d, lay = P.d, P.lay
    L = capi.load()
    h = C.c_void_p()
    assert L.apexgpu_create(d.n_cam, d.n_pt, d.n_obs, P.opt.value, 0, C.byref(h)) == 0
    keep = [np.ascontiguousarray(a) for a in (d.cam_idx.astype(np.uint32), d.pt_idx.astype(np.uint32), d.obs_uv.astype(np.float64),
                                              lay.intr_col, lay.pose_col, lay.pt_col, P.masks["pose"], P.masks["intr"], P.masks["pt"])]
    assert L.apexgpu_set_structure(h, *[capi.ptr(a) for a in keep], -1.0) == 0
    assert L.apexgpu_dogleg_step(h, 1e-4, 1.0, 0, None) == -6          # no parameters yet
    par = [np.ascontiguousarray(x) for x in P.params]
    assert L.apexgpu_set_params(h, *[capi.ptr(x) for x in par]) == 0
    r, J = P.jacobian()
    J = J.toarray()
    a, b = J.T @ r, np.random.default_rng(1).normal(size=P.n)
    o3 = (C.c_double * 3)()
    assert L.apexgpu_jv_gram(h, capi.ptr(a), None, C.byref(o3)) == -5
    assert L.apexgpu_jv_gram(h, capi.ptr(a), capi.ptr(b), C.byref(o3)) == 0
    assert o3[0] == pytest.approx((J @ a) @ (J @ a), rel=1e-12) and o3[2] == pytest.approx((J @ b) @ (J @ b), rel=1e-12)
    o8 = (C.c_double * 8)()
    assert L.apexgpu_dogleg_step(h, 1e-4, 1.0, 1, C.byref(o8)) == -6   # nothing to reuse
    assert L.apexgpu_dogleg_step(h, 1e-4, 1e9, 0, C.byref(o8)) == 0
    assert o8[3] == tr.GAUSS_NEWTON and o8[7] == 0.0 and o8[0] == pytest.approx(np.linalg.norm(a), rel=1e-10)
    assert L.apexgpu_dogleg_step(h, 1e-4, 1e-3 * o8[6], 1, C.byref(o8)) == 0
    assert o8[7] == 1.0 and o8[3] == tr.STEEPEST_DESCENT
    ref = bt.dogleg_reference("ba-noloss-plain")
    cfg = DogLegConfig(max_iterations=bt.DL_ITERS, trust_region_radius=ref["radius0"], use_jacobi_scaling=False, **bt.MU["ba-noloss-plain"]).to_c()
    res = capi.LmResultC()
    hist = (capi.DlIterC * 16)()
    assert L.apexgpu_dogleg_optimize(h, None, C.byref(res), None, 0) == -5
    assert L.apexgpu_dogleg_optimize(h, C.byref(cfg), C.byref(res), C.cast(hist, C.c_void_p), 16) == 0
    assert (res.status, res.iterations) == (ref["status"], ref["iterations"])
    assert res.final_cost == pytest.approx(ref["final_cost"], rel=1e-7)
    assert hist[0].cost == pytest.approx(ref["history"][0, 0], rel=1e-7) and cfg.mu == ref["mu"]
    L.apexgpu_destroy(h)
