"""Prior factors on camera poses and intrinsics in bundle adjustment (apexgpu_set_pose_priors / _set_intrinsic_priors; DESIGN.md
§17) on the device, against tests/ba_prior_ref.py (needs a real MI355X: `pytest -m gpu`).

Bounds are those the same quantities are held to without priors: residuals, gradient, S, the matvecs, column norms and the cost
1e-12, g_red 1e-10 (tests/test_gpu_parity.py); the Gram sums 1e-12 (tests/test_gpu_ba_trust_region.py); the step at lambda = 1e4,
where cond(S) <= 1e5, 1e-10 for the Cholesky variant and 1e-9 for the two PCG variants run to 1e-13 (tests/test_gpu_parity.py);
covariance blocks 1e-10 at lambda = 1e4 (tests/test_gpu_covariance.py); LM / Dog-Leg histories: decisions exactly, costs 1e-7
(tests/test_gpu_ba_loss.py, tests/test_gpu_ba_trust_region.py)."""
import ctypes as C
import functools
import json
import os
import subprocess

import numpy as np
import pytest
import scipy.sparse as sp

import ba_custom
import ba_prior_ref as br
import fixed_masks as fm
import np_ref
import np_ref_ba_tr as bt
import np_ref_trust_region as tr
from apex_solver_amd import capi
from apex_solver_amd.loss import Loss
from apex_solver_amd.pose_graph import DogLegConfig
from apex_solver_amd.solver import (DogLeg, GpuSchurComplementSolver, LevenbergMarquardtConfig, OptimizationType, SchurVariant)

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LAM = 1e4
SELFCAL, BA = OptimizationType.SelfCalibration, OptimizationType.BundleAdjustment


def rel(a, b):
    a = np.ravel(a); b = np.ravel(b)
    return float(np.linalg.norm(a - b) / max(np.linalg.norm(b), 1e-300))


@functools.lru_cache(maxsize=None)
def crafted(n_cam):
    """17 cameras at nine columns / 25 at six: the last cameras' columns lie in the second 144-row tile of S"""
    rng = np.random.default_rng(n_cam)
    lists = [sorted(rng.choice(n_cam, size=int(rng.integers(2, 7)), replace=False).tolist()) for _ in range(90)]
    lists += [[c, (c + 1) % n_cam, (c + 5) % n_cam] for c in range(n_cam)]   # every camera is observed
    return ba_custom.custom_problem(n_cam, lists, seed=11, noise=0.7, outlier_every=7)


def make_priors(d, n, seed, cams=None, intr=True, delta="mixed", weights=(1.0, 0.25, 7.0)):
    """n pose (and n intrinsics) priors near the start values; cams: the cameras to draw from (default: all, cycled so that
    n > n_cam puts several on one camera)"""
    rng = np.random.default_rng(seed)
    cams = np.arange(d.n_cam) if cams is None else np.asarray(cams)
    x = br.pose_vector(d.poses)
    pp, ip = [], []
    for k in range(n):
        c = int(cams[k % len(cams)])
        dl = None if delta is None or (delta == "mixed" and k % 2 == 0) else 0.05
        pp.append((c, x[c] + rng.normal(0, 0.03, 7), dl, float(weights[k % len(weights)])))
        if intr:
            dl = None if delta is None or (delta == "mixed" and k % 2 == 1) else 2.0
            ip.append((c, d.intr[c] + rng.normal(0, [3.0, 1e-3, 1e-4]), dl, float(weights[(k + 1) % len(weights)])))
    return pp, ip


def problem(kind, n_prior, seed=0, loss="huber", cams=None, **kw):
    if kind.startswith("golden"):
        d, opt, delta, _ = bt.golden_data("ba6x40_selfcal" if kind == "golden9" else "ba6x40_ba")
    else:
        d, opt, delta = crafted(17 if kind == "crafted9" else 25), SELFCAL if kind == "crafted9" else BA, 1.0
    L = {"huber": bt.huber(delta), "cauchy": Loss(capi.LOSS_CAUCHY, 2.0), None: None}[loss]
    pp, ip = make_priors(d, n_prior, seed, cams=cams, intr=opt == SELFCAL, **kw)
    return br.PriorBaProblem(d, opt, L, bt.gauge(d), pose_priors=pp, intr_priors=ip)


def device(P, variant=SchurVariant.Sparse, options=None, priors=True):
    s = GpuSchurComplementSolver(0).with_variant(variant)
    for k, v in (options or {}).items():
        s.with_option(k, v)
    s.initialize_structure(P.device_problem() if priors else bt.device_problem(P))
    s.set_parameters(*P.params)
    return s


def kind_of(call, *a, **k):
    with pytest.raises(capi.LinAlgError) as e:
        call(*a, **k)
    return e.value.kind


CASES = {
    "golden9-1": ("golden9", 1, {}), "golden9-2-same-camera": ("golden9", 2, dict(cams=[3])), "golden9-fixed-camera": ("golden9", 2, dict(cams=[0])),
    "golden9-64": ("golden9", 64, {}), "golden9-65-cauchy": ("golden9", 65, dict(loss="cauchy")), "golden9-130": ("golden9", 130, {}),
    "golden6-1": ("golden6", 1, {}), "golden6-65": ("golden6", 65, {}), "golden6-130-cauchy": ("golden6", 130, dict(loss="cauchy")),
    "crafted9-last-camera": ("crafted9", 2, dict(cams=[16, 0])), "crafted9-65": ("crafted9", 65, {}),
    "crafted6-last-camera": ("crafted6", 2, dict(cams=[24, 0])), "crafted6-130-w1-nohuber": ("crafted6", 130, dict(delta=None, weights=(1.0,))),
}


@pytest.mark.parametrize("case", list(CASES))
def test_every_export_against_the_reference(case):
    kind, n, kw = CASES[case]
    P = problem(kind, n, **kw)
    s = device(P)
    lay, nc = P.lay, P.lay.cam_dof
    rp, ri = s.prior_residuals()
    wp, wi = P.prior_residuals()
    assert rel(rp, wp) < 1e-12 and (len(wi) == 0 or rel(ri, wi) < 1e-12)
    assert s.compute_cost() == pytest.approx(P.cost(), rel=1e-12)
    r, J = P.jacobian()
    dx, g, H = np_ref.direct_step(J, r, LAM)
    S, gred = np_ref.schur_dense(H, g, nc, LAM)
    step = s.solve_augmented_equation(LAM)
    errs = dict(grad=rel(s.get_gradient(), g), step=rel(step, dx))
    trial = s.eval_step()   # (before the exports: they void the step)
    s.discard_step()
    Q = br.PriorBaProblem(P.d, P.opt, P.loss, P.masks, P.params, P.pose_priors, P.intr_priors)
    Q.apply_step(dx)
    dS, dg = s.get_schur()
    errs.update(S=rel(dS, S), gred=rel(dg, gred))
    Hd = s.get_hessian().toarray()
    errs["H"] = rel(Hd, H.toarray())
    x = np.random.default_rng(1).normal(size=nc)
    ye, yi = s.schur_matvec(LAM, x)
    errs.update(mv_explicit=rel(ye, S @ x), mv_implicit=rel(yi, S @ x))
    errs["norms"] = rel(s.compute_column_norms(), P.column_norms())
    a, b = np.random.default_rng(2).normal(size=(2, P.n))
    got, (want, u, w) = s.jv_gram(a, b), P.jv_gram(a, b)
    errs["gram"] = max(abs(got[0] / want[0] - 1), abs(got[2] / want[2] - 1), abs(got[1] - want[1]) / (np.linalg.norm(u) * np.linalg.norm(w)))
    print(case, {k: f"{v:.2e}" for k, v in errs.items()})
    cams = sorted({q[0] for q in P.pose_priors})
    assert br.camera_blocks_agree(Hd, H.toarray(), lay, cams)
    assert errs["grad"] < 1e-12 and errs["S"] < 1e-12 and errs["gred"] < 1e-10 and errs["H"] < 1e-12
    assert errs["mv_explicit"] < 1e-12 and errs["mv_implicit"] < 1e-12 and errs["norms"] < 1e-12 and errs["gram"] < 1e-12
    assert errs["step"] < 1e-10
    assert trial == pytest.approx(Q.cost(), rel=1e-9)   # the trial point carries the prior rows too
    s.close()


@pytest.mark.parametrize("kind", ["golden9", "crafted6"])
@pytest.mark.parametrize("variant", [SchurVariant.Iterative, SchurVariant.Implicit])
def test_step_of_the_pcg_variants(kind, variant):
    P = problem(kind, 65)
    r, J = P.jacobian()
    dx, g, _ = np_ref.direct_step(J, r, LAM)
    s = device(P, variant).with_cg_params(5000, 1e-13)
    step = s.solve_augmented_equation(LAM)
    print(kind, variant, rel(step, dx), s.info()["pcg_iterations"])
    assert rel(step, dx) < 1e-9 and rel(s.get_gradient(), g) < 1e-12
    s.close()


def test_matrix_free_only_handle():
    P = problem("crafted9", 65)
    r, J = P.jacobian()
    dx, g, _ = np_ref.direct_step(J, r, LAM)
    s = device(P, SchurVariant.Implicit, options={"matrix_free_only": 1}).with_cg_params(5000, 1e-13)
    assert rel(s.solve_augmented_equation(LAM), dx) < 1e-9
    s.close()


@pytest.mark.parametrize("kind", ["golden9", "crafted6"])
def test_jacobi_scaling_solves_the_scaled_augmented_system(kind):
    P = problem(kind, 65)
    s = device(P)
    scale = 1.0 / (1.0 + P.column_norms())
    s.apply_column_scaling(scale)
    r, J = P.jacobian()
    y, gs, _ = np_ref.direct_step((J @ sp.diags(scale)).tocsc(), r, 1e-3)
    # (in the scaled variables the columns have norm < 1 and lambda = 1e-3 is what the LM loop starts from: cond is modest)
    step = s.solve_augmented_equation(1e-3)
    touched = P.column_norms() > 0
    print(kind, rel(step[touched], y[touched]), rel(s.get_gradient(), gs))
    assert rel(s.get_gradient(), gs) < 1e-12 and rel(step[touched], y[touched]) < 1e-7
    s.close()


@pytest.mark.parametrize("kind", ["golden9", "crafted6"])
def test_camera_covariance_is_the_inverse_of_the_reference_s(kind):
    P = problem(kind, 65)
    s = device(P)
    s.solve_augmented_equation(LAM)
    cov = s.camera_covariance_blocks()
    r, J = P.jacobian()
    _, g, H = np_ref.direct_step(J, r, LAM)
    S, _ = np_ref.schur_dense(H, g, P.lay.cam_dof, LAM)
    Z = np.linalg.inv(S)
    worst = 0.0
    for c in range(P.d.n_cam):
        idx = np.concatenate([P.lay.pose_col[c] + np.arange(6), P.lay.intr_col[c] + np.arange(3)])
        worst = max(worst, rel(cov[c], Z[np.ix_(idx, idx)]))
    print(kind, worst)
    assert worst < 1e-10
    s.close()


def _bytes(s, lam=1e-3, iterations=3):
    step = s.solve_augmented_equation(lam)
    out = [step, s.get_gradient(), *s.get_schur()]
    s.lm_optimize(LevenbergMarquardtConfig(max_iterations=iterations, cost_tolerance=0.0, parameter_tolerance=0.0, gradient_tolerance=0.0))
    return out + list(s.get_parameters())


@pytest.mark.parametrize("kind", ["golden9", "crafted6"])
def test_bit_reproducible_and_independent_of_the_order_between_cameras(kind):
    P = problem(kind, 130)
    a, b = device(P), device(P)
    A, B = _bytes(a), _bytes(b)
    assert all(np.array_equal(x, y) for x, y in zip(A, B))
    # another order of the caller's list that keeps the order within every camera
    Q = br.PriorBaProblem(P.d, P.opt, P.loss, P.masks, P.params, P.pose_priors, P.intr_priors)
    order = np.argsort([(-q[0]) for q in P.pose_priors], kind="stable")
    Q.pose_priors = [P.pose_priors[k] for k in order]
    if Q.intr_priors:
        order = np.argsort([(q[0] * 7) % 5 for q in P.intr_priors], kind="stable")
        Q.intr_priors = [P.intr_priors[k] for k in order]
    c = device(Q)
    assert all(np.array_equal(x, y) for x, y in zip(A, _bytes(c)))
    for s in (a, b, c):
        s.close()


@pytest.mark.parametrize("kind", ["golden9", "crafted6"])
@pytest.mark.parametrize("variant", [SchurVariant.Sparse, SchurVariant.Implicit])
def test_clearing_restores_the_handle_that_never_had_priors(kind, variant):
    P = problem(kind, 65)
    plain, s = device(P, variant, priors=False), device(P, variant)
    with_priors = s.solve_augmented_equation(1e-3)
    s.set_priors([], [] if P.intr_priors else None)
    assert s.prior_residuals()[0].shape == (0, 7)
    a, b = s.solve_augmented_equation(1e-3), plain.solve_augmented_equation(1e-3)
    assert np.array_equal(a, b) and not np.array_equal(a, with_priors) and np.array_equal(s.get_gradient(), plain.get_gradient())
    if variant == SchurVariant.Sparse:
        assert all(np.array_equal(x, y) for x, y in zip(s.get_schur(), plain.get_schur()))
    assert s.compute_cost() == plain.compute_cost()
    s.set_priors(P.pose_priors, P.intr_priors or None)   # re-applicable
    assert np.array_equal(s.solve_augmented_equation(1e-3), with_priors)
    s.close(); plain.close()


def test_setting_priors_voids_the_step_the_dogleg_cache_and_the_factor():
    P = problem("golden9", 2)
    s = device(P, priors=False)
    s.solve_augmented_equation(LAM)
    s.camera_covariance_blocks()
    s.set_priors(P.pose_priors, P.intr_priors)
    assert kind_of(s.eval_step) == "InvalidState" and kind_of(s.commit_step) == "InvalidState"
    assert kind_of(s.camera_covariance_blocks) == "InvalidState" and kind_of(s.landmark_covariance_blocks) == "InvalidState"
    s.dogleg_step(1e-4, 1.0)
    s.eval_step()
    s.discard_step()
    s.set_priors(P.pose_priors[:1], None)
    assert kind_of(s.dogleg_step, 1e-4, 1.0, reuse=True) == "InvalidState"
    s.set_priors(P.pose_priors, None)
    r, J = P.jacobian()
    dx, g, _ = np_ref.direct_step(J, r, LAM)
    assert rel(s.solve_augmented_equation(LAM), dx) < 1e-10   # a new solve sees them
    s.close()


def test_refusals_leave_the_handle_as_it_was():
    P = problem("golden9", 3)
    L = capi.load()
    cam = np.array([0, 1], np.uint32); d7 = np.tile(br.pose_vector(P.d.poses)[0], (2, 1)); d3 = np.tile(P.d.intr[0], (2, 1))
    # before set_structure
    h = capi.Handle(P.d.n_cam, P.d.n_pt, P.d.n_obs, SELFCAL.value, 0)
    assert L.apexgpu_set_pose_priors(h.h, 2, capi.ptr(cam), capi.ptr(d7), None, None) == -6
    assert L.apexgpu_set_intrinsic_priors(h.h, 2, capi.ptr(cam), capi.ptr(d3), None, None) == -6
    del h
    s = device(P)
    h = s._need()
    before = s.solve_augmented_equation(LAM)
    res_before = s.prior_residuals()

    def refused(fn, n, c, data, dl=None, w=None, code=-5):
        rc = fn(h.h, n, capi.ptr(c), capi.ptr(data), capi.ptr(dl), capi.ptr(w))
        assert rc == code, (rc, L.apexgpu_last_error(h.h))
        assert len(L.apexgpu_last_error(h.h)) > 0

    bad_cam = np.array([0, P.d.n_cam], np.uint32)
    nan7 = d7.copy(); nan7[1, 4] = np.nan
    nan3 = d3.copy(); nan3[0, 2] = np.nan
    for fn, data, nan in ((L.apexgpu_set_pose_priors, d7, nan7), (L.apexgpu_set_intrinsic_priors, d3, nan3)):
        refused(fn, 2, bad_cam, data)
        refused(fn, 2, cam, nan)
        refused(fn, 2, cam, data, dl=np.array([1.0, np.nan]))
        for w in (np.nan, 0.0, -1.0, np.inf):
            refused(fn, 2, cam, data, w=np.array([1.0, w]))
    for a, b in zip(s.prior_residuals(), res_before):
        assert np.array_equal(a, b)
    assert np.array_equal(s.export_step()[0], before) and s.eval_step() > 0   # the pending step is still there
    s.close()
    # intrinsics priors on a six-column handle; pose priors are fine there
    Q = problem("golden6", 2)
    s6 = device(Q)
    h = s6._need()
    rc = L.apexgpu_set_intrinsic_priors(h.h, 2, capi.ptr(cam), capi.ptr(d3), None, None)
    assert rc == -5 and b"six columns" in L.apexgpu_last_error(h.h)
    assert L.apexgpu_set_intrinsic_priors(h.h, 0, None, None, None, None) == 0
    assert len(s6.prior_residuals()[0]) == 2
    s6.close()
    # a sharded handle
    sh = GpuSchurComplementSolver(0).with_shard(0, 2)
    sh.initialize_structure(bt.device_problem(P))
    h = sh._need()
    assert L.apexgpu_set_pose_priors(h.h, 2, capi.ptr(cam), capi.ptr(d7), None, None) == -6
    assert b"single-rank" in L.apexgpu_last_error(h.h)
    sh.close()
    # set_shard on a handle that holds priors
    s = device(P)
    h = s._need()
    assert L.apexgpu_set_shard(h.h, 0, 2) == -6 and b"priors" in L.apexgpu_last_error(h.h)
    assert len(s.prior_residuals()[0]) == 3
    s.close()


@pytest.mark.parametrize("kind,loss", [("golden9", "huber"), ("golden6", None), ("crafted9", "cauchy")])
def test_lm_history_against_the_numpy_loop(kind, loss):
    P = problem(kind, 65, loss=loss)
    s = device(P)
    start = P.cost()
    hist_ref = br.lm(P, 8)
    before = np.r_[start, hist_ref[:-1, 0]]
    assert (np.abs(before - hist_ref[:, 7]) > 1e-6 * before).all()   # every accept / reject decision away from its threshold
    res, hist, _ = s.lm_optimize(LevenbergMarquardtConfig(max_iterations=7, cost_tolerance=0.0, parameter_tolerance=0.0, gradient_tolerance=0.0))
    print(kind, "accepted", hist[:, 3], "costs", hist[:, 0])
    assert len(hist) == 8 and np.array_equal(hist[:, 3], hist_ref[:, 3])
    assert np.allclose(hist[:, 0], hist_ref[:, 0], rtol=1e-7, atol=0) and np.allclose(hist[:, 7], hist_ref[:, 7], rtol=1e-7, atol=0)
    s.close()


@pytest.mark.parametrize("kind,scaling", [("golden9", True), ("golden6", False)])
def test_dogleg_history_against_the_numpy_loop(kind, scaling):
    P = problem(kind, 65)
    mu = dict(initial_mu=1.0, min_mu=1e-2, max_mu=1e4) if not scaling else {}   # (pixels: tests/np_ref_ba_tr.py, MU)
    _, _, _, _, _, p_c = bt.first_linearisation(P, scaling, mu.get("initial_mu", 1e-4))
    P.scaling = None
    radius0 = 0.5 * float(np.linalg.norm(p_c))
    start = P.params
    ref = tr.dog_leg(P, trust_region_radius=radius0, use_jacobi_scaling=scaling, max_iterations=8, **mu)
    assert ref["margins"].min() > 1e-6
    P.params = start; P.scaling = None
    cfg = DogLegConfig(max_iterations=8, trust_region_radius=radius0, use_jacobi_scaling=scaling, **mu)
    out = DogLeg.with_config(cfg).optimize(P.device_problem(), initial_values=P.params)
    H, R = out.history, ref["history"]
    print(kind, out.status, out.iterations, "types", R[:, 9], "reused", R[:, 11])
    assert (out.status.value, out.iterations) == (ref["status"], ref["iterations"])
    assert np.array_equal(H[:, [4, 9, 11]], R[:, [4, 9, 11]]) and np.array_equal(H[:, 2], R[:, 2])
    np.testing.assert_allclose(H[:, 0], R[:, 0], rtol=1e-7)
    np.testing.assert_allclose(H[:, 1], R[:, 1], rtol=1e-7)


def test_from_plain_c(tmp_path):
    out = os.path.join(ROOT, "tests", "_build")
    os.makedirs(out, exist_ok=True)
    exe = os.path.join(out, "capi_prior_client")
    libdir = os.path.join(ROOT, "apex-solver_amd")
    subprocess.run(["gcc", "-O2", "-Wall", "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "capi_prior_client.c"), "-o", exe,
                    "-L", libdir, "-lapexgpu", "-lm", f"-Wl,-rpath,{libdir}", "-Wl,-rpath,/opt/rocm/lib"], check=True)
    P = problem("golden9", 5)
    d = P.d
    f = tmp_path / "ba_prior.bin"
    cp, xp, dp, wp = br._rows(P.pose_priors, 7)
    ci, xi, di, wi = br._rows(P.intr_priors, 3)
    with open(f, "wb") as fh:
        np.array([d.n_cam, d.n_pt, d.n_obs, len(cp), len(ci)], np.int64).tofile(fh)
        d.cam_idx.astype(np.uint32).tofile(fh); d.pt_idx.astype(np.uint32).tofile(fh)
        d.obs_uv.astype(np.float64).tofile(fh); d.poses.tofile(fh); d.intr.tofile(fh); d.points.tofile(fh)
        cp.astype(np.uint32).tofile(fh); xp.tofile(fh); dp.tofile(fh); wp.tofile(fh)
        ci.astype(np.uint32).tofile(fh); xi.tofile(fh); di.tofile(fh); wi.tofile(fh)
    p = subprocess.run([exe, str(f)], capture_output=True, text=True, timeout=120)
    assert p.returncode == 0, p.stderr
    got = json.loads(p.stdout.strip().splitlines()[-1])
    Q = br.PriorBaProblem(d, P.opt, None, fm.empty(d.n_cam, d.n_pt), P.params, P.pose_priors, P.intr_priors)   # (the client sets no loss, no mask)
    r, J = Q.jacobian()
    dx, _, _ = np_ref.direct_step(J, r, LAM)
    rp, ri = Q.prior_residuals()
    assert got["cost"] == pytest.approx(Q.cost(), rel=1e-12) and got["step_norm"] == pytest.approx(np.linalg.norm(dx), rel=1e-9)
    assert got["pose_r_norm"] == pytest.approx(np.linalg.norm(rp), rel=1e-12) and got["intr_r_norm"] == pytest.approx(np.linalg.norm(ri), rel=1e-12)
    assert got["cleared_cost"] < got["cost"] and got["bad_camera"] == -5
