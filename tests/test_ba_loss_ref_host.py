"""The numpy reference of bundle adjustment under the loss family (tests/np_ref_ba_loss.py), the first-arm property of the
losses BA accepts (apexgpu_loss_evaluate, pg_loss_first_arm_only) and the general-loss per-observation math of ba_device.hpp
compiled for the host (tests/host_harness_ba_loss.cpp).  No GPU needed."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import ba_loss_cases as bc
import np_ref
import np_ref_ba_loss as nb
import np_ref_loss as nl
from apex_solver_amd import capi
from apex_solver_amd.loss import Loss, create_loss_function

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_f = np.ctypeslib.ndpointer(dtype=np.float64, flags="C_CONTIGUOUS")
K = {n: i for i, n in enumerate(capi.LOSS_KINDS)}

# (kind, p0, p1): every kind, several parameters each; Barron on both sides of its special cases and of alpha = 2
ACCEPTED = ([(K["NONE"], 0, 0), (K["L2"], 0, 0), (K["L1"], 0, 0)]
            + [(K[k], c, 0) for k in ("HUBER", "CAUCHY", "FAIR", "GEMAN_MCCLURE", "WELSCH", "TUKEY", "RAMSAY", "TRIMMED_MEAN")
               for c in (0.05, 1.345, 30.0)]
            + [(K["LP_NORM"], p, 0) for p in (0.5, 1.0, 1.5, 2.0)]
            + [(K["BARRON"], a, c) for a in (-1e3, -2.0, -1e-7, 0.0, 1e-7, 1.0, 2.0 - 1e-5, 2.0 - 1e-7, 2.0, 2.0 + 9e-7) for c in (0.3, 4.0)]
            + [(K["T_DISTRIBUTION"], nu, 0) for nu in (0.5, 5.0, 200.0)])
REFUSED = ([(K["ANDREWS"], c, 0) for c in (1e-3, 1.339, 1e4)] + [(K["LP_NORM"], p, 0) for p in (2.0 + 1e-9, 3.0, 8.0)]
           + [(K["BARRON"], a, c) for a in (2.0 + 1e-6, 2.0 + 2e-6, 3.0, 50.0) for c in (0.3, 4.0)])
S_GRID = np.concatenate([[0.0], np.logspace(-20, 12, 129)])


@pytest.fixture(scope="module")
def hb():
    out = os.path.join(ROOT, "tests", "_build")
    os.makedirs(out, exist_ok=True)
    so = os.path.join(out, "libhost_harness_ba_loss.so")
    subprocess.run(["g++", "-O2", "-ffp-contract=off", "-std=c++17", "-shared", "-fPIC", "-I", os.path.join(ROOT, "apex-solver_amd", "csrc"),
                    os.path.join(ROOT, "tests", "host_harness_ba_loss.cpp"), "-o", so], check=True)
    L = C.CDLL(so)
    L.hb_first_arm_only.argtypes = [C.c_int, C.c_double, C.c_double]
    L.hb_linearize_obs.argtypes = [C.c_int, _f, _f, _f, _f, C.c_int, C.c_double, C.c_double, _f, _f, _f, _f]
    L.hb_residual_obs.argtypes = [_f, _f, _f, _f, C.c_int, C.c_double, C.c_double, _f]
    return L


@pytest.fixture(scope="module")
def data():
    return bc.problem()


@pytest.mark.parametrize("delta", [0.5, 1.0, 7.0])
def test_huber_through_the_loss_family_is_the_huber_delta_reference(data, delta):
    d = data
    ci, pi = d.cam_idx.astype(int), d.pt_idx.astype(int)
    r, _, w, _ = np_ref.residuals(d.poses, d.intr, d.points, ci, pi, d.obs_uv, delta)
    rt, Jp, Jl, Ji, s, wl = nb.linearize(d.poses, d.intr, d.points, ci, pi, d.obs_uv, Loss(capi.LOSS_HUBER, delta))
    assert (w < 1).sum() > 10 and (w == 1).sum() > 10
    assert np.max(np.abs(w - wl)) <= 1e-15
    assert np.max(np.abs(r - rt)) <= 1e-15 * np.max(np.abs(r))
    _, _, Jp0, Jl0, Ji0 = np_ref.jacobian_blocks(d.poses, d.intr, d.points, ci, pi, d.obs_uv, delta)
    for a, b in ((Jp, Jp0), (Jl, Jl0), (Ji, Ji0)):
        assert np.max(np.abs(a - b)) <= 1e-15 * np.max(np.abs(b))


@pytest.mark.parametrize("kind,p0,p1", ACCEPTED)
def test_accepted_losses_keep_to_the_first_arm(hb, kind, p0, p1):
    assert hb.hb_first_arm_only(kind, p0, p1) == 1
    loss = Loss(kind, float(p0), float(p1))
    for s in S_GRID:
        o = loss.evaluate(s)   # apexgpu_loss_evaluate: rho, rho', rho'', sqrt_rho1, residual_scaling, alpha_sq_norm
        assert o[5] == 0.0 and o[4] == o[3], (s, o)
        assert not o[2] > 0.0


@pytest.mark.parametrize("kind,p0,p1", REFUSED)
def test_refused_losses_reach_the_second_arm(hb, kind, p0, p1):
    """pins pg_loss_first_arm_only to pg_loss_evaluate: what it refuses has rho'' > 0 somewhere on the grid"""
    assert hb.hb_first_arm_only(kind, p0, p1) == 0
    loss = Loss(kind, float(p0), float(p1))
    assert any(loss.evaluate(s)[2] > 0.0 for s in S_GRID)


def test_what_the_constructors_refuse_is_not_asked():
    L = capi.load()
    o = (C.c_double * 6)()
    for kind, p0, p1 in ((K["CAUCHY"], 0.0, 0), (K["BARRON"], 1.0, -1.0), (99, 1.0, 1.0), (K["TUKEY"], float("nan"), 0)):
        assert L.apexgpu_loss_evaluate(kind, p0, p1, 1.0, C.byref(o)) == -5


@pytest.mark.parametrize("name", bc.SWEEP)
def test_the_sweep_problem_meets_its_conditions(data, name):
    loss = bc.sweep_losses(bc.raw_residuals(data))[name]
    s, rho1 = bc.check_conditions(name, loss, data)
    assert (s < nl.EPS).sum() >= 4 and (np.sqrt(s) > 15).sum() >= len(s) // 6


@pytest.mark.parametrize("dc", [9, 6])
@pytest.mark.parametrize("name", ["cauchy", "tukey", "l1", "barron1", "trimmed", "lp"])
def test_general_per_observation_math_on_the_host(hb, data, name, dc):
    """linearize_obs / residual_obs with a PgLoss, on the CPU, against the numpy reference; the record's weight is sqrt(rho')
    and a cut observation is zero everywhere.  Bound per observation: 1e-13 of the largest entry of each block kind, plus what
    the raw residual's own rounding does to the weight.  u - u_obs cancels numbers of size U = max |u_obs|, so two evaluations
    of it differ by about dr = 2 eps U; sqrt(rho') is a function of s = |r|^2 with |d log w / d log s| <= 1/2 for every loss
    of this list away from its thresholds, i.e. a relative dr / |r| in the weight -- and in everything it multiplies."""
    d = data
    loss = bc.sweep_losses(bc.raw_residuals(d))[name]
    ci, pi = d.cam_idx.astype(int), d.pt_idx.astype(int)
    rt, Jp, Jl, Ji, s, w = nb.linearize(d.poses, d.intr, d.points, ci, pi, d.obs_uv, loss)
    idx = np.concatenate([np.arange(0, d.n_obs, 7), np.flatnonzero(w == 0)[:20], np.flatnonzero(s < nl.EPS)])
    sr, sp, sl, si = (np.max(np.abs(x)) for x in (rt, Jp, Jl, Ji))
    dr = 2 * nl.EPS * np.max(np.abs(d.obs_uv))
    for i in idx:
        r = np.zeros(2); jc = np.zeros(2 * dc); jl = np.zeros(6); rec = np.zeros(4); r2 = np.zeros(2)
        args = [np.ascontiguousarray(x, dtype=np.float64) for x in (d.poses[ci[i]], d.intr[ci[i]], d.points[pi[i]], d.obs_uv[i])]
        assert hb.hb_linearize_obs(dc, *args, loss.kind, loss.p0, loss.p1, r, jc, jl, rec) == 1
        assert hb.hb_residual_obs(*args, loss.kind, loss.p0, loss.p1, r2) == 1
        jc = jc.reshape(2, dc)
        assert np.array_equal(r, r2)
        tol = 1e-13 + (dr / np.sqrt(s[i]) if s[i] >= nl.EPS else 0.0)   # (below EPSILON the weight is 1 exactly)
        assert np.max(np.abs(r - rt[i])) <= tol * sr and np.max(np.abs(jl.reshape(2, 3) - Jl[i])) <= tol * sl
        assert np.max(np.abs(jc[:, :6] - Jp[i])) <= tol * sp
        if dc == 9:
            assert np.max(np.abs(jc[:, 6:] - Ji[i])) <= tol * si
        assert abs(rec[3] - w[i]) <= tol * max(1.0, w[i])
        if w[i] == 0.0:
            assert rec[3] == 0.0 and not r.any() and not jc.any() and not jl.any()
