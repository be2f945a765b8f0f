"""The edge-information per-edge math of pg_device.hpp / pg2_device.hpp, compiled for the host
(tests/host_harness_info.cpp), against the literal whitened and corrected blocks of tests/np_ref_info.py.  No GPU needed:
isolates formula errors -- a transposed cross block above all -- from kernel-structure errors.

Bounds: 1e-12 max(1, |J_w|^2) for blocks and Jacobian products (J_w = U J, the whitened uncorrected Jacobian of the edge),
1e-12 relative for g and the cost, both taken over the graph (the stacked gradient segments, the summed cost): an odometry
edge of these graphs has a residual of rounding size, whose own digits differ between two fp64 evaluations, so its g segment
has no relative accuracy edge by edge."""
import ctypes as C
import os
import subprocess
from types import SimpleNamespace

import numpy as np
import pytest

import info_graphs as ig
import loss_graphs as lg
import np_ref_info as ni
import np_ref_loss as nl
import np_ref_trust_region as tr
from apex_solver_amd import capi
from apex_solver_amd.pose_graph import PoseGraphProblem, create_loss_function

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_f = np.ctypeslib.ndpointer(dtype=np.float64, flags="C_CONTIGUOUS")
NAMES = ("none", "huber", "cauchy", "tukey", "andrews", "lp3")


@pytest.fixture(scope="module")
def hi():
    out = os.path.join(ROOT, "tests", "_build")
    os.makedirs(out, exist_ok=True)
    so = os.path.join(out, "libhost_harness_info.so")
    subprocess.run(["g++", "-O2", "-ffp-contract=off", "-std=c++17", "-shared", "-fPIC",
                    "-I", os.path.join(ROOT, "apex-solver_amd", "csrc"),
                    os.path.join(ROOT, "tests", "host_harness_info.cpp"), "-o", so], check=True)
    L = C.CDLL(so)
    head = [C.c_int, _f, _f, _f, C.c_int, C.c_double, C.c_double, _f]
    L.hi_edge.argtypes = head + [_f, _f]
    L.hi_blocks.argtypes = head + [C.c_int] + [_f] * 5
    L.hi_jv.argtypes = head + [_f] * 5
    L.hi_cost.argtypes = head + [_f]
    return L


def losses_for(rw):
    """the sweep's losses, their scales cut at quantiles of the WHITENED residual norms"""
    return {"none": SimpleNamespace(kind=capi.LOSS_NONE, p0=0.0, p1=0.0),
            "huber": create_loss_function("huber", float(lg.scale_between(rw, 0.6))),
            "cauchy": create_loss_function("cauchy"), "tukey": create_loss_function("tukey", lg.scale_between(rw, 0.8)),
            "andrews": create_loss_function("andrews"), "lp3": create_loss_function("lp", 3.0)}


@pytest.fixture(scope="module", params=["se3", "se2"])
def edge_sets(request):
    """both variants of the graph: the uncorrected linearisation, the information matrices, the whitened blocks -- once"""
    out = {}
    for jitter in (False, True):
        d = ig.graph(request.param, 40, jitter=jitter)
        r, J = lg.linearize(d)
        W = ig.information(d)
        rw, Jw = ni.whiten(r, J, W)
        out[jitter] = SimpleNamespace(d=d, r=r, J=J, W=W, rw=rw, Jw=Jw, man=1 if request.param == "se2" else 0, D=r.shape[1],
                                      losses=losses_for(rw))
    return out


def conditions(name, loss, rw):
    ss = lg.squared_norms(rw)
    assert nl.threshold_margin(loss, ss) > 1e-9
    arms = np.array([nl.corrector(loss, s)[3] for s in ss])
    rho1 = np.array([float(nl.evaluate(loss, s)[1]) for s in ss])
    if name in ("andrews", "lp3"):   # both arms of the corrector
        assert (arms == 1).sum() >= 10 and (arms == 2).sum() >= 10, (name, (arms == 1).sum(), (arms == 2).sum())
    if name == "tukey":              # rho' = 0 on some edges
        assert (rho1 == 0.0).sum() >= 1 and (rho1 > 0.0).sum() >= 1
    if name == "huber":
        assert (ss > loss.p0 ** 2).any() and (ss < loss.p0 ** 2).any()
    return arms, rho1


@pytest.mark.parametrize("name", NAMES)
def test_weighted_blocks_match_the_literal_whitened_jacobian(hi, edge_sets, name):
    E = edge_sets[lg.needs_jitter(name)]
    d, D, man = E.d, E.D, E.man
    loss = E.losses[name]
    arms, rho1 = conditions(name, loss, E.rw)
    rng = np.random.default_rng(3)
    worst = dict(r=0.0, J=0.0, H=0.0, cross=0.0, jv=0.0)
    g_got, g_want, c_got, c_want = [], [], 0.0, np.longdouble(0)
    assert d.e_from[-1] == d.e_to[-1]   # the self-loop
    for e in range(d.n_e):
        k0, k1, m = (np.ascontiguousarray(x, dtype=np.float64) for x in (d.poses[d.e_from[e]], d.poses[d.e_to[e]], d.meas[e]))
        W = np.ascontiguousarray(E.W[e])
        rt, Jt, arm, s = nl.correct(E.rw[e], E.Jw[e], loss)   # long double
        assert arm == arms[e]
        Jn = max(1.0, float(np.abs(E.Jw[e]).max()) ** 2)
        args = (man, k0, k1, m, loss.kind, loss.p0, loss.p1, W)
        r = np.zeros(D); J = np.zeros((D, 2 * D))
        assert hi.hi_edge(*args, r, J) == 0
        worst["r"] = max(worst["r"], float(np.abs(r - rt).max() / max(1.0, np.abs(rt).max())))
        worst["J"] = max(worst["J"], float(np.abs(J - Jt).max() / max(1.0, np.abs(Jt).max())))
        Ja, Jb = Jt[:, :D], Jt[:, D:]
        self_loop = d.e_from[e] == d.e_to[e]
        for order in ((2,) if self_loop else (0, 1)):   # every edge with from < to and with from > to
            Hff, Htt, Hx = np.zeros((D, D)), np.zeros((D, D)), np.zeros((D, D)); gf, gt = np.zeros(D), np.zeros(D)
            assert hi.hi_blocks(*args, order, Hff, Htt, Hx, gf, gt) == 0
            if order == 2:
                Js = Ja + Jb
                ref = [(Hff, Js.T @ Js), (Htt, 0 * Hff)]; xref = 0 * Hff; gref = [(gf, Js.T @ rt), (gt, 0 * gf)]
            else:
                ref = [(Hff, Ja.T @ Ja), (Htt, Jb.T @ Jb)]; gref = [(gf, Ja.T @ rt), (gt, Jb.T @ rt)]
                xref = Jb.T @ Ja if order == 0 else Ja.T @ Jb   # row vertex = the larger of (from, to)
            for got, want in ref:
                worst["H"] = max(worst["H"], float(np.abs(got - want).max()) / Jn)
            worst["cross"] = max(worst["cross"], float(np.abs(Hx - xref).max()) / Jn)
            if order != 2 and rho1[e] > 0:   # the transposed block is far away: the test can see the orientation
                assert float(np.abs(xref - xref.T).max()) > 1e-6 * float(np.abs(xref).max())
            for got, want in gref:
                g_got.append(got.copy()); g_want.append(want)
            if rho1[e] == 0.0:
                assert not Hff.any() and not Htt.any() and not Hx.any() and not gf.any() and not gt.any() and not J.any() and not r.any()
        ab = [x / np.linalg.norm(x) for x in (rng.standard_normal(2 * D), rng.standard_normal(2 * D))]
        a0, a1, b0, b1 = (np.ascontiguousarray(x) for x in (ab[0][:D], ab[0][D:], ab[1][:D], ab[1][D:]))
        o3 = np.zeros(3)
        assert hi.hi_jv(*args, a0, a1, b0, b1, o3) == 0
        u, w = Jt @ ab[0], Jt @ ab[1]
        worst["jv"] = max(worst["jv"], float(np.abs(o3 - np.array([u @ u, u @ w, w @ w], dtype=nl.LD)).max()) / Jn)
        c = np.zeros(1)
        assert hi.hi_cost(*args, c) == 0
        c_got += c[0]; c_want += rt @ rt
    g_got = np.concatenate(g_got); g_want = np.concatenate(g_want)
    g_err = float(np.linalg.norm(g_got - g_want) / np.linalg.norm(g_want))
    c_err = float(abs(c_got - c_want) / c_want)
    print(name, "se2" if man else "se3", "arms", (arms == 1).sum(), (arms == 2).sum(), "rho'=0:", (rho1 == 0).sum(), worst, "g", g_err, "cost", c_err)
    assert worst["r"] < 1e-12 and worst["J"] < 1e-12, worst
    assert worst["H"] < 1e-12 and worst["cross"] < 1e-12 and worst["jv"] < 1e-12, worst
    assert g_err < 1e-12 and c_err < 1e-12


@pytest.mark.parametrize("name", ["none", "cauchy", "lp3"])
@pytest.mark.parametrize("man", ["se3", "se2"])
def test_the_fixture_is_well_conditioned_for_the_step_bound(man, name):
    """The device tests hold the step at lambda = 1e-3 and 1e4 to 1e-10 of np_ref_trust_region.solve_damped.  That presumes
    numpy's own fp64 solve of the weighted system is an order better: within 1e-11 of the solve carried out in long double.
    Lp(3) is the worst conditioned of the sweep (its weights grow with the residual); info_graphs' sigma range was narrowed for it."""
    d = ig.graph(man, 120)
    r, J = lg.linearize(d)
    W = ig.information(d)
    rw, _ = ni.whiten(r, J, W)
    loss = losses_for(rw)[name]
    P = ni.numpy_problem(PoseGraphProblem.pose_graph(d, loss=None if name == "none" else loss, information=W))
    H, g = P.normal_equations()
    for lam in (1e-3, 1e4):
        x64 = tr.solve_damped(H, g, lam)
        xld = ni.solve_damped_ld(H, g, lam)
        err = float(np.linalg.norm(x64 - xld) / np.linalg.norm(xld))
        print(man, name, lam, "fp64 solve against the long-double solve", err)
        assert err < 1e-11


def test_standalone_harness_runs():
    """-DHI_MAIN: the same file as a program of its own (the form that is built with -fsanitize=address,undefined)"""
    out = os.path.join(ROOT, "tests", "_build")
    os.makedirs(out, exist_ok=True)
    exe = os.path.join(out, "host_harness_info")
    subprocess.run(["g++", "-O1", "-g", "-ffp-contract=off", "-std=c++17", "-DHI_MAIN", "-I", os.path.join(ROOT, "apex-solver_amd", "csrc"),
                    os.path.join(ROOT, "tests", "host_harness_info.cpp"), "-o", exe], check=True)
    p = subprocess.run([exe], capture_output=True, text=True)
    assert p.returncode == 0 and "host_harness_info:" in p.stdout, (p.returncode, p.stdout, p.stderr)
