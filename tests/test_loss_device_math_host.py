"""pg_loss.hpp and the general-loss per-edge math of pg_device.hpp / pg2_device.hpp, compiled for the host
(tests/host_harness_loss.cpp), against tests/np_ref_loss.py.  No GPU needed: isolates formula errors from kernel-structure
errors.  The bounds are those of tests/test_pg_device_math_host.py: 1e-13 relative (floor 1) for residual-like values,
1e-12 max(1, |J|^2) for products of Jacobians."""
import ctypes as C
import os
import subprocess
from types import SimpleNamespace

import numpy as np
import pytest

import loss_graphs as lg
import np_ref_loss as nl
from apex_solver_amd import capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_f = np.ctypeslib.ndpointer(dtype=np.float64, flags="C_CONTIGUOUS")
EPS = nl.EPS

# every kind at the reference front end's default parameters (Lp at p = 3: the one with rho'' > 0), Barron at alpha = 1, -2, 0, 2
KINDS = [("NONE", 0, 0), ("L2", 0, 0), ("L1", 0, 0), ("HUBER", 1.345, 0), ("CAUCHY", 2.3849, 0), ("FAIR", 1.3999, 0),
         ("GEMAN_MCCLURE", 1.0, 0), ("WELSCH", 2.9846, 0), ("TUKEY", 4.6851, 0), ("ANDREWS", 1.339, 0), ("RAMSAY", 0.3, 0),
         ("TRIMMED_MEAN", 2.0, 0), ("LP_NORM", 3.0, 0), ("LP_NORM", 1.5, 0), ("BARRON", 1.0, 1.0), ("BARRON", -2.0, 1.0),
         ("BARRON", 0.0, 1.0), ("BARRON", 2.0, 1.0), ("BARRON", 1.0 + 1e-7, 2.5), ("T_DISTRIBUTION", 5.0, 0)]


def mk(name, p0, p1):
    return SimpleNamespace(kind=capi.LOSS_KINDS.index(name), p0=float(p0), p1=float(p1))


@pytest.fixture(scope="module")
def hl():
    out = os.path.join(ROOT, "tests", "_build")
    os.makedirs(out, exist_ok=True)
    so = os.path.join(out, "libhost_harness_loss.so")
    subprocess.run(["g++", "-O2", "-ffp-contract=off", "-std=c++17", "-shared", "-fPIC",
                    "-I", os.path.join(ROOT, "apex-solver_amd", "csrc"),
                    os.path.join(ROOT, "tests", "host_harness_loss.cpp"), "-o", so], check=True)
    L = C.CDLL(so)
    L.hl_loss.argtypes = [C.c_int, C.c_double, C.c_double, C.c_double, _f]
    L.hl_corrector.argtypes = [_f, C.c_double, _f]
    L.hl_corrector.restype = None
    L.hl_edge.argtypes = [C.c_int, _f, _f, _f, C.c_int, C.c_double, C.c_double, _f, _f]
    L.hl_blocks.argtypes = [C.c_int, _f, _f, _f, C.c_int, C.c_double, C.c_double, C.c_int] + [_f] * 5
    L.hl_jv.argtypes = [C.c_int, _f, _f, _f, C.c_int, C.c_double, C.c_double] + [_f] * 6
    return L


def s_grid(loss):
    g = [0.0, 1e-300, 1e-20, EPS * 0.5, EPS * (1 - 1e-9), EPS, EPS * (1 + 1e-9), EPS * 2]
    for t in nl.thresholds(loss):
        # Both sides, 1e-4 (relative) away.  AT a threshold rho'' is a rounding residue of either sign and the arm is not
        # defined.  Closer than ~1e-5 to Andrews' cut at (pi c)^2 no fp64 evaluation can meet 1e-13: sqrt(rho') there is
        # sqrt(0.5 sin(x / c)) with x / c one rounding (3.5e-16) away from its value, which moves it by
        # 0.25 * 3.5e-16 / sqrt(rho') -- 3e-12 at a distance of 1e-9, 1e-14 at 1e-4.
        g += [t * (1 - 1e-4), t * (1 + 1e-4)]
    g += [m * 10.0 ** e for e in range(-12, 7) for m in (1.0, 3.7)]
    return g


@pytest.mark.parametrize("kind", KINDS, ids=lambda k: f"{k[0]}-{k[1]}")
def test_loss_and_corrector_match_the_reference_on_the_grid(hl, kind):
    loss = mk(*kind)
    worst = 0.0
    for s in s_grid(loss):
        out = np.zeros(6)
        assert hl.hl_loss(loss.kind, loss.p0, loss.p1, s, out) == 0
        ref = nl.six(loss, s)
        err = np.abs(out.astype(nl.LD) - ref) / np.maximum(1.0, np.abs(ref))
        assert np.all(np.isfinite(out)), (kind, s, out)
        worst = max(worst, float(err.max()))
        assert err.max() < 1e-13, (kind, s, out, ref)
    print(kind, "worst", worst)


def test_constructor_refusals(hl):
    out = np.zeros(6)
    for name in ("HUBER", "CAUCHY", "FAIR", "GEMAN_MCCLURE", "WELSCH", "TUKEY", "ANDREWS", "RAMSAY", "TRIMMED_MEAN", "LP_NORM", "T_DISTRIBUTION"):
        for bad in (0.0, -1.0, float("nan")):
            assert hl.hl_loss(capi.LOSS_KINDS.index(name), bad, 1.0, 1.0, out) == -1
    assert hl.hl_loss(capi.LOSS_BARRON, -7.5, 0.0, 1.0, out) == -1 and hl.hl_loss(capi.LOSS_BARRON, -7.5, 1.0, 1.0, out) == 0
    assert hl.hl_loss(15, 1.0, 1.0, 1.0, out) == -1 and hl.hl_loss(-1, 1.0, 1.0, 1.0, out) == -1


def test_corrector_on_the_reference_edge_case_triples(hl):
    """corrector.rs:411-457: the two tests that feed Corrector::new a fixed (rho, rho', rho'') -- a negative rho' (sqrt_rho1 is
    NaN, d clamps to 0 and alpha to 1) and a small positive rho' with positive rho'' (nothing is NaN) -- on pg_corrector and
    on np_ref_loss.corrector_of."""
    out = np.zeros(3)
    hl.hl_corrector(np.array([0.5, -0.1, 0.5]), 100.0, out)             # test_corrector_no_nan_on_negative_d
    ref = nl.corrector_of([0.5, -0.1, 0.5], 100.0)
    assert np.isnan(out[0]) and np.isnan(float(ref[0]))                  # sqrt of a negative rho'
    assert ref[3] == 2 and out[2] == 1.0 / 100.0 == float(ref[2])        # d = max(1 - 1000, 0) = 0, alpha = 1: alpha / s, not NaN
    hl.hl_corrector(np.array([0.5, 0.001, 0.001]), 10.0, out)           # test_corrector_positive_rho1_large_rho2_ratio
    ref = nl.corrector_of([0.5, 0.001, 0.001], 10.0)
    assert not np.isnan(out).any() and ref[3] == 2
    want = np.array([float(x) for x in ref[:3]])
    assert np.all(np.abs(out - want) <= 1e-13 * np.maximum(1.0, np.abs(want))), (out, want)
    alpha = 1.0 - np.sqrt(1.0 + 2.0 * 10.0 * 0.001 / 0.001)
    assert out[2] == pytest.approx(alpha / 10.0, rel=1e-15) and out[1] == pytest.approx(np.sqrt(0.001) / (1.0 - alpha), rel=1e-15)


# ---- per-edge blocks and products on graph edges -----------------------------------------------------------------------
@pytest.fixture(scope="module", params=["se3", "se2"])
def edge_sets(request):
    """the uncorrected linearisation of both variants of the graph, once"""
    out = {}
    for jitter in (False, True):
        d = lg.graph(request.param, 40, jitter=jitter)
        r, J = lg.linearize(d)
        out[jitter] = SimpleNamespace(d=d, r=r, J=J, man=1 if request.param == "se2" else 0, D=r.shape[1], losses=lg.sweep_losses(r))
    return out


@pytest.mark.parametrize("name", lg.SWEEP)
def test_blocks_and_jv_match_the_literal_corrected_jacobian(hl, edge_sets, name):
    edges = edge_sets[lg.needs_jitter(name)]
    d, D, man = edges.d, edges.D, edges.man
    loss = edges.losses[name]
    arms, rho1 = lg.check_conditions(name, loss, edges.r)
    rng = np.random.default_rng(3)
    worst = dict(r=0.0, J=0.0, H=0.0, g=0.0, jv=0.0)
    assert d.e_from[-1] == d.e_to[-1]   # the self-loop
    for e in range(d.n_e):
        k0, k1, m = (np.ascontiguousarray(x, dtype=np.float64) for x in (d.poses[d.e_from[e]], d.poses[d.e_to[e]], d.meas[e]))
        self_loop = int(d.e_from[e] == d.e_to[e])
        rt, Jt, arm, s = nl.correct(edges.r[e], edges.J[e], loss)
        assert arm == arms[e]
        Jn = max(1.0, float(np.abs(edges.J[e]).max()) ** 2)
        # export: the literal J~
        r = np.zeros(D); J = np.zeros((D, 2 * D))
        assert hl.hl_edge(man, k0, k1, m, loss.kind, loss.p0, loss.p1, r, J) == 0
        worst["r"] = max(worst["r"], float(np.abs(r - rt).max() / max(1.0, np.abs(rt).max())))
        worst["J"] = max(worst["J"], float(np.abs(J - Jt).max() / max(1.0, np.abs(Jt).max())))
        # blocks
        Haa, Hbb, Hba = np.zeros((D, D)), np.zeros((D, D)), np.zeros((D, D)); ga, gb = np.zeros(D), np.zeros(D)
        assert hl.hl_blocks(man, k0, k1, m, loss.kind, loss.p0, loss.p1, self_loop, Haa, Hbb, Hba, ga, gb) == 0
        Ja, Jb = Jt[:, :D], Jt[:, D:]
        if self_loop:
            Js = Ja + Jb
            ref = [(Haa, Js.T @ Js), (Hbb, 0 * Haa), (Hba, 0 * Haa)]; gref = [(ga, Js.T @ rt), (gb, 0 * ga)]
        else:
            ref = [(Haa, Ja.T @ Ja), (Hbb, Jb.T @ Jb), (Hba, Jb.T @ Ja)]; gref = [(ga, Ja.T @ rt), (gb, Jb.T @ rt)]
        for got, want in ref:
            worst["H"] = max(worst["H"], float(np.abs(got - want).max()) / Jn)
        for got, want in gref:
            worst["g"] = max(worst["g"], float(np.abs(got - want).max()) / Jn)
        if rho1[e] == 0.0:
            assert not Haa.any() and not Hbb.any() and not Hba.any() and not ga.any() and not gb.any() and not J.any() and not r.any()
        # edge_jv
        a0, a1, b0, b1 = (np.ascontiguousarray(rng.standard_normal(D)) for _ in range(4))
        u = np.zeros(D); w = np.zeros(D)
        assert hl.hl_jv(man, k0, k1, m, loss.kind, loss.p0, loss.p1, a0, a1, b0, b1, u, w) == 0
        worst["jv"] = max(worst["jv"], float(max(np.abs(u - Jt @ np.concatenate([a0, a1])).max(), np.abs(w - Jt @ np.concatenate([b0, b1])).max())) / Jn)
    print(name, "se2" if man else "se3", "arms", (arms == 1).sum(), (arms == 2).sum(), "rho'=0:", (rho1 == 0).sum(), worst)
    if lg.needs_jitter(name):
        # H and g also on the graph as the generators give it, odometry edges of rounding size included: quadratic in J~, they
        # carry rho' ~ 1e-17 there and do not see the noise that J~ itself and J~ x (linear in J~: 1e-8 of |J|^2) show
        plain = edge_sets[False]
        d = plain.d
        tiny = 0
        for e in range(d.n_e):
            k0, k1, m = (np.ascontiguousarray(x, dtype=np.float64) for x in (d.poses[d.e_from[e]], d.poses[d.e_to[e]], d.meas[e]))
            self_loop = int(d.e_from[e] == d.e_to[e])
            rt, Jt, _, s = nl.correct(plain.r[e], plain.J[e], loss)
            tiny += s < EPS
            Jn = max(1.0, float(np.abs(plain.J[e]).max()) ** 2)
            Haa, Hbb, Hba = np.zeros((D, D)), np.zeros((D, D)), np.zeros((D, D)); ga, gb = np.zeros(D), np.zeros(D)
            assert hl.hl_blocks(man, k0, k1, m, loss.kind, loss.p0, loss.p1, self_loop, Haa, Hbb, Hba, ga, gb) == 0
            Ja, Jb = Jt[:, :D], Jt[:, D:]
            if self_loop:
                Ja, Jb = Ja + Jb, 0 * Jb
            for got, want in ((Haa, Ja.T @ Ja), (Hbb, Jb.T @ Jb), (Hba, Jb.T @ Ja), (ga, Ja.T @ rt), (gb, Jb.T @ rt)):
                assert float(np.abs(got - want).max()) < 1e-12 * Jn, (e, s)
        assert tiny >= 10
    assert worst["r"] < 1e-13 and worst["J"] < 1e-12, worst
    assert worst["H"] < 1e-12 and worst["g"] < 1e-12 and worst["jv"] < 1e-12, worst
