"""tr_loop.cpp (Gauss-Newton, Dog-Leg) and dogleg_combine.hpp as a host program (tests/host_harness_tr.cpp, g++, no GPU) against
the numpy loops of tests/np_ref_trust_region.py, on the reference's Rosenbrock factor pair (dog_leg.rs:1426-1485).

Bounds.  The combine is a dozen fp64 operations on the same seven inputs in both languages: 1e-14 relative.  The histories run
the same arithmetic on a 2 x 2 system (cond <= 1e5 along these paths); costs and radii are held to 1e-9 relative, flags and
step types exactly.

The d^2 < 0 guard of compute_dog_leg_step has no case: no real input reaches it.  In the dog-leg branch c = |p_c|^2 - Delta^2 < 0
and |h|^2 > Delta^2; for a >= 0, d^2 = b^2 - a c >= 0 at once, and for a < 0, -a c > -a (|p_c|^2 - |h|^2), which gives
d^2 > (p_c.h - |h|^2)^2 >= 0 (with p_c.h and the norms any reals, consistent or not).  The branch is restated all the same."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

import apex_solver_amd as pkg
import np_ref_trust_region as tr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "apex-solver_amd", "csrc")
SRCS = [os.path.join(ROOT, "tests", "host_harness_tr.cpp"), os.path.join(CSRC, "tr_loop.cpp"), os.path.join(CSRC, "lm_loop.cpp")]


def build(tmp, name, flags):
    exe = str(tmp / name)
    cc = subprocess.run(["g++", "-std=c++17", "-ffp-contract=off", *flags, "-I", CSRC, *SRCS, "-o", exe], capture_output=True, text=True)
    assert cc.returncode == 0, cc.stderr[-4000:]
    return exe


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    return build(tmp_path_factory.mktemp("tr"), "host_harness_tr", ["-O2"])


def run(exe, *args):
    p = subprocess.run([exe, *[repr(float(a)) if isinstance(a, float) else str(a) for a in args]], capture_output=True, text=True, timeout=60)
    assert p.returncode == 0, (p.stdout[-2000:], p.stderr[-2000:])
    rows = [ln.split() for ln in p.stdout.strip().splitlines()]
    return rows, p.stderr


def assert_costs_close(got, want):
    """Costs as residual norms |r| = sqrt(2 cost): 1e-9 relative, and 1e-13 absolute -- at the minimum r is what rounding leaves
    of 10 (x2 - x1^2) and 1 - x1 at x = (1, 1): a few ulp of x times |J| ~ 20."""
    np.testing.assert_allclose(np.sqrt(2.0 * got), np.sqrt(2.0 * want), rtol=1e-9, atol=1e-13)


def vectors(kind):
    """(H, g, h, delta, expected type) hitting one branch of compute_dog_leg_step each"""
    rng = np.random.default_rng(11)
    A = rng.normal(size=(9, 6)); H = A.T @ A
    g = rng.normal(size=6)
    h = np.linalg.solve(H + 1e-4 * np.eye(6), -g)
    alpha, p_c = tr.cauchy_point(H, g)
    hn, pn = np.linalg.norm(h), np.linalg.norm(p_c)
    assert pn < hn
    if kind == "gauss-newton": return H, g, h, 2.0 * hn, tr.GAUSS_NEWTON
    if kind == "steepest-descent": return H, g, h, 0.5 * pn, tr.STEEPEST_DESCENT
    if kind == "dogleg-b-negative": return H, g, h, 0.5 * (pn + hn), tr.DOG_LEG   # b = p_c.(h - p_c) <= 0 needs an h behind p_c: below
    raise KeyError(kind)


COMBINE_CASES = {
    # name: (gg, hh, gh, uu, uw, ww, delta), expected type, what it is there for
    "gauss-newton": None, "steepest-descent": None, "dogleg-b-positive": None,
    # p_c = -alpha g with alpha = 1 (gg = uu); h chosen so that b = -alpha gh - alpha^2 gg <= 0: gh = -gg exactly gives b = 0
    "dogleg-b-zero": ((4.0, 25.0, -4.0, 4.0, -4.0, 30.0, 3.0), tr.DOG_LEG),
    "dogleg-b-negative": ((4.0, 25.0, 1.0, 4.0, 1.0, 30.0, 3.0), tr.DOG_LEG),     # g.h > 0: h points uphill, b = -1 - 4 < 0 ... see below
    # |a| < 1e-15: h = p_c up to an ulp, with |p_c| < delta < |h| by one ulp each side of 1
    "a-tiny": ((float(np.nextafter(1.0, 0.0)), float(np.nextafter(np.nextafter(1.0, 2.0), 2.0)), -1.0, float(np.nextafter(1.0, 0.0)), -1.0, 1.0, 1.0), tr.DOG_LEG),
    # |g.Hg| <= 1e-15: alpha = 1
    "flat-gradient": ((1e-4, 9.0, -1e-3, 1e-16, 0.0, 2.0, 1.0), tr.DOG_LEG),
}


def combine_inputs(name):
    if COMBINE_CASES[name] is not None:
        return COMBINE_CASES[name]
    kind = {"dogleg-b-positive": "dogleg-b-negative"}.get(name, name)   # (vectors(): the generic dog leg; its b is positive)
    H, g, h, delta, typ = vectors(kind)
    return tuple(tr.sums_of(H, g, h)) + (delta,), typ


@pytest.mark.parametrize("name", sorted(COMBINE_CASES))
def test_combine_matches_numpy(exe, name):
    args, typ = combine_inputs(name)
    ref = tr.combine(*args)
    assert ref["type"] == typ
    gg, hh, gh, uu, uw, ww, delta = args
    alpha = ref["alpha"]
    b = -alpha * gh - alpha * alpha * gg
    a = hh + 2 * alpha * gh + alpha * alpha * gg
    d2 = b * b - a * (alpha * alpha * gg - delta * delta)
    if name == "dogleg-b-positive": assert b > 0 and d2 >= 0 and abs(a) >= 1e-15
    if name in ("dogleg-b-zero", "dogleg-b-negative"): assert b <= 0 and d2 >= 0 and abs(a) >= 1e-15
    if name == "a-tiny": assert d2 >= 0 and abs(a) < 1e-15 and ref["beta"] == 1.0
    if name == "flat-gradient": assert abs(uu) <= 1e-15 and alpha == 1.0
    rows, _ = run(exe, "combine", *[float(v) for v in args])
    got = [float(v) for v in rows[0][:6]]
    assert int(rows[0][6]) == typ
    for k, key in enumerate(("alpha", "beta", "c_g", "c_h", "step_norm", "predicted_reduction")):
        print(name, key, got[k], ref[key])
        assert got[k] == pytest.approx(ref[key], rel=1e-14, abs=0.0 if ref[key] != 0.0 else 1e-300)


@pytest.mark.parametrize("kind", ["gauss-newton", "steepest-descent", "dogleg-b-negative"])
def test_numpy_combine_agrees_with_the_vector_form(kind):
    """The scalar restatement against the reference's own vector statements (no cancellation in these cases: 1e-12)."""
    H, g, h, delta, typ = vectors(kind)
    _, p_c = tr.cauchy_point(H, g)
    step, t, beta = tr.dog_leg_step(-g, p_c, h, delta)
    c = tr.combine(*tr.sums_of(H, g, h), delta)
    assert t == typ == c["type"]
    assert c["beta"] == pytest.approx(beta, rel=1e-12)
    assert np.linalg.norm(-c["c_g"] * g + c["c_h"] * h - step) <= 1e-12 * np.linalg.norm(step)
    assert c["predicted_reduction"] == pytest.approx(tr.predicted_reduction(step, g, H), rel=1e-12)
    assert c["step_norm"] == pytest.approx(np.linalg.norm(step), rel=1e-12)


@pytest.mark.parametrize("scaling", [0, 1], ids=["plain", "jacobi-scaling"])
@pytest.mark.parametrize("radius", [1e4, 0.05], ids=["wide", "narrow"])
def test_dogleg_history_matches_the_numpy_loop(exe, radius, scaling):
    ref = tr.dog_leg(tr.Rosenbrock(), max_iterations=60, trust_region_radius=radius, use_jacobi_scaling=bool(scaling))
    rows, _ = run(exe, "dl", -1.2, 1.0, radius, 1e-4, scaling, 1, 60)
    status, iters = int(rows[0][0]), int(rows[0][1])
    H = np.array(rows[1:], dtype=np.float64).reshape(-1, 12)
    R = ref["history"]
    print(status, iters, ref["status"], ref["iterations"], "types", sorted(set(R[:, 9])), "reused", int(R[:, 11].sum()), "rejected", int((R[:, 4] == 0).sum()))
    assert (status, iters) == (ref["status"], ref["iterations"]) and int(rows[0][4]) == iters   # jacobian_evaluations counts iterations
    assert ref["margins"].min() > 1e-6   # no decision of the reference run sits on its threshold
    assert np.array_equal(H[:, [4, 9, 11]], R[:, [4, 9, 11]])   # accepted, type, reused
    assert_costs_close(H[:, 0], R[:, 0])
    np.testing.assert_allclose(H[:, 1], R[:, 1], rtol=1e-9)
    assert np.array_equal(H[:, 2], R[:, 2])   # mu: powers of the factors, exactly
    np.testing.assert_allclose(H[:, 7], R[:, 7], rtol=1e-7, atol=1e-13 * np.sqrt(2.0 * ref["initial_cost"]))   # (-s.g - s.Hs / 2 cancels at the minimum)
    assert float(rows[0][2]) == pytest.approx(ref["radius"], rel=1e-9) and float(rows[0][3]) == ref["mu"]
    assert ref["status"] == 1 or ref["final_cost"] < 1e-10 * ref["initial_cost"]   # (converged runs reach the minimum)


def test_narrow_start_shows_every_branch_of_the_loop():
    """What the history test above relies on, stated on the numpy loop alone: the narrow start walks through all three step
    types, a rejection followed by a reused step and a good-step growth of the radius."""
    R = tr.dog_leg(tr.Rosenbrock(), max_iterations=60, trust_region_radius=0.05, use_jacobi_scaling=False)["history"]
    assert set(R[:, 9]) == {0.0, 1.0, 2.0}
    rej = np.nonzero(R[:-1, 4] == 0)[0]
    assert rej.size and (R[rej + 1, 11] == 1).any()
    assert (np.diff(R[:, 1]) > 0).any()


@pytest.mark.parametrize("scaling", [0, 1], ids=["plain", "jacobi-scaling"])
def test_gauss_newton_history_matches_the_numpy_loop(exe, scaling):
    ref = tr.gauss_newton(tr.Rosenbrock(), max_iterations=30, use_jacobi_scaling=bool(scaling))
    rows, _ = run(exe, "gn", -1.2, 1.0, scaling, 30)
    H = np.array(rows[1:], dtype=np.float64).reshape(-1, 8)
    R = ref["history"]
    assert (int(rows[0][0]), int(rows[0][1])) == (ref["status"], ref["iterations"])
    assert_costs_close(H[:, 0], R[:, 0])
    np.testing.assert_allclose(H[:, [4, 5]], R[:, [4, 5]], rtol=1e-7, atol=1e-12)   # (at the minimum g and the step are rounding residue: a few ulp of x times |J|^2 ~ 400)
    assert (H[:, 3] == 1).all() and (H[:, 1] == 0).all()


def test_lm_loop_still_converges_through_the_shared_convergence_check(exe):
    rows, _ = run(exe, "lm", -1.2, 1.0, 0, 100)
    H = np.array(rows[1:], dtype=np.float64).reshape(-1, 8)
    assert int(rows[0][0]) in (2, 3, 4) and H[-1, 0] < 1e-12


def test_harness_is_clean_under_asan_and_ubsan(tmp_path):
    if shutil.which("g++") is None:
        pytest.skip("no g++ on this machine")
    exe = build(tmp_path, "host_harness_tr_san", ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"])
    for args in (("dl", -1.2, 1.0, 0.05, 1e-4, 1, 1, 60), ("dl", -1.2, 1.0, 1e4, 1e-4, 0, 0, 60), ("gn", -1.2, 1.0, 0, 30),
                 ("lm", -1.2, 1.0, 1, 50), ("combine", 4.0, 25.0, -4.0, 4.0, -4.0, 30.0, 3.0)):
        _, err = run(exe, *args)
        assert "runtime error" not in err and "AddressSanitizer" not in err, err[-3000:]


def test_struct_layouts_of_the_new_c_structs():
    # apexgpu_gn_config: int (+pad) + 5 doubles + 2 ints; apexgpu_dl_config: int (+pad) + 15 doubles + 3 ints (+pad); apexgpu_dl_iter: 12 doubles
    assert C.sizeof(pkg.capi.GnConfigC) == 8 + 5 * 8 + 8
    assert C.sizeof(pkg.capi.DlConfigC) == 8 + 15 * 8 + 16
    assert C.sizeof(pkg.capi.DlIterC) == 96
    d = pkg.DogLegConfig().to_c()
    assert (d.trust_region_radius, d.mu, d.max_mu, d.use_jacobi_scaling, d.enable_step_reuse) == (1e4, 1e-4, 1.0, 1, 1)
    g = pkg.GaussNewtonConfig().to_c()
    assert (g.max_iterations, g.use_jacobi_scaling, g.variant) == (50, 0, 0)
