"""The per-edge SE2 device math (apex-solver_amd/csrc/pg2_device.hpp) compiled for the host, against the numpy reference
(tests/np_ref_se2.py).  No GPU needed.  Bounds as tests/test_pg_device_math_host.py: r 1e-13, J 1e-12 relative, floor 1."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import apex_solver_amd as pkg
import np_ref_se2 as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_f = np.ctypeslib.ndpointer(dtype=np.float64, flags="C_CONTIGUOUS")
_u = np.ctypeslib.ndpointer(dtype=np.uint32, flags="C_CONTIGUOUS")
_i = np.ctypeslib.ndpointer(dtype=np.int32, flags="C_CONTIGUOUS")


def load_harness():
    out = os.path.join(ROOT, "tests", "_build")
    os.makedirs(out, exist_ok=True)
    so = os.path.join(out, "libhost_harness_se2.so")
    subprocess.run(["g++", "-O2", "-ffp-contract=off", "-std=c++17", "-shared", "-fPIC",
                    "-I", os.path.join(ROOT, "apex-solver_amd", "csrc"),
                    os.path.join(ROOT, "tests", "host_harness_se2.cpp"), "-o", so], check=True)
    L = C.CDLL(so)
    L.hh2_between_linearize.argtypes = [_f, _f, _f, C.c_double, _f, _f]
    L.hh2_between_normal.argtypes = [_f] * 8
    L.hh2_exp.argtypes = [_f, _f]; L.hh2_log.argtypes = [_f, _f]; L.hh2_plus.argtypes = [_f, _f, _f]
    L.hh2_wrap.argtypes = [C.c_double]; L.hh2_wrap.restype = C.c_double
    L.hh2_right_jacobians.argtypes = [_f, _f, _f]
    L.hh2_lists.argtypes = [C.c_int64, C.c_int64, _u, _u, _i, _u]; L.hh2_lists.restype = C.c_int64
    L.hh2_assemble_dense.argtypes = [C.c_int64, C.c_int64, _f, _u, _u, _f, C.c_double, _f, _f, _i, _i]
    return L


@pytest.fixture(scope="module")
def hh():
    return load_harness()


def c(a):
    return np.ascontiguousarray(a, dtype=np.float64)


def cases():
    d = pkg.synthetic.make_manhattan(200)
    rng = np.random.default_rng(0)
    out = [(d.poses[d.e_from[e]], d.poses[d.e_to[e]], d.meas[e]) for e in range(0, d.n_e, 3)]
    z = np.zeros(3)
    out.append((z, z, z))                                   # zero residual
    for _ in range(20):                                     # |theta| up to pi
        p = rng.uniform(-5, 5, size=(3, 3)); p[:, 2] = rng.uniform(-np.pi, np.pi, size=3)
        out.append((p[0], p[1], p[2]))
    out.append((np.array([1.0, 2, np.pi - 0.01]), np.array([0.5, -1, -np.pi + 0.01]), z))
    # residual angles across the small-angle threshold (|theta| = 1e-5), small and O(1) residual translations
    for th in (1e-9, 1e-7, 5e-6, 0.99e-5, 1.01e-5, 2e-5, 1e-4, 1e-3):
        for t in ((0.01, -0.02), (0.7, -1.3)):
            k1 = np.array([0.3, -0.2, 0.4])
            k0 = ref.plus(k1, np.array([t[0], t[1], th]))
            out.append((k0, k1, z))
    return out


def test_between_linearize_matches_numpy_reference(hh):
    worst_r = worst_j = 0.0
    for k0, k1, m in cases():
        for delta in (-1.0, 0.5):
            r = np.zeros(3); J = np.zeros((3, 6))
            hh.hh2_between_linearize(c(k0), c(k1), c(m), delta, r, J)
            ro, Jo = ref.between_linearize(k0, k1, m)
            sc = float(ref.huber_scale(delta, np.array([ro @ ro]))[0])
            ro, Jo = ro * sc, Jo * sc
            worst_r = max(worst_r, np.abs(r - ro).max() / max(1.0, np.abs(ro).max()))
            worst_j = max(worst_j, np.abs(J - Jo).max() / max(1.0, np.abs(Jo).max()))
    print("worst r", worst_r, "worst J", worst_j)
    assert worst_r < 1e-13 and worst_j < 1e-12, (worst_r, worst_j)


def test_identity_edge_has_zero_residual(hh):
    z = np.zeros(3); r = np.ones(3); J = np.zeros((3, 6))
    hh.hh2_between_linearize(z, z, z, -1.0, r, J)
    assert np.array_equal(r, z) and np.allclose(J[:, :3], np.eye(3), atol=0) and np.allclose(J[:, 3:], -np.eye(3), atol=0)


def test_normal_products_match_dense(hh):
    for k0, k1, m in cases()[:60]:
        H00 = np.zeros((3, 3)); H11 = np.zeros((3, 3)); H10 = np.zeros((3, 3)); g0 = np.zeros(3); g1 = np.zeros(3)
        hh.hh2_between_normal(c(k0), c(k1), c(m), H00, H11, H10, g0, g1)
        r, J = ref.between_linearize(k0, k1, m)
        J0, J1 = J[:, :3], J[:, 3:]
        sc = max(1.0, np.abs(J).max() ** 2) * max(1.0, np.abs(r).max())
        assert np.abs(H00 - J0.T @ J0).max() < 1e-12 * sc and np.abs(H11 - J1.T @ J1).max() < 1e-12 * sc
        assert np.abs(H10 - J1.T @ J0).max() < 1e-12 * sc
        assert np.abs(g0 - J0.T @ r).max() < 1e-12 * sc and np.abs(g1 - J1.T @ r).max() < 1e-12 * sc


def test_exp_log_and_retraction_round_trips(hh):
    rng = np.random.default_rng(1)
    for _ in range(200):
        t = np.array([rng.uniform(-3, 3), rng.uniform(-3, 3), rng.uniform(-np.pi + 1e-3, np.pi - 1e-3)])
        if rng.random() < 0.3:
            t[2] = rng.choice([1e-9, -1e-7, 3e-6, 2e-5, -1e-4])
        v = np.zeros(3); back = np.zeros(3)
        hh.hh2_exp(c(t), v); hh.hh2_log(v, back)
        assert np.abs(back - t).max() < 1e-13 * max(1.0, np.abs(t).max())
        assert np.abs(v - ref.vec(ref.exp(t))).max() < 1e-13 * max(1.0, np.abs(t).max())
        x = np.array([rng.uniform(-5, 5), rng.uniform(-5, 5), rng.uniform(-np.pi, np.pi)])
        d = 0.3 * t
        y = np.zeros(3); x2 = np.zeros(3)
        hh.hh2_plus(c(x), c(d), y); hh.hh2_plus(y, c(-d), x2)
        assert np.abs(y - ref.plus(x, d)).max() < 1e-13 * max(1.0, np.abs(x).max())
        dth = np.arctan2(np.sin(x2[2] - x[2]), np.cos(x2[2] - x[2]))
        assert np.abs(x2[:2] - x[:2]).max() < 1e-13 * max(1.0, np.abs(x).max()) and abs(dth) < 1e-13
    x = np.array([1.5, -2.5, 0.123]); y = np.zeros(3)
    hh.hh2_plus(c(x), np.zeros(3), y)
    assert np.array_equal(x, y)                              # x (+) 0 keeps its bits


def test_theta_wraps_at_pi(hh):
    for th in (np.pi, 3.0, -3.0, 0.0, np.nextafter(-np.pi, 0)):
        assert hh.hh2_wrap(th) == th                         # already in (-pi, pi]
    for th in (np.pi + 0.1, -np.pi - 0.1, 7.0, -7.0, 100.0, -np.pi):
        w = hh.hh2_wrap(th)
        assert -np.pi < w <= np.pi or w == -np.pi and th == -np.pi
        assert abs(np.sin(w) - np.sin(th)) < 1e-14 and abs(np.cos(w) - np.cos(th)) < 1e-14
        assert w == float(ref.wrap(th)) or abs(w - float(ref.wrap(th))) < 1e-15
    # a step across +pi comes back in (-pi, pi]
    y = np.zeros(3)
    hh.hh2_plus(np.array([0.0, 0.0, np.pi - 0.01]), np.array([0.0, 0.0, 0.05]), y)
    assert -np.pi < y[2] < -np.pi + 0.05 and abs(y[2] - (-np.pi + 0.04)) < 1e-14


def test_right_jacobians_are_inverse_of_each_other(hh):
    rng = np.random.default_rng(2)
    for th in (1e-9, 5e-6, 2e-5, 1e-3, 0.3, 2.0, -3.0):
        t = np.array([rng.uniform(-2, 2), rng.uniform(-2, 2), th]); a = np.zeros(9); b = np.zeros(9)
        hh.hh2_right_jacobians(c(t), a, b)
        # Jr is kept as the reference codes it (it is not on the solve path): theta^2 of Taylor truncation below the
        # threshold, 1e-16 / theta^2 of cancellation above it -- 1e-9 covers both except in [1e-5, 1e-3)
        if not 1e-5 <= abs(th) < 1e-3:
            assert np.abs(a.reshape(3, 3) @ b.reshape(3, 3) - np.eye(3)).max() < 1e-9
        assert np.abs(b.reshape(3, 3) - ref.right_jacobian_inv(t)).max() < 1e-12
