"""tests/manifold_ref.py proven on the CPU, and the host builds of the device headers held to it.

  * every function of manifold_ref against a 60-digit mpmath evaluation of the LITERAL formulas (no series, no regrouping:
    at 60 digits the cancellations are harmless) on the shared case list: 2^-60 relative to max(1, |value|max) per array;
  * the fp64 oracles' own distance from it, e_oracle, capped (1e-8 Jacobians, 1e-10 residuals and retractions): a
    condition on the cases, so that 8 e_oracle cannot hide a wrong formula;
  * the host harnesses compiled with -ffp-contract=off and with -ffp-contract=fast -mfma, under the referee rule
    e <= max(8 e_oracle, floor) of tests/test_gpu_manifold_edges.py on every case;
  * the retraction graphs populate every band of rotation-step norms the GPU test names (the oracles' solve)."""
import ctypes as C
import functools
import os
import subprocess

import numpy as np
import pytest

import manifold_ref as mr
import np_ref_se2 as ref2
from oracle import pg_oracle as po

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_f = np.ctypeslib.ndpointer(dtype=np.float64, flags="C_CONTIGUOUS")
AGREE = 2.0 ** -60
FLAGS = {"contract-off": ["-ffp-contract=off"], "contract-fast-fma": ["-ffp-contract=fast", "-mfma"]}


def c(a):
    return np.ascontiguousarray(a, dtype=np.float64)


# ---- shared data, computed once ----------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def se3():
    cs = mr.se3_cases()
    r, J = mr.se3_between(cs["k0"], cs["k1"], cs["meas"])
    ro = np.zeros((len(r), 6)); Jo = np.zeros((len(r), 6, 12))
    for e in range(len(r)):
        ro[e], Jo[e] = po.between_linearize(cs["k0"][e], cs["k1"][e], cs["meas"][e])
    return cs, r, J, ro, Jo


@functools.lru_cache(maxsize=None)
def se2():
    cs = mr.se2_cases()
    r, J = mr.se2_between(cs["k0"], cs["k1"], cs["meas"])
    ro, Jo = ref2.between_linearize(cs["k0"], cs["k1"], cs["meas"])
    return cs, r, J, ro, Jo


def corrected(r, J, delta):
    sc = mr.huber_scale(delta, (r * r).sum(-1))
    return r * sc[:, None], J * sc[:, None, None]


def corrected64(r, J, delta):
    """the fp64 oracles' loss correction (pg_oracle.c huber_scale, np_ref_se2.huber_scale)"""
    sc = ref2.huber_scale(delta, np.einsum("ei,ei->e", r, r))
    return r * sc[:, None], J * sc[:, None, None]


@functools.lru_cache(maxsize=None)
def se3_steps():
    """(poses, steps) of the SE3 retraction graph: the oracle's solve at RETRACT_LAMBDA, unscaled, per vertex"""
    prob, scal = mr.retraction_problem(se3()[0])
    o = po.PgOracle.from_problem(prob)
    o.linearize()
    o.set_column_scaling(scal)
    rc, y, _ = o.solve_augmented(mr.RETRACT_LAMBDA)
    assert rc == 0
    step = (y * scal)[prob.pose_col[:, None] + np.arange(6)[None]]
    return prob, step


@functools.lru_cache(maxsize=None)
def se2_steps():
    prob, scal = mr.retraction_problem(se2()[0])
    o = ref2.Problem.from_problem(prob)
    o.scaling = scal
    y, _ = o.solve(mr.RETRACT_LAMBDA)
    assert y is not None
    step = (y * scal)[prob.pose_col[:, None] + np.arange(3)[None]]
    return prob, step


# ---- mpmath: the literal formulas --------------------------------------------------------------------------------------
def _mp():
    mp = pytest.importorskip("mpmath")
    mp.mp.dps = 60
    return mp


class MpSe3:
    def __init__(self, mp):
        self.mp = mp
        self.small = mp.mpf(1e-10)

    def vec(self, v):
        return [self.mp.mpf(float(x)) for x in v]

    def cross(self, a, b):
        return [a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0]]

    def hat(self, v):
        return self.mp.matrix([[0, -v[2], v[1]], [v[2], 0, -v[0]], [-v[1], v[0], 0]])

    def qmul(self, a, b):
        cr = self.cross(a[1:], b[1:])
        return [a[0] * b[0] - (a[1] * b[1] + a[2] * b[2] + a[3] * b[3])] + [a[0] * b[i + 1] + b[0] * a[i + 1] + cr[i] for i in range(3)]

    def qrot(self, q, v):
        t = [2 * x for x in self.cross(q[1:], v)]
        cr = self.cross(q[1:], t)
        return [t[i] * q[0] + cr[i] + v[i] for i in range(3)]

    def from_vec(self, v):
        v = self.vec(v)
        q = v[3:]
        for _ in range(2):
            n = self.mp.sqrt(sum(x * x for x in q))
            q = [x / n for x in q]
        return v[:3], q

    def inv(self, t, q):
        qi = [q[0], -q[1], -q[2], -q[3]]
        return [-x for x in self.qrot(qi, t)], qi

    def mul(self, ta, qa, tb, qb):
        r = self.qrot(qa, tb)
        return [r[i] + ta[i] for i in range(3)], self.qmul(qa, qb)

    def rot(self, q):
        w, x, y, z = q
        return self.mp.matrix([[w * w + x * x - y * y - z * z, 2 * x * y - 2 * w * z, 2 * w * y + 2 * x * z],
                               [2 * w * z + 2 * x * y, w * w - x * x + y * y - z * z, 2 * y * z - 2 * w * x],
                               [2 * x * z - 2 * w * y, 2 * w * x + 2 * y * z, w * w - x * x - y * y + z * z]])

    def adjoint(self, t, q):
        mp = self.mp
        R = self.rot(q); TR = self.hat(t) * R
        A = mp.zeros(6, 6)
        for i in range(3):
            for j in range(3):
                A[i, j] = R[i, j]; A[i + 3, j + 3] = R[i, j]; A[i, j + 3] = TR[i, j]
        return A

    def log(self, q):
        mp = self.mp
        s2 = q[1] * q[1] + q[2] * q[2] + q[3] * q[3]
        coeff = mp.mpf(2)
        if s2 > self.small:
            s = mp.sqrt(s2)
            coeff = 2 * (mp.atan2(-s, -q[0]) if q[0] < 0 else mp.atan2(s, q[0])) / s
        return [x * coeff for x in q[1:]]

    def jlinv(self, th):
        mp = self.mp
        a = sum(x * x for x in th)
        K = self.hat(th)
        c2 = mp.mpf(0)
        if a > self.small:
            t = mp.sqrt(a)
            c2 = 1 / a - (1 + mp.cos(t)) / (2 * t * mp.sin(t))
        return mp.eye(3) - K / 2 + c2 * (K * K)

    def qblock(self, rho, th):
        mp = self.mp
        Rk, Tk = self.hat(rho), self.hat(th)
        t2 = sum(x * x for x in th)
        b, cc, d = mp.mpf(1) / 6 + t2 / 120, -mp.mpf(1) / 24 + t2 / 720, -mp.mpf(1) / 60
        if t2 > self.small:
            tn = mp.sqrt(t2)
            s, co = mp.sin(tn), mp.cos(tn)
            b = (tn - s) / tn ** 3
            cc = (1 - t2 / 2 - co) / tn ** 4
            d = (cc - 3) * (tn - s - tn ** 3 / 6) / tn ** 5
        tr, rt = Tk * Rk, Rk * Tk
        trt, rtt = tr * Tk, rt * Tk
        trtt = trt * Tk
        return Rk / 2 + (tr + rt + trt) * b - (rtt - rtt.T - trt * 3) * cc - trtt * d

    def between(self, k0, k1, m):
        mp = self.mp
        (t0, q0), (t1, q1), (tm, qm) = self.from_vec(k0), self.from_vec(k1), self.from_vec(m)
        tA, qA = self.mul(*self.inv(t1, q1), t0, q0)
        tD, qD = self.mul(tA, qA, tm, qm)
        th = self.log(qD)
        D = self.jlinv(th)
        rho = list(D * mp.matrix(tD))
        Q = self.qblock([-x for x in rho], [-x for x in th])
        B = -(D * Q * D)
        Jlog = mp.zeros(6, 6)
        for i in range(3):
            for j in range(3):
                Jlog[i, j] = D[i, j]; Jlog[i + 3, j + 3] = D[i, j]; Jlog[i, j + 3] = B[i, j]
        Am = self.adjoint(*self.inv(tm, qm))
        J0 = Jlog * Am
        J1 = Jlog * (Am * (-self.adjoint(*self.inv(tA, qA))))
        return rho + th, J0, J1

    def plus(self, pose, delta):
        mp = self.mp
        p, d = self.vec(pose), self.vec(delta)
        rho, th = d[:3], d[3:]
        a = sum(x * x for x in th)
        k1 = self.cross(th, rho); k2 = self.cross(th, k1)
        if a > self.small:
            h = [x / 2 for x in th]
            n = mp.sqrt(sum(x * x for x in h))
            s = mp.sin(n) / n
            qe = [mp.cos(n)] + [x * s for x in h]
            t = mp.sqrt(a)
            c1, c2 = (1 - mp.cos(t)) / a, (t - mp.sin(t)) / (a * t)
            te = [rho[i] + c1 * k1[i] + c2 * k2[i] for i in range(3)]
        else:
            qs = [mp.mpf(1)] + [x / 2 for x in th]
            n = mp.sqrt(sum(x * x for x in qs))
            qe = [x / n for x in qs]
            te = [rho[i] + k1[i] / 2 for i in range(3)]
        rt = self.qrot(p[3:], te)
        return [rt[i] + p[i] for i in range(3)] + self.qmul(p[3:], qe)


class MpSe2:
    def __init__(self, mp):
        self.mp = mp
        self.small = mp.mpf(1e-10)

    def mat(self, v):
        mp = self.mp
        x, y, th = (mp.mpf(float(a)) for a in v)
        return mp.matrix([[mp.cos(th), -mp.sin(th), x], [mp.sin(th), mp.cos(th), y], [0, 0, 1]])

    def inv(self, T):
        mp = self.mp
        Rt = mp.matrix([[T[0, 0], T[1, 0]], [T[0, 1], T[1, 1]]])
        t = -(Rt * mp.matrix([T[0, 2], T[1, 2]]))
        return mp.matrix([[Rt[0, 0], Rt[0, 1], t[0]], [Rt[1, 0], Rt[1, 1], t[1]], [0, 0, 1]])

    def adjoint(self, T):
        return self.mp.matrix([[T[0, 0], T[0, 1], T[1, 2]], [T[1, 0], T[1, 1], -T[0, 2]], [0, 0, 1]])

    def ab(self, th):
        mp = self.mp
        t2 = th * th
        if t2 < self.small:
            return 1 - t2 / 6, th / 2 - th * t2 / 24
        return mp.sin(th) / th, (1 - mp.cos(th)) / th

    def between(self, k0, k1, m):
        """right_jacobian_inv as tests/np_ref_se2.py states it (se2.rs:588-603: J00 = t sin t / (2 - 2 cos t), J02 = y/2 + x k,
        J12 = -x/2 + y k, k = (1 - J00) / t), every quotient taken literally"""
        mp = self.mp
        K0, K1, M = self.mat(k0), self.mat(k1), self.mat(m)
        A = self.inv(K1) * K0
        D = A * M
        th = mp.atan2(D[1, 0], D[0, 0])
        a, b = self.ab(th)
        den = a * a + b * b
        x, y = (a * D[0, 2] + b * D[1, 2]) / den, (-b * D[0, 2] + a * D[1, 2]) / den
        t2 = th * th
        if t2 > self.small:
            cs, sn = mp.cos(th), mp.sin(th)
            d = th * sn / (2 * (1 - cs))
            j02, j12 = y / 2 + x * (1 - d) / th, -x / 2 + y * (1 - d) / th
        else:
            d = 1 - t2 / 12
            j02, j12 = y / 2 + th * x / 12, -x / 2 + th * y / 12
        Jl = mp.matrix([[d, -th / 2, j02], [th / 2, d, j12], [0, 0, 1]])
        Am = self.adjoint(self.inv(M))
        return [x, y, th], Jl * Am, Jl * (Am * (-self.adjoint(self.inv(A))))

    def plus(self, v, d):
        mp = self.mp
        if all(float(x) == 0.0 for x in d):
            return [mp.mpf(float(x)) for x in v]
        tx, ty, th = (mp.mpf(float(x)) for x in d)
        a, b = self.ab(th)
        E = mp.matrix([[mp.cos(th), -mp.sin(th), a * tx - b * ty], [mp.sin(th), mp.cos(th), b * tx + a * ty], [0, 0, 1]])
        T = self.mat(v) * E
        return [T[0, 2], T[1, 2], mp.atan2(T[1, 0], T[0, 0])]


def _to_ld(mp, x):
    """an mpf rounded to long double (through two fp64 pieces)"""
    hi = float(x)
    return mr.LD(hi) + mr.LD(float(x - mp.mpf(hi)))


def _mp_err(mp, got, want_flat):
    want = np.array([_to_ld(mp, w) for w in want_flat], dtype=mr.LD)
    got = np.asarray(got, dtype=mr.LD).ravel()
    return float(np.abs(got - want).max() / max(mr.LD(1), np.abs(want).max()))


@functools.lru_cache(maxsize=None)
def se3_mp_errors():
    mp = _mp()
    M = MpSe3(mp)
    cs, r, J, _, _ = se3()
    _, step = se3_steps()
    poses = mr.graph_of(cs).poses
    P = mr.se3_plus(poses, step)
    er, ej = np.zeros(len(r)), np.zeros(len(r))
    for e in range(len(r)):
        rm, J0, J1 = M.between(cs["k0"][e], cs["k1"][e], cs["meas"][e])
        er[e] = _mp_err(mp, r[e], rm)
        ej[e] = max(_mp_err(mp, J[e][:, :6], list(J0)), _mp_err(mp, J[e][:, 6:], list(J1)))
    ep = np.array([_mp_err(mp, P[v], M.plus(poses[v], step[v])) for v in range(len(poses))])
    print("se3 reference vs mpmath, worst in units of 2^-60: r %.2f  J %.2f  plus %.2f" % (er.max() / AGREE, ej.max() / AGREE, ep.max() / AGREE))
    return cs, step, er, ej, ep


def test_se3_residual_reference_agrees_with_mpmath():
    cs, _, er, _, _ = se3_mp_errors()
    assert er.max() <= AGREE, (cs["label"][int(er.argmax())], er.max() / AGREE)


def test_se3_jacobian_reference_agrees_with_mpmath():
    """Measured worst 0.84 x 2^-60.  What decides it is the rounding of the stored unit quaternions to long double, which a
    translation multiplies: the inverse adjoints are therefore formed as [R^T, -R^T [t]x] (manifold_ref._adjoint_inv), and
    dr/dk1 from Adj((A meas)^-1) -- the reference's matrices in exact arithmetic, without the products that cancel."""
    cs, _, _, ej, _ = se3_mp_errors()
    assert ej.max() <= AGREE, (cs["label"][int(ej.argmax())], ej.max() / AGREE, int((ej > AGREE).sum()))


def test_se3_retraction_reference_agrees_with_mpmath():
    cs, step, _, _, ep = se3_mp_errors()
    v = int(ep.argmax())
    assert ep.max() <= AGREE, (cs["label"][v // 2], "vertex", v, "rotation step", float(np.linalg.norm(step[v, 3:])), ep.max() / AGREE)


def test_se2_reference_agrees_with_mpmath():
    mp = _mp()
    M = MpSe2(mp)
    cs, r, J, _, _ = se2()
    prob, step = se2_steps()
    poses = ref2.Problem.from_problem(prob).poses
    P = mr.se2_plus(poses, step)
    for e in range(len(r)):
        rm, J0, J1 = M.between(cs["k0"][e], cs["k1"][e], cs["meas"][e])
        er = _mp_err(mp, r[e], rm)
        ej = max(_mp_err(mp, J[e][:, :3], list(J0)), _mp_err(mp, J[e][:, 3:], list(J1)))
        assert er <= AGREE and ej <= AGREE, (cs["label"][e], er, ej)
    for v in range(len(poses)):
        ep = _mp_err(mp, P[v], M.plus(poses[v], step[v]))
        assert ep <= AGREE, (cs["label"][v // 2], "vertex", v, ep)


def test_huber_scale_agrees_with_mpmath():
    mp = _mp()
    s = np.concatenate([[np.nextafter(2.25, 0), 2.25, np.nextafter(2.25, 3)], np.random.default_rng(0).uniform(0, 40, 50)])
    got = mr.huber_scale(mr.HUBER_DELTA, s)
    for x, g in zip(s, got):
        want = mp.sqrt(mp.mpf(mr.HUBER_DELTA) / mp.sqrt(mp.mpf(float(x)))) if x > mr.HUBER_DELTA ** 2 else mp.mpf(1)
        assert abs(g - _to_ld(mp, want)) <= AGREE, (x, g)
    assert np.all(mr.huber_scale(None, s) == 1) and np.all(mr.huber_scale(-1.0, s) == 1)


# ---- the cap ---------------------------------------------------------------------------------------------------------
def test_the_oracles_stay_under_the_cap_on_every_case():
    for name, (cs, r, J, ro, Jo) in (("se3", se3()), ("se2", se2())):
        er, ej = mr.err(ro, r), mr.err(Jo, J)
        mr.report(f"{name} oracle vs reference", cs["angle"], e_r=er, e_J=ej)
        assert er.max() <= mr.CAP_R, (name, cs["label"][int(er.argmax())], er.max())
        assert ej.max() <= mr.CAP_J, (name, cs["label"][int(ej.argmax())], ej.max())
    prob, step = se3_steps()
    poses = prob.data.poses
    out = np.array([po.call("pgo_se3_plus", poses[v], step[v], out_shape=7) for v in range(len(poses))])
    ep = mr.err(out, mr.se3_plus(poses, step))
    assert ep.max() <= mr.CAP_R, (int(ep.argmax()), ep.max())
    prob2, step2 = se2_steps()
    poses2 = ref2.Problem.from_problem(prob2).poses
    ep2 = mr.err(ref2.plus(poses2, step2), mr.se2_plus(poses2, step2))
    assert ep2.max() <= mr.CAP_R, (int(ep2.argmax()), ep2.max())


def test_case_list_has_the_regimes_it_names():
    cs, r, J, _, _ = se3()
    th = np.linalg.norm(r[:, 3:].astype(np.float64), axis=1)
    want = np.array(cs["angle"])
    assert 240 <= len(want) <= 280
    assert np.abs(th - want).max() < 1e-12                      # the residual rotation is the angle aimed at
    assert (th == 0).sum() >= 18                                 # exactly zero, with either sign of the scalar part
    assert ((th ** 2 < mr.SMALL2) & (th > 0)).sum() >= 36 and (np.abs(th - np.pi) < 2e-6).sum() >= 18
    cs2, r2, _, _, _ = se2()
    th2 = np.abs(r2[:, 2].astype(np.float64))
    assert 110 <= len(th2) <= 130 and np.abs(th2 - np.abs(cs2["angle"])).max() < 1e-12
    for name, rr in (("se3", r), ("se2", r2)):                   # the Huber threshold is met from both sides, one ulp away
        s = (rr.astype(np.float64) ** 2).sum(-1)[-3:]
        assert s[0] == np.nextafter(2.25, 0) and s[1] == 2.25 and s[2] == np.nextafter(2.25, 3), (name, s)


# ---- the host builds under the referee rule -----------------------------------------------------------------------------
def build_harnesses(flags_name, csrc=None, tag=""):
    out = os.path.join(ROOT, "tests", "_build")
    os.makedirs(out, exist_ok=True)
    libs = []
    for src, stem in (("host_harness.cpp", "libmanifold_host"), ("host_harness_se2.cpp", "libmanifold_host_se2")):
        so = os.path.join(out, f"{stem}_{flags_name}{tag}.so")
        subprocess.run(["g++", "-O2", *FLAGS[flags_name], "-std=c++17", "-shared", "-fPIC",
                        "-I", csrc or os.path.join(ROOT, "apex-solver_amd", "csrc"), os.path.join(ROOT, "tests", src), "-o", so], check=True)
        libs.append(C.CDLL(so))
    L3, L2 = libs
    L3.hh_between_linearize.argtypes = [_f, _f, _f, C.c_double, _f, _f]
    L3.hh_se3_plus.argtypes = [_f, _f, _f]
    L2.hh2_between_linearize.argtypes = [_f, _f, _f, C.c_double, _f, _f]
    L2.hh2_plus.argtypes = [_f, _f, _f]
    return L3, L2


def host_failures(L3, L2):
    """Every (array, case) at which a host build of the headers misses the referee rule; empty: it holds."""
    bad = []
    for delta in (None, mr.HUBER_DELTA):
        for name, (cs, r, J, ro, Jo), fn, dof in (("se3", se3(), L3.hh_between_linearize, 6), ("se2", se2(), L2.hh2_between_linearize, 3)):
            rr, JJ = corrected(r, J, delta)
            rro, JJo = corrected64(ro, Jo, delta)
            n = len(rr)
            rh = np.zeros((n, dof)); Jh = np.zeros((n, dof, 2 * dof))
            for e in range(n):
                fn(c(cs["k0"][e]), c(cs["k1"][e]), c(cs["meas"][e]), -1.0 if delta is None else delta, rh[e], Jh[e])
            for what, eh, eo, floor in (("r", mr.err(rh, rr), mr.err(rro, rr), mr.FLOOR_R), ("J", mr.err(Jh, JJ), mr.err(JJo, JJ), mr.FLOOR_J)):
                ok, at = mr.referee(eh, eo, floor)
                if not ok:
                    bad.append((name, what, "huber" if delta else "no loss", cs["label"][at], float(eh[at]), float(eo[at])))
    prob, step = se3_steps()
    poses = prob.data.poses
    got = np.zeros_like(poses); oracle = np.zeros_like(poses)
    for v in range(len(poses)):
        L3.hh_se3_plus(c(poses[v]), c(step[v]), got[v])
        oracle[v] = po.call("pgo_se3_plus", poses[v], step[v], out_shape=7)
    want = mr.se3_plus(poses, step)
    ok, at = mr.referee(mr.err(got, want), mr.err(oracle, want), mr.FLOOR_POSE)
    if not ok:
        bad.append(("se3", "plus", "vertex %d" % at, "rotation step %.3e" % np.linalg.norm(step[at, 3:]), float(mr.err(got, want)[at]), float(mr.err(oracle, want)[at])))
    prob2, step2 = se2_steps()
    poses2 = ref2.Problem.from_problem(prob2).poses
    got2 = np.zeros_like(poses2)
    for v in range(len(poses2)):
        L2.hh2_plus(c(poses2[v]), c(step2[v]), got2[v])
    want2 = mr.se2_plus(poses2, step2)
    ok, at = mr.referee(mr.err(got2, want2), mr.err(ref2.plus(poses2, step2), want2), mr.FLOOR_POSE)
    if not ok:
        bad.append(("se2", "plus", "vertex %d" % at, "theta step %.3e" % step2[at, 2], float(mr.err(got2, want2)[at])))
    return bad


@pytest.mark.parametrize("flags", sorted(FLAGS))
def test_host_builds_meet_the_referee_rule(flags):
    bad = host_failures(*build_harnesses(flags))
    assert not bad, bad


# ---- band population ---------------------------------------------------------------------------------------------------
def test_retraction_graphs_populate_every_band():
    prob, step = se3_steps()
    free = ~prob.fix.astype(bool).all(axis=1)
    b = mr.band_of(np.linalg.norm(step[free, 3:], axis=1))
    counts = np.bincount(b, minlength=5)
    print("se3 rotation-step bands", dict(zip(mr.BAND_NAMES, counts)))
    assert (counts >= 8).all(), counts
    prob2, step2 = se2_steps()
    free2 = ~prob2.fix.astype(bool).all(axis=1)
    counts2 = np.bincount(mr.band_of(step2[free2, 2]), minlength=5)
    print("se2 theta-step bands", dict(zip(mr.BAND_NAMES, counts2)))
    assert (counts2 >= 8).all(), counts2
    poses2 = ref2.Problem.from_problem(prob2).poses
    after = ref2.plus(poses2[free2], step2[free2])[:, 2]
    crossed = (np.sign(after) != np.sign(poses2[free2, 2])) & (np.abs(after) > 3.0) & (np.abs(poses2[free2, 2]) > 3.0)
    assert crossed.sum() >= 2, crossed.sum()                     # a step that carries theta across +-pi


def test_ba_problem_populates_three_bands(oracle):
    """the premise of test_ba_camera_retraction_bands, with the oracle's first step"""
    from apex_solver_amd.solver import OptimizationType, Problem

    d = mr.ba_band_problem()
    prob = Problem.bundle_adjustment(d, OptimizationType.OnlyPose)
    o = oracle.from_data(d, prob.layout, mode="only_pose")
    o.linearize()
    step, _ = o.solve_augmented(mr.BA_LAMBDA, 0)
    rot = step[prob.layout.pose_col[1:, None] + np.arange(3, 6)[None]]
    counts = np.bincount(mr.band_of(np.linalg.norm(rot, axis=1)), minlength=5)
    print("ba rotation-step bands", dict(zip(mr.BAND_NAMES, counts.tolist())))
    assert (counts > 0).sum() >= 3, counts


def test_both_sides_of_the_huber_loss_are_populated():
    for data in (se3(), se2()):
        sc = mr.huber_scale(mr.HUBER_DELTA, (data[1] * data[1]).sum(-1))
        assert (sc < 1).sum() >= 8 and (sc == 1).sum() >= 2, ((sc < 1).sum(), (sc == 1).sum())
