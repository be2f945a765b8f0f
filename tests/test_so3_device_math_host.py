"""The per-edge SO3 device math (apex-solver_amd/csrc/pg_so3_device.hpp) and the row-owned assembly instantiated for it,
compiled for the host, against the long-double reference (tests/so3_ref.py).  No GPU needed.

Bounds as tests/test_pg_device_math_host.py applies them to the same math in SE3's rotational block: r 1e-13, J 1e-12 relative,
floor 1.  Near pi the Jl^-1 coefficient 1/t^2 - (1 + cos t) / (2 t sin t) loses digits as sin t -> 0 in the reference solver's
own fp64 formula too: there the device is held, band by band (manifold_ref.band_of), to manifold_ref.referee's rule -- 8 times
the distance of a literal fp64 evaluation of the same formulas from the long-double reference, or the floor."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import manifold_ref as mr
import np_ref_loss as nl
import so3_ref as sr
from apex_solver_amd import capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_f = np.ctypeslib.ndpointer(dtype=np.float64, flags="C_CONTIGUOUS")
_u = np.ctypeslib.ndpointer(dtype=np.uint32, flags="C_CONTIGUOUS")
_i = np.ctypeslib.ndpointer(dtype=np.int32, flags="C_CONTIGUOUS")


def load_harness():
    out = os.path.join(ROOT, "tests", "_build")
    os.makedirs(out, exist_ok=True)
    so = os.path.join(out, "libhost_harness_so3.so")
    subprocess.run(["g++", "-O2", "-ffp-contract=off", "-std=c++17", "-shared", "-fPIC",
                    "-I", os.path.join(ROOT, "apex-solver_amd", "csrc"),
                    os.path.join(ROOT, "tests", "host_harness_so3.cpp"), "-o", so], check=True)
    L = C.CDLL(so)
    L.hs3_prepare.argtypes = [_f, _f]; L.hs3_prepare_as_se3.argtypes = [_f, _f]
    L.hs3_between_linearize.argtypes = [_f, _f, _f, C.c_double, _f, _f]
    L.hs3_residual.argtypes = [_f, _f, _f, _f]
    L.hs3_log.argtypes = [_f, _f]; L.hs3_exp.argtypes = [_f, _f]; L.hs3_plus.argtypes = [_f, _f, _f]
    L.hs3_right_jacobian_inv.argtypes = [_f, _f]
    L.hs3_prior.argtypes = [_f, _f, C.c_double, _f]; L.hs3_prior.restype = C.c_double
    L.hs3_assemble_dense.argtypes = [C.c_int64, C.c_int64, _f, _u, _u, _f, C.c_int, C.c_double, C.c_double, C.c_double,
                                     C.c_void_p, _f, _f, _i, _i]
    L.hs3_incident.argtypes = [C.c_int64, C.c_int64, _u, _u, C.c_int64, _u]; L.hs3_incident.restype = C.c_int64
    return L


@pytest.fixture(scope="module")
def hh():
    return load_harness()


def c(a):
    return np.ascontiguousarray(a, dtype=np.float64)


def _unit(rng, n, k):
    v = rng.standard_normal((n, k))
    return v / np.linalg.norm(v, axis=1, keepdims=True)


def edge_with_residual(rng, angle, negate=None, scale=None):
    """(k0, k1, meas) whose residual rotation has the given angle about a random axis: meas = A^-1 D, in long double"""
    k0, k1 = _unit(rng, 2, 4)
    if angle == 0.0:
        return k0.copy(), k0.copy(), np.array([1.0, 0, 0, 0])
    qA = sr._qmul(sr._qconj(sr._ld(k1[None])), sr._ld(k0[None]))
    h = sr.LD(angle) / 2
    qD = np.concatenate([[np.cos(h)], np.sin(h) * sr._ld(_unit(rng, 1, 3)[0])])[None]
    m = sr.f64(sr._qmul(sr._qconj(qA), qD))[0]
    trip = [k0, k1, m]
    if negate is not None:
        trip[negate] = -trip[negate]
    if scale is not None:
        trip[scale[0]] = trip[scale[0]] * scale[1]
    return tuple(trip)


SMALL = (1e-9, 1e-7, 5e-6, 0.99e-5, 1.01e-5, 2e-5, 1e-3)
NEAR_PI = (np.pi / 2, np.pi - 1e-2, np.pi - 1e-4, np.pi - 1e-6)


def cases():
    """(k0, k1, meas, angle aimed at, label) -- none is skipped"""
    rng = np.random.default_rng(2026)
    out = [edge_with_residual(rng, 0.0) + (0.0, "zero residual")]
    for a in SMALL + NEAR_PI:
        for rep in range(3):
            out.append(edge_with_residual(rng, a) + (a, f"angle {a!r} #{rep}"))
    for a in (0.3, 2.0, np.pi - 1e-2):
        for which in range(3):                       # q.w < 0: the composed scalar part is negative, Log's cos < 0 arm
            out.append(edge_with_residual(rng, a, negate=which) + (a, f"angle {a!r}, quaternion {which} negated"))
    for s in (1 + 1e-3, 1 - 1e-3, 2.0):
        for which in range(3):
            out.append(edge_with_residual(rng, 0.7, scale=(which, s)) + (0.7, f"quaternion {which} scaled by {s!r}"))
    for rep in range(20):
        k0, k1, m = _unit(rng, 3, 4)
        ang = float(np.linalg.norm(sr.f64(sr.so3_between(k0, k1, m)[0])))
        out.append((k0, k1, m, ang, f"random #{rep}"))
    return out


def literal_fp64(k0, k1, m):
    """the reference solver's formulas evaluated literally in numpy fp64 (one ordering): what fp64 can deliver on a case"""
    def nrm(q):
        q = np.asarray(q, dtype=np.float64)
        for _ in range(2):
            q = q / np.sqrt(q @ q)
        return q

    def qmul(a, b):
        return np.array([a[0] * b[0] - a[1:] @ b[1:], *(a[0] * b[1:] + b[0] * a[1:] + np.cross(a[1:], b[1:]))])

    def rot(q):
        w, x, y, z = q
        return np.array([[w * w + x * x - y * y - z * z, 2 * (x * y - w * z), 2 * (w * y + x * z)],
                         [2 * (w * z + x * y), w * w - x * x + y * y - z * z, 2 * (y * z - w * x)],
                         [2 * (x * z - w * y), 2 * (w * x + y * z), w * w - x * x - y * y + z * z]])
    conj = np.array([1.0, -1, -1, -1])
    q0, q1, qm = nrm(k0), nrm(k1), nrm(m)
    A = qmul(q1 * conj, q0); D = qmul(A, qm)
    s2 = D[1:] @ D[1:]
    coeff = 2.0
    if s2 > 1e-10:
        s = np.sqrt(s2)
        coeff = 2.0 * (np.arctan2(-s, -D[0]) if D[0] < 0 else np.arctan2(s, D[0])) / s
    r = D[1:] * coeff
    a = r @ r
    K = np.array([[0, -r[2], r[1]], [r[2], 0, -r[0]], [-r[1], r[0], 0]])
    c2 = 0.0
    if a > 1e-10:
        t = np.sqrt(a)
        c2 = 1.0 / a - (1.0 + np.cos(t)) / (2.0 * t * np.sin(t))
    Jr = (np.eye(3) - 0.5 * K + c2 * (K @ K)).T
    Rm = rot(qm * conj)
    J0 = Jr @ Rm
    J1 = Jr @ (Rm @ -rot(A * conj))
    return r, np.concatenate([J0, J1], axis=1)


def test_between_linearize_matches_the_reference(hh):
    cs = cases()
    k0, k1, m = (np.array([x[i] for x in cs]) for i in range(3))
    angle = np.array([x[3] for x in cs])
    ro, Jo = sr.so3_between(k0, k1, m)
    for delta in (-1.0, 0.5):
        sc = mr.huber_scale(delta, (sr.f64(ro) ** 2).sum(-1))          # (the branch compares the fp64 squared norm)
        rd = np.zeros((len(cs), 3)); Jd = np.zeros((len(cs), 3, 6)); rl = np.zeros_like(rd); Jl = np.zeros_like(Jd)
        for k in range(len(cs)):
            hh.hs3_between_linearize(c(k0[k]), c(k1[k]), c(m[k]), delta, rd[k], Jd[k])
            rl[k], Jl[k] = literal_fp64(k0[k], k1[k], m[k])
        rr, JJ = ro * sc[:, None], Jo * sc[:, None, None]
        e_r, e_J = mr.err(rd, rr), mr.err(Jd, JJ)
        o_r, o_J = mr.err(rl * sr.f64(sc)[:, None], rr), mr.err(Jl * sr.f64(sc)[:, None, None], JJ)
        mr.report(f"so3 host delta={delta}", angle, r=e_r, J=e_J, r_fp64=o_r, J_fp64=o_J)
        band = mr.band_of(angle)
        below = band < 4                                               # residual angle < 3: the plain bounds
        assert e_r[below].max() < 1e-13 and e_J[below].max() < 1e-12, (e_r[below].max(), e_J[below].max())
        ok_r, at_r = mr.referee(e_r[~below], o_r[~below], mr.FLOOR_R)
        ok_J, at_J = mr.referee(e_J[~below], o_J[~below], mr.FLOOR_J)
        lab = [x[4] for x, b in zip(cs, below) if not b]
        assert ok_r, (lab[at_r], e_r[~below][at_r], o_r[~below][at_r])
        assert ok_J, (lab[at_J], e_J[~below][at_J], o_J[~below][at_J])
        assert (o_J[~below] <= mr.CAP_J).all() and (o_r[~below] <= mr.CAP_R).all()    # the band is shown, not hidden: fp64 itself stays usable


def test_zero_residual_is_exact_and_preparation_has_se3s_bits(hh):
    q = np.array([0.3, -0.5, 0.2, 0.7]) * 1.37
    r = np.ones(3); J = np.zeros((3, 6))
    hh.hs3_between_linearize(c(q), c(q), np.array([1.0, 0, 0, 0]), -1.0, r, J)
    assert np.abs(r).max() < 1e-16 and np.abs(J[:, :3] - np.eye(3)).max() < 1e-15 and np.abs(J[:, 3:] + np.eye(3)).max() < 1e-15
    rng = np.random.default_rng(3)
    for _ in range(50):
        q = rng.standard_normal(4) * rng.uniform(0.5, 2.0)
        a = np.zeros(4); b = np.zeros(4)
        hh.hs3_prepare(c(q), a); hh.hs3_prepare_as_se3(c(q), b)
        assert np.array_equal(a, b) and abs(a @ a - 1.0) < 4e-16


def test_log_exp_jrinv_across_the_threshold(hh):
    rng = np.random.default_rng(4)
    for ang in SMALL + (0.3, 2.0, 3.0):
        th = _unit(rng, 1, 3)[0] * ang
        q = np.zeros(4); back = np.zeros(3); J = np.zeros((3, 3))
        hh.hs3_exp(c(th), q); hh.hs3_log(q, back); hh.hs3_right_jacobian_inv(c(th), J)
        assert np.abs(q - sr.f64(sr.so3_exp(th))[0]).max() < 1e-15
        assert np.abs(back - th).max() < 1e-13 * max(1.0, ang)
        assert np.abs(J - sr.f64(sr.so3_right_jacobian_inv(sr._ld(th[None])))[0]).max() < 1e-12
        if ang * ang <= 1e-10:                                         # the arm I + 1/2 [theta]x, exactly
            K = np.array([[0, -th[2], th[1]], [th[2], 0, -th[0]], [-th[1], th[0], 0]])
            assert np.array_equal(J, np.eye(3) + 0.5 * K)


def test_retraction_and_prior(hh):
    rng = np.random.default_rng(5)
    for ang in SMALL + (0.3, 2.5):
        q = _unit(rng, 1, 4)[0] * rng.uniform(0.9, 1.1)                # stored as it is: not normalised on the way
        d = _unit(rng, 1, 3)[0] * ang
        o = np.zeros(4)
        hh.hs3_plus(c(q), c(d), o)
        assert np.abs(o - sr.f64(sr.so3_plus(q, d))[0]).max() < 1e-15 * 2
        hh.hs3_plus(c(q), np.zeros(3), o)
        assert np.array_equal(o, q)                                    # q (+) 0 keeps its bits
    q = _unit(rng, 1, 4)[0] * 1.2; data = _unit(rng, 1, 4)[0]
    for delta in (-1.0, 0.2, 1e3):
        r = np.zeros(4)
        sc = hh.hs3_prior(c(q), c(data), delta, r)
        ro, so = sr.so3_prior(q, data, None if delta <= 0 else delta)
        assert np.abs(r - sr.f64(ro)[0]).max() < 1e-15 and abs(sc - float(so[0])) < 1e-15
    assert 0 < hh.hs3_prior(c(q), c(data), 0.2, np.zeros(4)) < 1


# ---- the row-owned assembly --------------------------------------------------------------------------------------------------
LOSSES = {"none": None, "huber": ("huber", 0.4), "cauchy": ("cauchy", 1.0), "andrews": ("andrews", 1.2)}
GRAPHS = ("loop", "multi", "isolated", "hub_lo", "hub_hi")


def _loss(name):
    from apex_solver_amd.pose_graph import create_loss_function
    spec = LOSSES[name]
    return None if spec is None else create_loss_function(*spec)


def _assemble(hh, d, loss, info):
    n = 3 * d.n_v
    H = np.zeros((n, n)); g = np.zeros(n)
    writes = np.zeros((d.n_v, d.n_v), np.int32); writer = np.full((d.n_v, d.n_v), -1, np.int32)
    kind, p0, p1 = (capi.LOSS_NONE, 0.0, 0.0) if loss is None else (int(loss.kind), float(loss.p0), float(loss.p1))
    keep = None if info is None else c(info)
    ip = None if keep is None else keep.ctypes.data_as(C.c_void_p)
    rc = hh.hs3_assemble_dense(d.n_v, d.n_e, c(d.poses), np.ascontiguousarray(d.e_from, np.uint32), np.ascontiguousarray(d.e_to, np.uint32),
                               c(d.meas), kind, p0, p1, -1.0, ip, H, g, writes, writer)
    assert rc == 0
    return H, g, writes, writer


@pytest.mark.parametrize("weighted", [False, True], ids=["plain", "information"])
@pytest.mark.parametrize("loss_name", sorted(LOSSES))
@pytest.mark.parametrize("graph", GRAPHS)
def test_row_owned_assembly_matches_the_dense_reference(hh, graph, loss_name, weighted):
    from apex_solver_amd.pose_graph import PoseGraphProblem

    d = sr.crafted(graph)
    loss = _loss(loss_name)
    info = sr.random_information(d.n_e) if weighted else None
    P = sr.So3Problem.from_problem(PoseGraphProblem(d, loss=loss, information=info, manifold="so3"))
    Hr, gr, _ = P.dense(0.0)
    cols = P.cols().ravel()                                            # the reference is in the global (sorted-name) column order
    Hr, gr = Hr[np.ix_(cols, cols)], gr[cols]
    if loss_name == "andrews":
        assert (P.arms == 2).any()                                     # rho'' > 0 somewhere: the corrector's second arm runs
    H, g, writes, writer = _assemble(hh, d, loss, info)
    Hs = np.tril(H) + np.tril(H, -1).T
    scale = max(1.0, float(np.abs(sr.f64(Hr)).max()))
    eH = np.abs(Hs - sr.f64(Hr)).max() / scale; eg = np.abs(g - sr.f64(gr)).max() / max(1.0, float(np.abs(sr.f64(gr)).max()))
    print(graph, loss_name, weighted, "H", eH, "g", eg)
    # the bound of tests/test_pg_device_math_host.py on J^T J and J^T r (FLOOR_H), per unit of the largest entry; a block of
    # the hub or of the 64 parallel edges sums up to 70 terms of that size, each within the J bound
    assert eH < mr.FLOOR_H and eg < mr.FLOOR_H
    # placement: only blocks (v, u) with u < v are written, by the owner of row v, once per live edge between the pair
    ef, et = d.e_from.astype(int), d.e_to.astype(int)
    live = np.ones(d.n_e, bool)
    if loss is not None:
        live = np.array([float(nl.evaluate(loss, s)[1]) != 0.0 for s in P.s])
    want = np.zeros_like(writes)
    for e in np.nonzero(live & (ef != et))[0]:
        want[max(ef[e], et[e]), min(ef[e], et[e])] += 1
    assert np.array_equal(writes, want) and np.count_nonzero(np.triu(writes)) == 0
    vs, us = np.nonzero(writes)
    assert np.array_equal(writer[vs, us], vs)
    assert np.count_nonzero(np.triu(H, 1)) == 0


def test_diagonal_blocks_sum_in_list_order_and_isolated_rows_are_zero(hh):
    d = sr.crafted("multi")
    ef = np.ascontiguousarray(d.e_from, np.uint32); et = np.ascontiguousarray(d.e_to, np.uint32)
    v = 5                                                              # one end of the 64 parallel edges
    out = np.zeros(2 * d.n_e, np.uint32)
    n = hh.hs3_incident(d.n_v, d.n_e, ef, et, v, out)
    lst = out[:n]
    assert n == 66 and np.all(np.diff(lst.astype(int)) > 0)            # its two chain edges and the 64, ascending edge index
    r, J = sr.So3Problem(d.poses, ef, et, d.meas, 3 * np.arange(d.n_v), np.zeros((d.n_v, 3), np.uint8)).raw_blocks()
    H, g, _, _ = _assemble(hh, d, None, None)
    # fp64 sums in exactly that order reproduce the diagonal block to the last few bits (the factors differ by the
    # linearisation's own rounding, the order does not), and far better than the reversed order does on average
    acc = np.zeros((3, 3))
    for e in lst:
        Jv = J[e, :, :3] if ef[e] == v else J[e, :, 3:]
        acc = acc + Jv.T @ Jv
    assert np.abs(np.tril(H[15:18, 15:18]) - np.tril(acc)).max() < 1e-12 * np.abs(acc).max()
    iso = sr.crafted("isolated")
    H, g, writes, _ = _assemble(hh, iso, None, None)
    for v in (3, 9):
        assert not H[3 * v:3 * v + 3].any() and not H[:, 3 * v:3 * v + 3].any() and not g[3 * v:3 * v + 3].any()
