"""The robust-loss correction edge by edge: the cases, the long-double reference and its fp64 restatement that the host test
(tests/test_loss_edge_cases_host.py) and the device test (tests/test_gpu_loss_edges.py) share -- TEST INFRASTRUCTURE ONLY.

Layout of tests/manifold_ref.py: per (manifold, kind, policy) one graph of disjoint vertex pairs, one edge per case, so that
every block of H and every row of g belongs to exactly one edge; every other pair is stored with `from` on the higher vertex
(the cross block of the lower triangle is then J_from^T J_to, the order the weighted forms tell apart); three lonely vertices
carry a self-loop each.

Kinds: the 20 parameterisations of tests/test_loss_device_math_host.py with Tukey's and Andrews' scales lowered so that every
threshold lies below s = 8 (SO3: |r| <= pi), Barron alpha = 3 (second arm at every s > 0) and Welsch at scale 0.1, whose
rho' = exp(-s / c^2) / 2 is subnormal at s = 730 c^2 and exactly 0 at s = 760 c^2 (exp underflows below -745.13).

Targets: s_grid of the host test (0, either side of f64::EPSILON, both sides of every threshold 1e-4 away, the decades
1e-12 .. 1e6), cut at s < pi^2 for SO3 in the list itself.  Two families:
  axis     identity rotations and a translation (SO3: an angle) along one or two axes: r is exact (SO3: to an ulp) and s is
           hit to an ulp.  Every target below 1e-6 and every target next to a threshold.  A residual of 1e-8 that went through a
           generic log has 1e-8 relative noise in its direction, which alpha / s r r^T carries into J~ (loss_graphs.graph).
  generic  random poses, measurement = true relative pose composed with Exp(tau), |tau|^2 = s: r r^T J is a full matrix.
           Targets in [1e-6, 1e6].
Policies: "general" (s = r^T r) and "weighted" (a fixed SPD Omega per edge, cond <= 100, s = r^T Omega r; the geometry is
scaled so that the target is hit through Omega).

Reference (long double): manifold_ref / so3_ref between-factor, then Corrector::new of np_ref_loss at the fp64 rounding of s:
    r^ = residual_scaling r,  J^ = sqrt(rho') (J - a r (Omega r)^T J),  exports r~ = U r^, J~ = U J^ (Omega = U^T U; I: general)
    blocks J^_x^T Omega J^_y, gradients J^_x^T Omega r^, Gram sums (J^ a)^T Omega (J^ b), cost term residual_scaling^2 s.
fp64 restatement: the fp64 linearisations the suite already has (oracle/pg_oracle.c, np_ref_se2, and for SO3 pg_oracle's
so3_log and Jl^-1 between numpy quaternion products), whitened by np_ref_info.whiten, corrected by np_ref_loss.correct with
dtype = float64, multiplied out by numpy.  Its distance from the reference is e_f64.

Rule, per edge and per output (errors as max |x - ref| / max(1, max |ref|)):

    e <= max(8 e_f64, floor max(1, kappa)),    kappa = |s rho'' / rho'|

floor 1e-13 for r~ and cost, 1e-12 max(1, |J|max^2) for J~, blocks, gradients and Gram sums (test_loss_device_math_host.py);
kappa is the condition number of rho' in s (so3_ref.asm_reference): whoever rebuilds s from its own linearisation moves rho' by
kappa eps.  No further conditioning term was needed: see DESIGN.md section 11 for the measured ratios.
"""
from __future__ import annotations

import functools
from types import SimpleNamespace

import numpy as np

import manifold_ref as mr
import np_ref_info as ni
import np_ref_loss as nl
import np_ref_se2
import so3_ref as sr
from apex_solver_amd import capi
from manifold_ref import LD
from test_loss_device_math_host import KINDS as HOST_KINDS, s_grid

EPS = nl.EPS
MANIFOLDS = ("se3", "se2", "so3")
DOF = {"se3": 6, "se2": 3, "so3": 3}
AMB = {"se3": 7, "se2": 3, "so3": 4}
POLICIES = ("general", "weighted")
SCALE_OVERRIDE = {"TUKEY": 2.0, "ANDREWS": 0.8}      # c^2 = 4; (pi c)^2 = 6.32, (pi c / 2)^2 = 1.58: all below 8
KINDS = [(n, SCALE_OVERRIDE.get(n, p0), p1) for n, p0, p1 in HOST_KINDS] + [("BARRON", 3.0, 1.0), ("WELSCH", 0.1, 0)]
SECOND_ARM = [("ANDREWS", 0.8, 0), ("LP_NORM", 3.0, 0)]      # the kinds with both arms on the grid (Barron 3: second at every s > 0)
REDESCENDING = ("TUKEY", "ANDREWS", "TRIMMED_MEAN")          # rho' = 0 beyond a cut
SO3_CUT = float(np.pi) ** 2
AXIS_BELOW = 1e-6
N_LOOPS = 3
LOOP_S = (1e-3, 0.5, 3.0)
LAMBDA = 0.5
FLOOR_R, FLOOR_J = 1e-13, 1e-12


def kind_id(k):
    return f"{k[0]}-{k[1]}"


def mk(kind):
    return SimpleNamespace(kind=capi.LOSS_KINDS.index(kind[0]), p0=float(kind[1]), p1=float(kind[2]))


def targets(kind, manifold):
    """[(s, family, both)] of one kind: family "axis" | "generic"; both: the one-axis and the two-axis form (else they alternate)"""
    loss = mk(kind)
    grid = s_grid(loss)
    fixed = len(grid) - 38                       # the decades are the last 38 entries of s_grid
    out = []
    for i, s in enumerate(grid):
        if i < fixed:
            out.append((s, "axis", s != EPS))    # s == EPS is hit exactly, which only one axis can do
        else:
            out.append((s, "axis" if s < AXIS_BELOW else "generic", False))
    if kind[0] == "WELSCH":                      # rho' subnormal, rho' == 0
        out += [(730.0 * kind[1] ** 2, "axis", False), (760.0 * kind[1] ** 2, "axis", False)]
    if manifold == "so3":
        out = [t for t in out if t[0] < SO3_CUT]
    return out


def expected_count(kind, manifold):
    """edges per graph, from the grid alone"""
    return sum(2 if both else 1 for _, _, both in targets(kind, manifold)) + N_LOOPS


# ---- geometry ------------------------------------------------------------------------------------------------------------
def _spd(rng, D):
    """symmetric positive definite, eigenvalues in [0.5, 40]"""
    Q, R = np.linalg.qr(rng.standard_normal((D, D)))
    Q = Q * np.sign(np.diag(R))[None, :]
    W = (Q * np.exp(rng.uniform(np.log(0.5), np.log(40.0), D))[None, :]) @ Q.T
    return 0.5 * (W + W.T)


def _ident(man):
    return {"se3": np.array([0.0, 0, 0, 1, 0, 0, 0]), "se2": np.zeros(3), "so3": np.array([1.0, 0, 0, 0])}[man]


def _random_pose(rng, man):
    if man == "se2":
        return np.array([*rng.uniform(-3, 3, 2), rng.uniform(-3, 3)])
    q = mr._unit(rng, 1, 4)[0]
    return q if man == "so3" else np.concatenate([rng.uniform(-3, 3, 3), q])


def _exp_pose(man, tau):
    """Exp(tau) as a stored pose, long double in, fp64 out"""
    tau = np.asarray(tau, dtype=LD)[None]
    if man == "se3":
        return mr.se3_plus(_ident(man)[None], tau)[0]
    if man == "se2":
        return mr.se2_plus(np.zeros((1, 3)), tau)[0]
    return sr.so3_exp(tau)[0]


def _axis_edge(man, d, scale, in_meas):
    """identity rotations, the residual scale * d (d over the exact axes: translations, SO3: the rotation vector)"""
    vec = (LD(scale) * np.asarray(d, dtype=LD))
    carrier = _ident(man).copy()
    if man == "so3":
        carrier = _exp_pose(man, vec).astype(np.float64)
    else:
        carrier[:len(vec)] = vec.astype(np.float64)
    return (_ident(man), _ident(man), carrier) if in_meas else (carrier, _ident(man), _ident(man))


def _generic_edge(rng, man, tau, loop):
    """random poses with (k1^-1 k0) meas = Exp(tau) up to the rounding of the stored measurement"""
    if loop:
        k = _random_pose(rng, man)
        return k, k.copy(), np.asarray(_exp_pose(man, tau)).astype(np.float64)
    if man == "se2":
        k1, m = _random_pose(rng, man), _random_pose(rng, man)
        K0 = mr._se2_mat(k1) @ mr._se2_mat(mr.se2_plus(np.zeros(3), np.asarray(tau, dtype=LD)[None])) @ mr._se2_inv(mr._se2_mat(m))
        return np.array([K0[0, 0, 2], K0[0, 1, 2], np.arctan2(K0[0, 1, 0], K0[0, 0, 0])], dtype=np.float64), k1, m
    k0, k1 = _random_pose(rng, man), _random_pose(rng, man)
    if man == "so3":
        q0, q1 = sr.so3_from_vec(k0), sr.so3_from_vec(k1)
        qm = mr._qmul(mr._qmul(mr._qconj(q0), q1), sr.so3_exp(np.asarray(tau, dtype=LD)[None]))
        return k0, k1, qm[0].astype(np.float64)
    (t0, q0), (t1, q1) = mr.se3_from_vec(k0), mr.se3_from_vec(k1)
    tI, qI = mr._mul(*mr._inv(t0, q0), t1, q1)              # (k1^-1 k0)^-1
    m = mr.se3_plus(np.concatenate([tI, qI], -1), np.asarray(tau, dtype=LD)[None])
    return k0, k1, m[0].astype(np.float64)


def _tangent(rng, man, s, W):
    """tau with tau^T W tau = s (long double) and its rotational part below 2.5 rad"""
    D = DOF[man]
    u = mr._unit(rng, 1, D)[0].astype(LD)
    rot = {"se3": slice(3, 6), "se2": slice(2, 3), "so3": slice(0, 0)}[man]
    Wl = np.asarray(W, dtype=LD)
    while True:
        tau = u * np.sqrt(LD(s) / (u @ Wl @ u))
        if float(np.sqrt((tau[rot] * tau[rot]).sum())) <= 2.5:
            return tau
        u[rot] = u[rot] / 2


_AXES1 = {"se3": ((0,), (1,), (2,)), "se2": ((0,), (1,)), "so3": ((0,), (1,), (2,))}
_AXES2 = {"se3": ((0, 1), (1, 2), (0, 2)), "se2": ((0, 1),), "so3": ((0, 1), (1, 2), (0, 2))}


@functools.lru_cache(maxsize=None)
def cases(manifold, kind, policy):
    """The graph of one (manifold, kind, policy): SimpleNamespace of k0, k1, meas (n, amb), e_from, e_to, poses, info (n, D, D) |
    None, target (n,), family, loop (n,) bool, label, a, b (n, 2 D): the Gram vectors of each edge's pair.  Deterministic."""
    man, D = manifold, DOF[manifold]
    rng = np.random.default_rng(1000 * MANIFOLDS.index(man) + 10 * KINDS.index(kind) + POLICIES.index(policy))
    weighted = policy == "weighted"
    k0s, k1s, ms, Ws, tg, fam, lab, loop = [], [], [], [], [], [], [], []

    def add(trip, W, s, family, label, is_loop=False):
        k0s.append(np.asarray(trip[0], dtype=np.float64)); k1s.append(np.asarray(trip[1], dtype=np.float64))
        ms.append(np.asarray(trip[2], dtype=np.float64)); Ws.append(W); tg.append(s); fam.append(family); lab.append(label); loop.append(is_loop)

    count = 0
    for s, family, both in targets(kind, man):
        if family == "generic":
            W = _spd(rng, D) if weighted else np.eye(D)
            add(_generic_edge(rng, man, _tangent(rng, man, s, W), False), W, s, family, f"generic s={s:.17g}")
            continue
        forms = (1, 2) if both else ((1,) if s == EPS else (1 + count % 2,))
        for form in forms:
            count += 1
            W = _spd(rng, D) if weighted else np.eye(D)
            if s == EPS:                     # exactly: x = 2^-26, or under Omega x^2 W_00 = 2^-52 with W_00 = 4, x = 2^-27
                axes = (0,)
                if weighted:
                    W = W * (4.0 / W[0, 0])
                    W[0, 0] = 4.0
            else:
                axes = (_AXES1 if form == 1 else _AXES2)[man]
                axes = axes[count % len(axes)]
            d = np.zeros(3 if man != "se2" else 2)
            d[list(axes)] = (1.0,) if form == 1 else (0.8, 0.6)
            dd = np.zeros(D, dtype=LD); dd[:len(d)] = d
            Wl = W.astype(LD)
            scale = np.sqrt(LD(s) / (dd @ Wl @ dd))
            add(_axis_edge(man, d, scale, in_meas=count % 3 == 0), W, s, "axis", f"axis{axes} s={s:.17g}")
    for s in LOOP_S:
        W = _spd(rng, D) if weighted else np.eye(D)
        add(_generic_edge(rng, man, _tangent(rng, man, s, W), True), W, s, "loop", f"self-loop s={s:g}", True)
    n = len(tg)
    loop = np.array(loop)
    n_pair = int((~loop).sum())
    assert loop[n_pair:].all()
    e = np.arange(n_pair)
    flip = e % 2 == 1
    ef = np.concatenate([np.where(flip, 2 * e + 1, 2 * e), 2 * n_pair + np.arange(N_LOOPS)]).astype(np.uint32)
    et = np.concatenate([np.where(flip, 2 * e, 2 * e + 1), 2 * n_pair + np.arange(N_LOOPS)]).astype(np.uint32)
    k0, k1, meas = np.array(k0s), np.array(k1s), np.array(ms)
    poses = np.zeros((2 * n_pair + N_LOOPS, AMB[man]))
    poses[ef] = k0
    poses[et[:n_pair]] = k1[:n_pair]
    ab = rng.standard_normal((2, n, 2 * D))
    ab[:, loop, D:] = ab[:, loop, :D]                     # one vertex: one set of columns
    return SimpleNamespace(manifold=man, kind=kind, policy=policy, loss=mk(kind), n=n, D=D, k0=k0, k1=k1, meas=meas, e_from=ef, e_to=et,
                           poses=poses, info=np.array(Ws) if weighted else None, target=np.array(tg), family=fam, loop=loop, label=lab,
                           a=ab[0], b=ab[1])


def graph_of(cs, keep=None):
    """PoseGraphData of the cases (keep: an index array, the sub-graph of those edges with its own vertex numbering) and the
    information matrices that go with it"""
    from apex_solver_amd.synthetic import PoseGraphData

    if keep is None:
        d = PoseGraphData(ids=np.arange(len(cs.poses), dtype=np.int64), poses=cs.poses.copy(), e_from=cs.e_from.copy(), e_to=cs.e_to.copy(),
                          meas=cs.meas.copy())
        return d, cs.info
    keep = np.asarray(keep)
    verts = np.unique(np.concatenate([cs.e_from[keep], cs.e_to[keep]]))
    new = np.full(len(cs.poses), -1); new[verts] = np.arange(len(verts))
    d = PoseGraphData(ids=np.arange(len(verts), dtype=np.int64), poses=cs.poses[verts].copy(), e_from=new[cs.e_from[keep]].astype(np.uint32),
                      e_to=new[cs.e_to[keep]].astype(np.uint32), meas=cs.meas[keep].copy())
    return d, (None if cs.info is None else cs.info[keep].copy())


# ---- the long-double reference and the fp64 restatement --------------------------------------------------------------------
def _between_ld(man, k0, k1, m):
    return {"se3": mr.se3_between, "se2": mr.se2_between, "so3": sr.so3_between}[man](k0, k1, m)


def _q_to_R64(q):
    w, x, y, z = q
    return np.array([[w * w + x * x - y * y - z * z, 2 * (x * y - w * z), 2 * (x * z + w * y)],
                     [2 * (x * y + w * z), w * w - x * x + y * y - z * z, 2 * (y * z - w * x)],
                     [2 * (x * z - w * y), 2 * (y * z + w * x), w * w - x * x - y * y + z * z]])


def _qmul64(a, b):
    return np.array([a[0] * b[0] - a[1] * b[1] - a[2] * b[2] - a[3] * b[3], a[0] * b[1] + a[1] * b[0] + a[2] * b[3] - a[3] * b[2],
                     a[0] * b[2] - a[1] * b[3] + a[2] * b[0] + a[3] * b[1], a[0] * b[3] + a[1] * b[2] - a[2] * b[1] + a[3] * b[0]])


def so3_between_f64(k0, k1, m):
    """BetweenFactor<SO3>::linearize in fp64: numpy quaternion products around pg_oracle's so3_log and so3_left_jacobian_inv"""
    from oracle import pg_oracle as po

    nrm = lambda q: (lambda p: p / np.sqrt(p @ p))(q / np.sqrt(q @ q))
    conj = lambda q: q * np.array([1.0, -1, -1, -1])
    q0, q1, qm = nrm(k0), nrm(k1), nrm(m)
    qD = _qmul64(_qmul64(conj(q1), q0), qm)
    r = po.call("pgo_so3_log", qD, out_shape=3)
    Jr = po.call("pgo_so3_left_jacobian_inv", r, out_shape=9).reshape(3, 3).T
    return r, np.hstack([Jr @ _q_to_R64(qm).T, -(Jr @ _q_to_R64(qD).T)])


def _between_f64(man, k0, k1, m):
    n = len(k0)
    if man == "se2":
        return np_ref_se2.between_linearize(k0, k1, m)
    D = DOF[man]
    r = np.zeros((n, D)); J = np.zeros((n, D, 2 * D))
    if man == "se3":
        from oracle import pg_oracle as po
        for e in range(n):
            r[e], J[e] = po.between_linearize(k0[e], k1[e], m[e])
    else:
        for e in range(n):
            r[e], J[e] = so3_between_f64(k0[e], k1[e], m[e])
    return r, J


def _chol_upper_ld(W):
    n = len(W)
    A = np.asarray(W, dtype=LD)
    L = np.zeros((n, n), dtype=LD)
    for j in range(n):
        L[j, j] = np.sqrt(A[j, j] - L[j, :j] @ L[j, :j])
        L[j + 1:, j] = (A[j + 1:, j] - L[j + 1:, :j] @ L[j, :j]) / L[j, j]
    return L.T


def _edge_outputs(cs, e, rt, Jt, rh, Jh, W, cost, dt):
    """the outputs of edge e: exports (rt, Jt literal), and from (rh, Jh, W) the blocks in the form every backend reports:
    Haa (from), Hbb (to), Hx = J_to^T Omega J_from, ga, gb; a self-loop has everything on Haa, ga"""
    D = cs.D
    Ja, Jb = Jh[:, :D], Jh[:, D:]
    WJa, WJb, Wr = (Ja, Jb, rh) if W is None else (W @ Ja, W @ Jb, W @ rh)
    z = np.zeros((D, D), dtype=dt)
    if cs.loop[e]:
        Js = Ja + Jb
        WJs = Js if W is None else W @ Js
        H = (Js.T @ WJs, z, z); g = (Js.T @ Wr, np.zeros(D, dtype=dt))
    else:
        H = (Ja.T @ WJa, Jb.T @ WJb, Jb.T @ WJa); g = (Ja.T @ Wr, Jb.T @ Wr)
    u, w = Jh @ cs.a[e].astype(dt), Jh @ cs.b[e].astype(dt)
    Wu, Ww = (u, w) if W is None else (W @ u, W @ w)
    gram = np.array([u @ Wu, u @ Ww, w @ Ww], dtype=dt)
    return dict(r=rt, J=Jt, Haa=H[0], Hbb=H[1], Hx=H[2], ga=g[0], gb=g[1], gram=gram, cost=cost)


KEYS = ("r", "J", "Haa", "Hbb", "Hx", "ga", "gb", "gram", "cost")


def _stack(rows, dt):
    return {k: np.array([np.asarray(x[k], dtype=dt) for x in rows], dtype=dt) for k in KEYS}


@functools.lru_cache(maxsize=None)
def reference(manifold, kind, policy):
    """(ld, f64, meta): dicts of per-edge arrays (KEYS; cost: the term residual_scaling^2 s, the graph's cost is half their sum) in
    long double and in the fp64 restatement; meta: s (fp64 of the reference), arm, rho1 (exact zeros kept), kappa, jn = max(1, |J|max^2),
    arm64 and s64 of the restatement"""
    cs = cases(manifold, kind, policy)
    loss, D, n = cs.loss, cs.D, cs.n
    r, J = _between_ld(manifold, cs.k0, cs.k1, cs.meas)
    r64, J64 = _between_f64(manifold, cs.k0, cs.k1, cs.meas)
    rows, rows64 = [], []
    meta = dict(s=np.zeros(n), arm=np.zeros(n, int), rho1=np.zeros(n), kappa=np.ones(n), jn=np.ones(n), s64=np.zeros(n), arm64=np.zeros(n, int))
    for e in range(n):
        W = None if cs.info is None else cs.info[e].astype(LD)
        Wr = r[e] if W is None else W @ r[e]
        s = float(mr._dot(r[e], Wr))
        sq, rs, a, arm = nl.corrector(loss, s)
        rho = nl.evaluate(loss, s)
        rh = rs * r[e]
        Jh = sq * (J[e] - a * np.outer(r[e], Wr @ J[e])) if arm == 2 else sq * J[e]
        U = None if W is None else _chol_upper_ld(W)
        rt, Jt = (rh, Jh) if U is None else (U @ rh, U @ Jh)
        rows.append(_edge_outputs(cs, e, rt, Jt, rh, Jh, W, rs * rs * LD(s), LD))
        meta["s"][e], meta["arm"][e], meta["rho1"][e] = s, arm, float(rho[1])
        if float(rho[1]) > 0.0:
            meta["kappa"][e] = max(1.0, abs(float(LD(s) * rho[2] / rho[1])))
        meta["jn"][e] = max(1.0, float(np.abs(J[e]).max()) ** 2)
        # fp64: whiten, correct literally, multiply out (the whitened block closes with the identity)
        rw, Jw = (r64[e], J64[e]) if cs.info is None else (lambda w: (w[0][0], w[1][0]))(ni.whiten(r64[e:e + 1], J64[e:e + 1], cs.info[e:e + 1]))
        rt64, Jt64, arm64, s64 = nl.correct(rw, Jw, loss, dtype=np.float64)
        rows64.append(_edge_outputs(cs, e, rt64, Jt64, rt64, Jt64, None, rt64 @ rt64, np.float64))
        meta["s64"][e], meta["arm64"][e] = s64, arm64
    return _stack(rows, LD), _stack(rows64, np.float64), meta


# ---- the rule ------------------------------------------------------------------------------------------------------------
def err(x, ref):
    return mr.err(x, ref)


def lower_blocks(x):
    """diagonal blocks are held to their lower triangle (what the dense export stores)"""
    return np.tril(x)


OUTPUTS = (("r", ("r",), FLOOR_R, False), ("J", ("J",), FLOOR_J, True), ("H", ("Haa", "Hbb", "Hx"), FLOOR_J, True),
           ("g", ("ga", "gb"), FLOOR_J, True), ("gram", ("gram",), FLOOR_J, True))
BANDS = ((0.0, EPS), (EPS, 1e-6), (1e-6, 1e-2), (1e-2, 10.0), (10.0, np.inf))
BAND_NAMES = ("<eps", "eps..1e-6", "1e-6..1e-2", "1e-2..10", ">10")


def errors(got, ld, f64, meta):
    """per output name -> (e_got, e_f64, bound) per edge"""
    out = {}
    for name, keys, floor, by_j in OUTPUTS:
        eg = np.max([err(lower_blocks(got[k]) if k in ("Haa", "Hbb") else got[k], lower_blocks(ld[k]) if k in ("Haa", "Hbb") else ld[k]) for k in keys], axis=0)
        e64 = np.max([err(f64[k], ld[k]) for k in keys], axis=0)
        fl = floor * (meta["jn"] if by_j else 1.0) * meta["kappa"]
        out[name] = (eg, e64, np.maximum(8.0 * e64, fl))
    return out


def blocks_from_dense(cs, H, g, lam, col=None):
    """the per-edge blocks (Haa, Hbb, Hx, ga, gb of KEYS) read off a dense lower-triangular H + lam I and g, and the assertion that
    nothing lies outside the edges' blocks.  col: the first column of every vertex (None: vertex order, D v)"""
    D, n = cs.D, cs.n
    col = D * np.arange(len(cs.poses)) if col is None else np.asarray(col)
    H = np.array(H, dtype=np.float64)
    H[np.diag_indices_from(H)] -= lam
    out = dict(Haa=np.zeros((n, D, D)), Hbb=np.zeros((n, D, D)), Hx=np.zeros((n, D, D)), ga=np.zeros((n, D)), gb=np.zeros((n, D)))
    rest = np.tril(H)
    for e in range(n):
        f, t = int(cs.e_from[e]), int(cs.e_to[e])
        cf, ct = col[f] + np.arange(D), col[t] + np.arange(D)
        out["Haa"][e] = H[np.ix_(cf, cf)]; out["ga"][e] = g[cf]
        rest[np.ix_(cf, cf)] = 0.0
        if f != t:
            out["Hbb"][e] = H[np.ix_(ct, ct)]; out["gb"][e] = g[ct]
            out["Hx"][e] = H[np.ix_(ct, cf)] if ct[0] > cf[0] else H[np.ix_(cf, ct)].T
            rest[np.ix_(ct, ct)] = 0.0
            rest[np.ix_(max(cf[0], ct[0]) + np.arange(D), min(cf[0], ct[0]) + np.arange(D))] = 0.0
    assert not rest.any(), "H has entries outside the edges' blocks"
    return out


def cost_groups(ld):
    """index arrays: the edges whose reference cost term is exactly 0, then runs of the sorted positive terms within a factor 1e3"""
    t = ld["cost"].astype(np.float64)          # (a subnormal term stays what it is)
    tl = ld["cost"]
    zero = np.nonzero(tl == 0)[0]
    order = [i for i in np.argsort(tl) if tl[i] > 0]
    groups, cur = ([zero] if len(zero) else []), []
    for i in order:
        if cur and tl[i] > LD(1e3) * tl[cur[0]]:
            groups.append(np.array(cur)); cur = []
        cur.append(i)
    if cur:
        groups.append(np.array(cur))
    assert sum(len(g) for g in groups) == len(t)
    return groups


def cost_error(got, group, ld, f64, meta):
    """(e_got, e_f64, bound) of one sub-graph's cost"""
    ref = LD(0.5) * ld["cost"][group].sum()
    den = max(LD(1), abs(ref))
    eg = float(abs(LD(got) - ref) / den)
    e64 = float(abs(LD(0.5 * f64["cost"][group].sum()) - ref) / den)
    return eg, e64, max(8.0 * e64, FLOOR_R * float(meta["kappa"][group].max()))


def report(tag, meta, errs, cost_worst):
    """one LOSSEDGE line: per band of s, the worst e, e_f64 and ratio to the bound over the outputs"""
    parts = []
    worst = 0.0
    for i, name in enumerate(BAND_NAMES):
        lo, hi = BANDS[i]
        sel = (meta["s"] >= lo) & (meta["s"] < hi)
        if not sel.any():
            continue
        eg = max(float(v[0][sel].max()) for v in errs.values()); e64 = max(float(v[1][sel].max()) for v in errs.values())
        ratio = max(float((v[0][sel] / v[2][sel]).max()) for v in errs.values())
        worst = max(worst, ratio)
        parts.append(f"{name} n={int(sel.sum())} e={eg:.1e} e_f64={e64:.1e} ratio={ratio:.2f}")
    worst = max(worst, cost_worst)
    print(f"LOSSEDGE {tag}: " + " | ".join(parts) + f" | cost ratio={cost_worst:.2f} | worst ratio={worst:.2f}")
    return worst


def check(tag, cs, got, ld, f64, meta):
    """the rule on every edge and output of `got` (KEYS without cost); exact zeros where rho' == 0; returns the errors"""
    for k in KEYS[:-1]:
        assert np.isfinite(got[k]).all(), (tag, k)
    errs = errors(got, ld, f64, meta)
    for name, (eg, e64, bound) in errs.items():
        bad = np.nonzero(~(eg <= bound))[0]
        at = int(np.argmax(eg / bound))
        assert not len(bad), (tag, name, cs.label[at], "e", float(eg[at]), "e_f64", float(e64[at]), "bound", float(bound[at]),
                              "kappa", float(meta["kappa"][at]), "edges over", len(bad))
    for e in np.nonzero(meta["rho1"] == 0.0)[0]:
        for k in KEYS[:-1]:
            assert not np.asarray(got[k][e]).any(), (tag, "rho' == 0 but", k, "is not exactly zero", cs.label[e])
    return errs
