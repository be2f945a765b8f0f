"""The premises of tests/loss_edge_cases.py on the reference alone, and the same cases through the host builds of the device math
(tests/host_harness_loss.cpp, host_harness_info.cpp, host_harness_se3_row.cpp, host_harness_so3.cpp: g++ -ffp-contract=off) under
the rule the device test applies (tests/test_gpu_loss_edges.py).  No GPU needed: a formula error shows here before a
kernel-structure error has to be found on the device."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import loss_edge_cases as lc
import np_ref_loss as nl
from apex_solver_amd import capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_f = np.ctypeslib.ndpointer(dtype=np.float64, flags="C_CONTIGUOUS")
_u = np.ctypeslib.ndpointer(dtype=np.uint32, flags="C_CONTIGUOUS")
_i = np.ctypeslib.ndpointer(dtype=np.int32, flags="C_CONTIGUOUS")
EPS = nl.EPS
c = lambda x: np.ascontiguousarray(x, dtype=np.float64)
KIND_IDS = [lc.kind_id(k) for k in lc.KINDS]


def _build(name):
    out = os.path.join(ROOT, "tests", "_build")
    os.makedirs(out, exist_ok=True)
    so = os.path.join(out, f"lib{name}_edges.so")
    subprocess.run(["g++", "-O2", "-ffp-contract=off", "-std=c++17", "-shared", "-fPIC", "-I", os.path.join(ROOT, "apex-solver_amd", "csrc"),
                    os.path.join(ROOT, "tests", f"{name}.cpp"), "-o", so], check=True)
    return C.CDLL(so)


@pytest.fixture(scope="module")
def libs():
    hl, hi, h6, h3 = (_build(n) for n in ("host_harness_loss", "host_harness_info", "host_harness_se3_row", "host_harness_so3"))
    loss = [C.c_int, C.c_double, C.c_double]
    hl.hl_edge.argtypes = [C.c_int, _f, _f, _f] + loss + [_f, _f]
    hl.hl_blocks.argtypes = [C.c_int, _f, _f, _f] + loss + [C.c_int] + [_f] * 5
    hl.hl_jv.argtypes = [C.c_int, _f, _f, _f] + loss + [_f] * 6
    hl.hl_cost.argtypes = [C.c_int, _f, _f, _f] + loss + [_f]
    head = [C.c_int, _f, _f, _f] + loss + [_f]
    hi.hi_edge.argtypes = head + [_f, _f]
    hi.hi_blocks.argtypes = head + [C.c_int] + [_f] * 5
    hi.hi_jv.argtypes = head + [_f] * 5
    hi.hi_cost.argtypes = head + [_f]
    h6.hs6_assemble_dense.argtypes = [C.c_int64, C.c_int64, _f, _u, _u, _f, C.c_int, C.c_double, C.c_double, C.c_double, C.c_void_p,
                                      C.c_double, C.c_int64, _u, _f, _f, _f, _f, _i, _i, _f, _f, _f, _f]
    h3.hs3_assemble_dense.argtypes = [C.c_int64, C.c_int64, _f, _u, _u, _f, C.c_int, C.c_double, C.c_double, C.c_double, C.c_void_p, _f, _f, _i, _i]
    h3.hs3_edge.argtypes = [_f, _f, _f] + loss + [C.c_void_p, _f, _f]
    h3.hs3_jv.argtypes = [_f, _f, _f] + loss + [C.c_void_p] + [_f] * 5
    h3.hs3_cost.argtypes = [_f, _f, _f] + loss + [C.c_void_p, _f]
    return dict(hl=hl, hi=hi, h6=h6, h3=h3)


# ---- the premises -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", lc.KINDS, ids=KIND_IDS)
@pytest.mark.parametrize("man", lc.MANIFOLDS)
def test_premises_of_the_cases(man, kind):
    loss = lc.mk(kind)
    second = {p: 0 for p in (1, 2)}
    for policy in lc.POLICIES:
        cs = lc.cases(man, kind, policy)
        ld, f64, meta = lc.reference(man, kind, policy)
        assert cs.n == lc.expected_count(kind, man) == len(cs.label)                  # no case skipped or filtered anywhere
        assert len(cs.poses) == 2 * (cs.n - lc.N_LOOPS) + lc.N_LOOPS <= 200 and cs.loop.sum() == lc.N_LOOPS
        if man == "so3":
            assert cs.target.max() < lc.SO3_CUT
        for k in lc.KEYS:
            assert np.isfinite(ld[k].astype(np.float64)).all() and np.isfinite(f64[k]).all(), k
        if cs.info is not None:
            assert max(np.linalg.cond(W) for W in cs.info) <= 100.0 and all(np.array_equal(W, W.T) for W in cs.info)
        # every target is hit on the intended side
        s, t = meta["s"], cs.target
        exact = t == EPS
        assert exact.sum() == 1 and (s[exact] == EPS).all()                           # at the threshold itself: to the bit
        assert (s[t == 0.0] == 0.0).all() and (t == 0.0).sum() == 2
        axis = np.array([f == "axis" for f in cs.family])
        # an ulp, or a few through SO3's log -- whose small-angle forms (Exp as (1, theta / 2) normalised, Log as 2 qv below
        # theta^2 = 1e-10) are first order: they move s by |r|^2 / 4 of itself at most, |r|^2 <= s / lambda_min(Omega) <= 2 s: 2e-10 where they apply
        assert (np.abs(s[axis] - t[axis]) <= (1e-14 + (0.52 * t[axis] if man == "so3" else 0.0)) * t[axis]).all()
        generic = ~axis & (t > 0)
        assert (np.abs(s[generic] - t[generic]) <= 1e-9 * t[generic]).all()
        for th in nl.thresholds(loss):
            slow = loss.kind in (capi.LOSS_TUKEY, capi.LOSS_ANDREWS)                      # through sqrt and sin: see s_grid
            margin = np.abs(s[~exact] - th) / th
            # (the grid's own points t (1 -+ 1e-4) and EPS (1 -+ 1e-9) are fp64 roundings: EPS (1 - 1e-9) lies 0.99999975e-9 from EPS)
            assert margin.min() >= (0.99e-4 if slow else 0.999999e-9), (policy, th, margin.min())
            assert ((s[~exact] > th) == (t[~exact] > th)).all()
        assert all(f == "axis" for f, tt in zip(cs.family, t) if tt < lc.AXIS_BELOW and f != "loop")
        # the two arithmetics take the same arm at the same side of every branch
        assert np.array_equal(meta["arm"], meta["arm64"]), np.nonzero(meta["arm"] != meta["arm64"])[0]
        assert ((meta["s64"] == 0.0) == (s == 0.0)).all()
        for th in nl.thresholds(loss):
            assert ((meta["s64"] > th) == (s > th))[~exact].all() and ((meta["s64"] >= th) == (s >= th))[exact].all()
        rho1_64 = np.array([float(nl.evaluate(loss, x, dtype=np.float64)[1]) for x in meta["s64"]])
        assert ((rho1_64 == 0.0) == (meta["rho1"] == 0.0)).all()
        for arm in (1, 2):
            second[arm] += int((meta["arm"] == arm).sum())
        if kind in lc.SECOND_ARM:
            assert (meta["arm"] == 1).sum() >= 10 and (meta["arm"] == 2).sum() >= 10, policy
        if kind[0] in lc.REDESCENDING:
            assert (meta["rho1"] == 0.0).sum() >= 1 and (meta["rho1"] > 0.0).sum() >= 1
        if kind == ("WELSCH", 0.1, 0):
            tiny = np.finfo(np.float64).tiny
            assert (meta["rho1"] == 0.0).sum() >= 1 and ((meta["rho1"] > 0.0) & (meta["rho1"] < tiny)).sum() >= 1
        if kind == ("BARRON", 3.0, 1.0):
            assert ((meta["arm"] == 2) == (s > 0.0)).all()
        # the restatement is a reference for fp64 code: it is itself within the floors, up to the conditioning the rule names
        errs = lc.errors(f64, ld, f64, meta)
        for name, (_, e64, _) in errs.items():
            floor = {"r": lc.FLOOR_R}.get(name, lc.FLOOR_J)
            assert (e64 <= 8.0 * floor * meta["kappa"] * (1.0 if name == "r" else meta["jn"])).all(), (policy, name, float(e64.max()))
    if kind[0] in ("NONE", "L2"):
        assert second[2] == 0


# ---- the host builds of the device forms under the rule ---------------------------------------------------------------------
def _per_edge(libs, path, cs):
    """r, J, gram, cost of every edge (every path), blocks of the paths that have a per-edge form"""
    n, D, loss = cs.n, cs.D, cs.loss
    man = {"se3": 0, "se3-row": 0, "se2": 1}.get(path)
    got = dict(r=np.zeros((n, D)), J=np.zeros((n, D, 2 * D)), gram=np.zeros((n, 3)), cost=np.zeros(n), Haa=np.zeros((n, D, D)), Hbb=np.zeros((n, D, D)),
               Hx=np.zeros((n, D, D)), ga=np.zeros((n, D)), gb=np.zeros((n, D)))
    lp = (loss.kind, loss.p0, loss.p1)
    for e in range(n):
        k0, k1, m = c(cs.k0[e]), c(cs.k1[e]), c(cs.meas[e])
        a0, a1, b0, b1 = c(cs.a[e, :D]), c(cs.a[e, D:]), c(cs.b[e, :D]), c(cs.b[e, D:])
        W = None if cs.info is None else c(cs.info[e])
        order = 2 if cs.loop[e] else int(cs.e_from[e] > cs.e_to[e])
        cost = np.zeros(1)
        if path == "so3":
            wp = None if W is None else W.ctypes.data_as(C.c_void_p)
            assert libs["h3"].hs3_edge(k0, k1, m, *lp, wp, got["r"][e], got["J"][e]) == 0
            assert libs["h3"].hs3_jv(k0, k1, m, *lp, wp, a0, a1, b0, b1, got["gram"][e]) == 0
            assert libs["h3"].hs3_cost(k0, k1, m, *lp, wp, cost) == 0
        elif W is None:
            hl = libs["hl"]
            u, w = np.zeros(D), np.zeros(D)
            assert hl.hl_edge(man, k0, k1, m, *lp, got["r"][e], got["J"][e]) == 0
            assert hl.hl_blocks(man, k0, k1, m, *lp, int(cs.loop[e]), got["Haa"][e], got["Hbb"][e], got["Hx"][e], got["ga"][e], got["gb"][e]) == 0
            assert hl.hl_jv(man, k0, k1, m, *lp, a0, a1, b0, b1, u, w) == 0
            got["gram"][e] = (u @ u, u @ w, w @ w)
            assert hl.hl_cost(man, k0, k1, m, *lp, cost) == 0
        else:
            hi = libs["hi"]
            assert hi.hi_edge(man, k0, k1, m, *lp, W, got["r"][e], got["J"][e]) == 0
            assert hi.hi_blocks(man, k0, k1, m, *lp, W, order, got["Haa"][e], got["Hbb"][e], got["Hx"][e], got["ga"][e], got["gb"][e]) == 0
            if order == 1:
                got["Hx"][e] = got["Hx"][e].T.copy()
            assert hi.hi_jv(man, k0, k1, m, *lp, W, a0, a1, b0, b1, got["gram"][e]) == 0
            assert hi.hi_cost(man, k0, k1, m, *lp, W, cost) == 0
        got["cost"][e] = cost[0]
    return got


def _dense(libs, path, cs, kind=None, delta=-1.0):
    """(H, g, r, J) of the whole graph by the row-owned host loops; kind None: the cases' loss, else the legacy delta form"""
    loss = cs.loss
    lp = (loss.kind, loss.p0, loss.p1) if kind is None else (kind, 0.0, 0.0)
    nv, n, D = len(cs.poses), cs.n, cs.D
    H = np.zeros((D * nv, D * nv)); g = np.zeros(D * nv)
    writes = np.zeros((nv, nv), np.int32); writer = np.full((nv, nv), -1, np.int32)
    keep = None if cs.info is None else c(cs.info)
    ip = None if keep is None else keep.ctypes.data_as(C.c_void_p)
    if path == "so3":
        assert libs["h3"].hs3_assemble_dense(nv, n, c(cs.poses), cs.e_from, cs.e_to, c(cs.meas), *lp, delta, ip, H, g, writes, writer) == 0
        return H, g, None, None, 0.0
    r = np.zeros((n, 6)); J = np.zeros((n, 6, 12))
    z = np.zeros(0)
    rc = libs["h6"].hs6_assemble_dense(nv, n, c(cs.poses), cs.e_from, cs.e_to, c(cs.meas), *lp, delta, ip, lc.LAMBDA, 0, np.zeros(0, np.uint32),
                                       z, z, H, g, writes, writer, r, J, z, z)
    assert rc >= 0
    return H, g, r, J, lc.LAMBDA


@pytest.mark.parametrize("kind", lc.KINDS, ids=KIND_IDS)
@pytest.mark.parametrize("path", ["se3", "se3-row", "se2", "so3"])
def test_host_forms_meet_the_rule_on_every_edge(libs, path, kind):
    man = path.split("-")[0]
    worst = {}
    for policy in lc.POLICIES:
        cs = lc.cases(man, kind, policy)
        ld, f64, meta = lc.reference(man, kind, policy)
        got = _per_edge(libs, path, cs)
        if path in ("se3-row", "so3"):
            H, g, r, J, lam = _dense(libs, path, cs)
            got.update(lc.blocks_from_dense(cs, H, g, lam))
            if r is not None:
                assert np.array_equal(r, got["r"]) and np.array_equal(J, got["J"])
        tag = f"{path} {lc.kind_id(kind)} {policy} (host)"
        errs = lc.check(tag, cs, got, ld, f64, meta)
        cw = 0.0
        for grp in lc.cost_groups(ld):
            eg, e64, bound = lc.cost_error(0.5 * got["cost"][grp].sum(), grp, ld, f64, meta)
            assert eg <= bound, (tag, "cost of the sub-graph", [cs.label[i] for i in grp[:3]], eg, e64, bound)
            if (meta["rho1"][grp] == 0.0).all() or (meta["s"][grp] == 0.0).all():
                assert not got["cost"][grp].any()
            cw = max(cw, eg / bound)
        worst[policy] = lc.report(tag, meta, errs, cw)
    assert all(np.isfinite(v) for v in worst.values())


@pytest.mark.parametrize("path", ["se3-row", "so3"])
def test_huber_through_the_loss_is_the_legacy_delta_on_the_host(libs, path):
    """the general path under Huber against set_structure's huber_delta: the same bits in every block and row"""
    kind = next(k for k in lc.KINDS if k[0] == "HUBER")
    cs = lc.cases(path.split("-")[0], kind, "general")
    a = _dense(libs, path, cs)
    b = _dense(libs, path, cs, kind=capi.LOSS_NONE, delta=kind[1])
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])
    if a[2] is not None:
        assert np.array_equal(a[2], b[2]) and np.array_equal(a[3], b[3])
    assert a[0].any()
