"""The row-owned SE3 assembly (pg_row_assemble6 of apex-solver_amd/csrc/pg_device.hpp, the loop of k_pg6_assemble behind the
option "row_owned_assembly") compiled for the host and replayed over build_incident_lists on every SE3 crafted graph of
tests/pg_asm_cases.py, under the three loss policies, against the long double reference of tests/pg_asm_ref.py: D x D block by
block and vertex row by vertex row with the block rule err <= max(8 e_np, gamma(P + c0(6, policy)) M), as
tests/test_gpu_pg_crafted.py applies it on the device.  No GPU needed.

The row function forms every product as k_pg_edges / pg_edge_weighted form it, so the rounding chains counted in c0 hold as
they stand; what is on trial is where the products go and in which order they are summed."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import pg_asm_cases as pc
import pg_asm_ref as pr
from apex_solver_amd import capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_f = np.ctypeslib.ndpointer(dtype=np.float64, flags="C_CONTIGUOUS")
_u = np.ctypeslib.ndpointer(dtype=np.uint32, flags="C_CONTIGUOUS")
_i = np.ctypeslib.ndpointer(dtype=np.int32, flags="C_CONTIGUOUS")
POLICY_ID = {"legacy": 0, "general": 1, "weighted": 2}
RUNS = [(n, p) for n, p, m in pc.all_runs() if m == "se3"]


def load_harness():
    out = os.path.join(ROOT, "tests", "_build")
    os.makedirs(out, exist_ok=True)
    so = os.path.join(out, "libhost_harness_se3_row.so")
    subprocess.run(["g++", "-O2", "-ffp-contract=off", "-std=c++17", "-shared", "-fPIC",
                    "-I", os.path.join(ROOT, "apex-solver_amd", "csrc"),
                    os.path.join(ROOT, "tests", "host_harness_se3_row.cpp"), "-o", so], check=True)
    L = C.CDLL(so)
    L.hs6_assemble_dense.argtypes = [C.c_int64, C.c_int64, _f, _u, _u, _f, C.c_int, C.c_double, C.c_double, C.c_double, C.c_void_p,
                                     C.c_double, C.c_int64, _u, _f, _f, _f, _f, _i, _i, _f, _f, _f, _f]
    L.hs6_incident.argtypes = [C.c_int64, C.c_int64, _u, _u, C.c_int64, _u]; L.hs6_incident.restype = C.c_int64
    return L


@pytest.fixture(scope="module")
def hh():
    return load_harness()


def c(a):
    return np.ascontiguousarray(a, dtype=np.float64)


def assemble(hh, prob, lam, relabel=None):
    """The harness on a PoseGraphProblem; relabel: a permutation of the vertices (new index of every vertex) applied first."""
    d = prob.data
    n_v, n_e = d.n_v, d.n_e
    new = np.arange(n_v) if relabel is None else np.asarray(relabel)
    poses = np.zeros((n_v, 7)); poses[new] = d.poses
    ef = np.ascontiguousarray(new[d.e_from.astype(np.int64)], np.uint32); et = np.ascontiguousarray(new[d.e_to.astype(np.int64)], np.uint32)
    loss = prob.loss
    kind, p0, p1 = (capi.LOSS_NONE, 0.0, 0.0) if loss is None else (int(loss.kind), float(loss.p0), float(loss.p1))
    delta = -1.0 if prob.huber_delta is None else float(prob.huber_delta)
    keep = None if prob.information is None else c(prob.information)
    ip = None if keep is None else keep.ctypes.data_as(C.c_void_p)
    pri = prob.priors
    pv = np.ascontiguousarray(new[[q[0] for q in pri]] if pri else [], np.uint32)
    pd = c([q[1] for q in pri]).reshape(-1, 7) if pri else np.zeros((0, 7))
    pdl = c([-1.0 if q[2] is None else q[2] for q in pri]) if pri else np.zeros(0)
    n = 6 * n_v
    H = np.zeros((n, n)); g = np.zeros(n)
    writes = np.zeros((n_v, n_v), np.int32); writer = np.full((n_v, n_v), -1, np.int32)
    r = np.zeros((n_e, 6)); J = np.zeros((n_e, 6, 12)); pres = np.zeros((len(pv), 7)); psc = np.zeros(len(pv))
    rc = hh.hs6_assemble_dense(n_v, n_e, c(poses), ef, et, c(d.meas), kind, p0, p1, delta, ip, lam, len(pv), pv, pd, pdl,
                               H, g, writes, writer, r, J, pres, psc)
    return SimpleRun(rc, H, g, writes, writer, r, J, pres, psc, ef, et)


class SimpleRun:
    def __init__(self, rc, H, g, writes, writer, r, J, pres, psc, ef, et):
        self.rc, self.H, self.g, self.writes, self.writer, self.r, self.J, self.pres, self.psc, self.ef, self.et = rc, H, g, writes, writer, r, J, pres, psc, ef, et

    def blocks(self):
        """(n_v, n_v, 6, 6) with the lower triangle mirrored, as the handle's export mirrors the tiles"""
        Hs = np.tril(self.H) + np.tril(self.H, -1).T
        n_v = len(self.writes)
        return np.ascontiguousarray(Hs.reshape(n_v, 6, n_v, 6).transpose(0, 2, 1, 3))


@pytest.mark.parametrize("name,pol", RUNS, ids=[f"{n}-{p}" for n, p in RUNS])
def test_row_function_on_crafted_graph(hh, name, pol):
    cse, p = pc.build(name, "se3"), pc.policy(name, "se3", pol)
    lam = pc.LAM
    run = assemble(hh, p.prob, lam)
    assert run.rc == POLICY_ID[p.kernel]                                      # the policy that was asked for is the one that ran
    nb = pc.numpy_blocks(name, "se3", pol)
    assert np.abs(run.r - nb.r).max() <= 1e-9 * max(1.0, np.abs(nb.r).max()) and np.abs(run.J - nb.J).max() <= 1e-9 * max(1.0, np.abs(nb.J).max())
    priors = None
    if cse.priors:
        pv, pres_np, psc_np = pc.numpy_blocks(name, "se3", "none").priors
        assert np.abs(run.pres - pres_np).max() <= 1e-13 and np.abs(run.psc - psc_np).max() <= 1e-13
        priors = (pv, run.pres, psc_np)
    ld, f64 = pc.reference(name, "se3", pol, run.J, run.r, priors, lam)
    C0 = pr.c0(6, p.kernel)
    H4 = run.blocks()
    ratios, bad, stray = pr.h_check(H4, ld, f64, C0)
    ratios["g"] = pr.g_check(run.g.reshape(-1, 6), ld, f64, C0)
    pr.report(f"host-row {name}-{pol}-se3", ratios)
    assert not bad, [(t, int(ld.P_d[t[1]])) for t in bad[:8]]
    assert stray == 0                                                         # pairs without an edge are exactly 0
    assert pr.worst(ratios["g"])[0] <= 1.0, pr.worst(ratios["g"])
    quiet = np.nonzero(~ld.touched)[0]
    assert (H4[quiet, quiet] == lam * np.eye(6)).all() and not run.g.reshape(-1, 6)[ld.P_g == 0].any()
    if name == "isolated":
        assert set(cse.facts.isolated) <= set(quiet.tolist())
    if name == "straddle" and pol == "tukey":
        assert cse.facts.rejected_vertex in quiet and (~ld.mags["live"]).any()
    # placement: only blocks (v, u) with u < v are written, by the owner of row v, once per live edge between the pair
    ef, et = run.ef.astype(int), run.et.astype(int)
    want = np.zeros_like(run.writes)
    for e in np.nonzero(ld.mags["live"] & (ef != et))[0]:
        want[max(ef[e], et[e]), min(ef[e], et[e])] += 1
    assert np.array_equal(run.writes, want) and np.count_nonzero(np.triu(run.writes)) == 0
    vs, us = np.nonzero(run.writes)
    assert np.array_equal(run.writer[vs, us], vs)
    assert np.count_nonzero(np.triu(run.H, 1) * (1 - np.kron(np.eye(len(want)), np.ones((6, 6))))) == 0   # nothing above the diagonal blocks
    # a second pass gives the same bits: every sum has a fixed order
    again = assemble(hh, p.prob, lam)
    assert np.array_equal(run.H, again.H) and np.array_equal(run.g, again.g)


def _list_order_sum(terms):
    acc = np.zeros_like(terms[0])
    for t in terms:
        acc = acc + t
    return acc


def test_parallel_edges_and_self_loops_sum_in_list_order(hh):
    """The 257 parallel edges: the block of their pair is the fp64 sum of J~_hi^T J~_lo over the owner's incident list, in that
    order (the factors differ by the linearisation's own rounding, the order does not).  The three self-loops of one vertex:
    G_00 + G_11 + G_01 + G_01^T each, between the vertex's chain edges, in list order."""
    p = pc.policy("multi", "se3", "huber")
    cse = pc.build("multi", "se3")
    run = assemble(hh, p.prob, 0.0)
    ef, et = run.ef, run.et
    a, b, P = cse.facts.pairs[-1]
    assert P == 257 and b > a
    out = np.zeros(2 * len(ef), np.uint32)
    n = hh.hs6_incident(cse.d.n_v, cse.d.n_e, ef, et, b, out)
    lst = out[:n].astype(int)
    between = [e for e in lst if {int(ef[e]), int(et[e])} == {a, b}]
    assert len(between) == 257 and np.all(np.diff(lst) > 0) and n == 257 + 2      # its two chain edges and the 257, ascending
    Jb = lambda e, v: run.J[e][:, :6] if ef[e] == v else run.J[e][:, 6:]
    acc = _list_order_sum([Jb(e, b).T @ Jb(e, a) for e in between])
    blk = run.H[6 * b:6 * b + 6, 6 * a:6 * a + 6]
    assert np.abs(blk - acc).max() < 1e-12 * np.abs(acc).max()
    dg = _list_order_sum([Jb(e, b).T @ Jb(e, b) for e in lst])
    assert np.abs(np.tril(run.H[6 * b:6 * b + 6, 6 * b:6 * b + 6]) - np.tril(dg)).max() < 1e-12 * np.abs(dg).max()
    assert np.abs(run.g[6 * b:6 * b + 6] - _list_order_sum([Jb(e, b).T @ run.r[e] for e in lst])).max() < 1e-12 * np.abs(run.g).max()

    p = pc.policy("loops", "se3", "huber")
    cse = pc.build("loops", "se3")
    run = assemble(hh, p.prob, 0.0)
    ef, et = run.ef, run.et
    for v in (cse.facts.lonely, cse.facts.triple, cse.facts.tile_end):
        n = hh.hs6_incident(cse.d.n_v, cse.d.n_e, ef, et, v, out)
        lst = out[:n].astype(int)
        loops = [e for e in lst if ef[e] == et[e]]
        assert len(loops) == (3 if v == cse.facts.triple else 1) and len(set(lst.tolist())) == n      # a self-loop is listed once
        terms, gt = [], []
        for e in lst:
            J0, J1 = run.J[e][:, :6], run.J[e][:, 6:]
            if ef[e] == et[e]:
                G = J0.T @ J1
                terms += [J0.T @ J0, J1.T @ J1, G + G.T]; gt += [J0.T @ run.r[e], J1.T @ run.r[e]]
            else:
                Jv = J0 if ef[e] == v else J1
                terms.append(Jv.T @ Jv); gt.append(Jv.T @ run.r[e])
        # (on a self-loop J~_1 = -J~_0, so its four terms cancel: the scale is that of the terms, not of their sum)
        dg, mag = _list_order_sum(terms), _list_order_sum([np.abs(t) for t in terms]).max()
        assert np.abs(np.tril(run.H[6 * v:6 * v + 6, 6 * v:6 * v + 6]) - np.tril(dg)).max() < 1e-12 * mag
        assert np.abs(run.g[6 * v:6 * v + 6] - _list_order_sum(gt)).max() < 1e-12 * _list_order_sum([np.abs(t) for t in gt]).max()


@pytest.mark.parametrize("name", ["straddle", "loops", "hub_hi"])
def test_weighted_cross_block_is_the_transpose_of_the_other_rows(hh, name):
    """G_vu = J_v^T Omega J_u is not symmetric in (v, u).  With the vertices numbered backwards the owner of every pair is its
    other endpoint, which forms J_u^T Omega J_v for (u, v): the transpose of the block formed here, to the rounding of the block
    rule on both sides -- and not the block itself."""
    p = pc.policy(name, "se3", "weighted")
    n_v = p.prob.data.n_v
    run = assemble(hh, p.prob, 0.0)
    back = assemble(hh, p.prob, 0.0, relabel=n_v - 1 - np.arange(n_v))
    assert run.rc == back.rc == 2
    ld, f64 = pc.reference(name, "se3", "weighted", run.J, run.r, None, 0.0)
    bound = 2.0 * pr.gamma(ld.P_o, pr.c0(6, "weighted")) * ld.M_o
    far = 0
    for k, (v, u) in enumerate(ld.pairs):
        mine = run.H[6 * v:6 * v + 6, 6 * u:6 * u + 6]
        rv, ru = n_v - 1 - v, n_v - 1 - u                                       # ru > rv: row ru owns the pair there
        theirs = back.H[6 * ru:6 * ru + 6, 6 * rv:6 * rv + 6]
        assert back.writer[ru, rv] == ru and run.writer[v, u] == v
        assert np.abs(mine - theirs.T).max() <= bound[k], (v, u)
        far += np.abs(mine - theirs).max() > 1e-3 * np.abs(mine).max()
    assert len(ld.pairs) > 0 and far >= 0.9 * len(ld.pairs)


def test_the_harness_runs_as_a_program_of_its_own(tmp_path):
    """-DHS6_MAIN: the same file with its own main (the form a sanitizer build takes); here built plainly and run once."""
    exe = str(tmp_path / "hs6_main")
    subprocess.run(["g++", "-O1", "-ffp-contract=off", "-std=c++17", "-DHS6_MAIN", "-I", os.path.join(ROOT, "apex-solver_amd", "csrc"),
                    os.path.join(ROOT, "tests", "host_harness_se3_row.cpp"), "-o", exe], check=True)
    out = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert out.returncode == 0 and out.stdout.strip() == "ok", (out.stdout[-500:], out.stderr[-500:])
