"""tests/pg_asm_ref.py and tests/pg_asm_cases.py on the CPU: the reference against the references the project already has (the
pose-graph oracle, np_ref_pg / np_ref_se2 / np_ref_info, with inputs those produce themselves), the premises of every crafted
case on its lists, the fp64 restatement alone inside the bound with the referee arm switched off, and the placement mutations:
each is flagged on a named case and attributed to the right blocks.  tests/test_gpu_pg_crafted.py runs the cases on the device."""
import os
import subprocess

import numpy as np
import pytest

import np_ref_info as ni
import np_ref_loss as nl
import pg_asm_cases as pc
import pg_asm_ref as pr
from oracle import pg_oracle as po

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "apex-solver_amd", "csrc")
MANIFOLDS = ["se3", "se2"]
CASES = list(pc.POLICIES)


def _ref(name, man, pol, lam=pc.LAM):
    nb = pc.numpy_blocks(name, man, pol)
    return nb, pc.reference(name, man, pol, nb.J, nb.r, nb.priors, lam)


def _c0(name, man, pol):
    return pr.c0(pc.DOF[man], pc.policy(name, man, pol).kernel)


# ---- 1. the reference against the existing references ---------------------------------------------------------------------------
@pytest.mark.parametrize("name,pol", [("straddle", "none"), ("loops", "huber"), ("priors_run", "none")])
def test_against_the_oracle_se3(name, pol):
    p = pc.policy(name, "se3", pol)
    o = po.PgOracle.from_problem(p.prob)
    cost, r, J = o.linearize()
    Ho, go = o.normal_equations()
    nb = pc.numpy_blocks(name, "se3", pol)
    priors = None if nb.priors is None else (nb.priors[0], o.prior_residuals(), nb.priors[2])
    ld, f64 = pc.reference(name, "se3", pol, J, r, priors, lam=0.0)
    C0 = _c0(name, "se3", pol)
    ratios, bad, stray = pr.h_check(pr.blocks_of(Ho, p.prob.pose_col, 6), ld, f64, C0)
    assert not bad and stray == 0, bad[:5]
    assert pr.g_check(pr.rows_of(go, p.prob.pose_col, 6), ld, f64, C0).max() <= 1.0
    assert pr.scalar_check(cost, ld.cost, f64.cost, ld.M_cost, ld.n_terms, C0).max() <= 1.0


@pytest.mark.parametrize("man", MANIFOLDS)
@pytest.mark.parametrize("name,pol", [("straddle", "tukey"), ("loops", "weighted"), ("priors_run", "cauchy"), ("isolated", "none")])
def test_against_the_numpy_references(name, pol, man):
    p = pc.policy(name, man, pol)
    D = pc.DOF[man]
    P = ni.numpy_problem(p.prob) if p.info is not None else (nl.Se2LossProblem if man == "se2" else nl.Se3LossProblem).from_problem(p.prob)
    P.loss = p.loss
    Hn, gn = P.normal_equations()
    nb, (ld, f64) = _ref(name, man, pol, lam=0.0)
    C0 = _c0(name, man, pol)
    ratios, bad, stray = pr.h_check(pr.blocks_of(Hn, p.prob.pose_col, D), ld, f64, C0)
    assert not bad and stray == 0, bad[:5]
    assert pr.g_check(pr.rows_of(gn, p.prob.pose_col, D), ld, f64, C0).max() <= 1.0
    assert pr.scalar_check(P.cost(), ld.cost, f64.cost, ld.M_cost, ld.n_terms, C0).max() <= 1.0
    rng = np.random.default_rng(3)
    a, b = rng.normal(size=(2, ld.n_v, D))
    _, Jd = P.jacobian()
    u, w = Jd @ pr.to_columns(a, p.prob.pose_col, D), Jd @ pr.to_columns(b, p.prob.pose_col, D)
    got, mag = ld.jv_gram(a, b)
    g64, _ = f64.jv_gram(a, b)
    assert pr.scalar_check([u @ u, u @ w, w @ w], got, g64, mag, ld.n_terms, C0 + D).max() <= 1.0


# ---- 2. premises ----------------------------------------------------------------------------------------------------------------
def _degree(d):
    return np.bincount(d.e_from, minlength=d.n_v) + np.bincount(d.e_to, minlength=d.n_v)


def _pair_count(d, a, b):
    ef, et = d.e_from.astype(int), d.e_to.astype(int)
    return int(((ef == a) & (et == b)).sum()), int(((ef == b) & (et == a)).sum())


@pytest.mark.parametrize("man", MANIFOLDS)
@pytest.mark.parametrize("name", CASES)
def test_premises(name, man):
    c = pc.build(name, man)
    d, f, vpt = c.d, c.facts, c.vpt
    ef, et = d.e_from.astype(int), d.e_to.astype(int)
    assert d.n_e <= 1500
    assert ((ef < et).sum() > 0) and ((ef > et).sum() > 0)                # both orientations
    assert c.turned.sum() >= 1
    if name == "straddle" or name in pc.PRIOR_LAYOUTS:
        assert d.n_v == 2 * vpt + 5 and (d.n_v - 1) // vpt == 2 and d.n_v % vpt != 0
        for a, b in f.straddling:
            fw, bw = _pair_count(d, a, b)
            assert fw >= 1 and bw >= 1 and a // vpt != b // vpt            # a multi-edge given in both directions across tiles
        assert _pair_count(d, vpt - 1, 2 * vpt)[0] == 1
    if name == "straddle":
        z = f.rejected_vertex
        touching = (ef == z) | (et == z)
        assert touching.sum() == 2
        for pol, info in (("tukey", False),):
            nb = pc.numpy_blocks(name, man, pol)                           # (np_ref_loss alone)
            assert (nb.rho1 == 0.0).sum() >= 1 and (nb.rho1 > 0.0).sum() >= 1
            assert (nb.rho1[touching] == 0.0).all()
            assert nl.threshold_margin(pc.policy(name, man, pol).loss, nb.s) > 1e-9
            assert not nb.r[nb.rho1 == 0.0].any() and not nb.J[nb.rho1 == 0.0].any()
    if name == "isolated":
        nb = pc.numpy_blocks(name, man, "tukey")
        assert (nb.rho1 == 0.0).sum() >= 1
        deg = _degree(d)
        assert all(deg[v] == 0 for v in f.isolated) and (np.delete(deg, f.isolated) > 0).all()
        assert f.isolated[-1] == d.n_v - 1 and f.isolated[1] % vpt == vpt - 1 and 0 < f.isolated[0] < vpt - 1
    if name == "multi":
        for a, b, P in f.pairs:
            fw, bw = _pair_count(d, a, b)
            assert fw + bw == P and a // vpt != b // vpt and (P < 2 or (fw > 0 and bw > 0))
        assert [P for _, _, P in f.pairs] == [1, 2, 64, 257]
        # the 257 are the last, consecutive edges (257 > 256: any such run lies in two workgroups of k_pg_edges)
        k0, (a, b, _) = f.first_parallel, f.pairs[-1]
        assert d.n_e == k0 + 257 and (np.minimum(ef[k0:], et[k0:]) == a).all() and (np.maximum(ef[k0:], et[k0:]) == b).all()
    if name in ("hub_lo", "hub_hi"):
        deg = _degree(d)
        assert d.n_v == 601 and deg[f.hub] == 600 and (np.delete(deg, f.hub) == 1).all()
        other = np.where(ef == f.hub, et, ef)
        assert (np.bincount(other // vpt)[:-1] >= 2).all()                 # several spokes per tile (the last tile holds one vertex)
        if man == "se2":
            assert (d.n_v + vpt - 1) // vpt < 24                           # (no dissection: the internal order is the caller's)
            assert (other > f.hub).all() if name == "hub_lo" else (other < f.hub).all()   # owns none | all of its blocks
    if name == "loops":
        loops = ef[ef == et]
        assert sorted(loops.tolist()) == sorted([f.lonely, f.triple, f.triple, f.triple, f.tile_end])
        deg = _degree(d)
        assert deg[f.lonely] == 2 and deg[f.triple] > 6 and f.tile_end % vpt == vpt - 1 and deg[f.tile_end] > 2
    if name.startswith("grid"):
        k = int(name[4:])
        assert d.n_e == k and (d.n_v == k if man == "se2" else d.n_v == 2 * vpt)
    if name in pc.PRIOR_LAYOUTS:
        n_prior, start = pc.PRIOR_LAYOUTS[name]
        pv = np.array([q[0] for q in c.priors])
        assert len(pv) == n_prior and not np.array_equal(pv, np.sort(pv))  # the sort has work to do
        sv = np.sort(pv, kind="stable")
        run = np.nonzero(sv == f.run_vertex)[0]
        assert run.tolist() == list(range(start, start + 11))
        counts = np.bincount(pv, minlength=d.n_v)
        assert counts[0] == 1 and counts[1] == 2 and counts[d.n_v - 1] >= 1 and 11 in counts
        if name == "priors_run":
            assert run[0] < 64 <= run[-1]                                  # across the 64-lane boundary
        if name == "priors64":
            assert n_prior == 64 and sv[63] == d.n_v - 1 and sv[62] != sv[63]
        if name == "priors65":
            assert n_prior == 65 and sv[64] == d.n_v - 1 and sv[63] != sv[64]
        deltas = [q[2] for q in c.priors]
        _, _, psc = pc.numpy_blocks(name, man, "none").priors
        assert any(x is None for x in deltas) and (psc < 1.0).any() and (psc == 1.0).any()
        assert (psc[[x is None or x > 1.0 for x in deltas]] == 1.0).all()


@pytest.fixture(scope="module")
def tile_order(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("tile_order") / "host_harness_tile_order")
    cc = subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Wextra", "-I", CSRC, os.path.join(ROOT, "tests", "host_harness_tile_order.cpp"),
                         os.path.join(CSRC, "plan_lists.cpp"), os.path.join(CSRC, "factor_schedule.cpp"), "-pthread", "-o", exe],
                        capture_output=True, text=True)
    assert cc.returncode == 0, cc.stderr[-4000:]

    def run(nt, nd, leaf, pairs):
        p = subprocess.run([exe, str(nt), str(nd), str(leaf)], input="".join(f"{a} {b}\n" for a, b in pairs), capture_output=True, text=True, timeout=60)
        assert p.returncode == 0 and p.stdout.startswith("ok "), (p.stdout[-500:], p.stderr[-500:])
        return np.array(p.stdout.split()[1:], dtype=np.int64)
    return run


@pytest.mark.parametrize("man", MANIFOLDS)
def test_permuted_premise(man, tile_order):
    """PoseGraphSolver::set_structure: vmap[v] = tperm[v / vpt] vpt + v % vpt with tperm = tile_order(nt, tile graph, nd, leaf 2)."""
    c = pc.build("permuted", man)
    d, vpt = c.d, c.vpt
    nt = (d.n_v + vpt - 1) // vpt
    assert nt == pc.PERMUTED_TILES >= 24
    ef, et = d.e_from.astype(int), d.e_to.astype(int)
    pairs = sorted({(a, b) for a, b in zip(ef // vpt, et // vpt) if a != b})
    assert np.array_equal(tile_order(nt, 0, 2, pairs), np.arange(nt))
    tperm = tile_order(nt, 1, 2, pairs)
    assert sorted(tperm.tolist()) == list(range(nt)) and not np.array_equal(tperm, np.arange(nt))
    vmap = tperm[np.arange(d.n_v) // vpt] * vpt + np.arange(d.n_v) % vpt
    a, b = vmap[ef], vmap[et]
    assert ((ef < et) & (a > b)).any() and ((ef > et) & (a < b)).any()
    # the placement restated with that order reproduces the reference: the vertex map is not what the check sees
    nb, (ld, f64) = _ref("permuted", man, "none")
    H4, g = pr.emulate_export(f64, None, vmap=vmap)
    ratios, bad, stray = pr.h_check(H4, ld, f64, _c0("permuted", man, "none"), use_referee=False)
    assert not bad and stray == 0


# ---- 3. the referee arm is not what makes the cases pass --------------------------------------------------------------------------
@pytest.mark.parametrize("name,pol,man", pc.all_runs(), ids=["-".join(t) for t in pc.all_runs()])
def test_fp64_restatement_passes_without_the_referee_arm(name, pol, man):
    nb, (ld, f64) = _ref(name, man, pol)
    C0 = _c0(name, man, pol)
    D = pc.DOF[man]
    dist = pr._dist
    b_d = pr.gamma(ld.P_d, C0) * ld.M_d; b_d[~ld.touched] = 0.0
    b_o = pr.gamma(ld.P_o, C0) * ld.M_o; b_o[ld.P_o == 0] = 0.0
    rng = np.random.default_rng(7)
    a, b = rng.normal(size=(2, ld.n_v, D))
    jl, mag = ld.jv_gram(a, b)
    j64, _ = f64.jv_gram(a, b)
    ratios = dict(diag=pr._ratio(dist(f64.Hd, ld.Hd), b_d), off=pr._ratio(dist(f64.Ho, ld.Ho), b_o),
                  g=pr.g_check(f64.g, ld, f64, C0, use_referee=False),
                  cost=pr.scalar_check(f64.cost, ld.cost, f64.cost, ld.M_cost, ld.n_terms, C0, use_referee=False),
                  jv=pr.scalar_check(j64, jl, j64, mag, ld.n_terms, C0 + D, use_referee=False))
    for k, v in ratios.items():
        assert pr.worst(v)[0] <= 1.0, (k, pr.worst(v))
    # vertices with no live term: exactly lambda I and a zero gradient, in both dtypes
    quiet = ~ld.touched
    assert (np.asarray(ld.Hd[quiet], dtype=np.float64) == pc.LAM * np.eye(D)).all() and not np.asarray(ld.g[ld.P_g == 0], dtype=np.float64).any()
    if name == "straddle" and pol == "tukey":
        assert quiet[pc.build(name, man).facts.rejected_vertex]
    if name == "isolated":
        assert quiet[pc.build(name, man).facts.isolated].all()


# ---- 4. mutations of the placement ------------------------------------------------------------------------------------------------
def _mutated(name, man, pol, mutation):
    nb, (ld, f64) = _ref(name, man, pol)
    C0 = _c0(name, man, pol)
    H4, g = pr.emulate_export(f64, mutation)
    ratios, bad, stray = pr.h_check(H4, ld, f64, C0)
    gbad = np.nonzero(pr.g_check(g, ld, f64, C0) > 1.0)[0].tolist()
    return pc.build(name, man), ld, bad, stray, gbad


@pytest.mark.parametrize("man", MANIFOLDS)
@pytest.mark.parametrize("name,pol", [("straddle", "weighted"), ("loops", "cauchy"), ("priors_run", "none"), ("isolated", "tukey"), ("multi", "huber")])
def test_the_unmutated_placement_passes(name, pol, man):
    c, ld, bad, stray, gbad = _mutated(name, man, pol, None)
    assert not bad and stray == 0 and not gbad


@pytest.mark.parametrize("man", MANIFOLDS)
def test_mutation_cross_block_transposed(man):
    """straddle, weighted: G_ab is not symmetric, every off-diagonal block with a live edge is wrong and nothing else is"""
    c, ld, bad, stray, gbad = _mutated("straddle", man, "weighted", "cross_transposed")
    live = {(int(h), int(l)) for (h, l), P in zip(ld.pairs, ld.P_o) if P > 0}
    assert {(k, a, b) for k, a, b in bad} == {(k, a, b) for k in ("lower", "upper") for a, b in live} and not gbad and stray == 0
    assert ("lower", c.vpt, c.vpt - 1) in bad and ("lower", 2 * c.vpt, c.vpt - 1) in bad


@pytest.mark.parametrize("man", MANIFOLDS)
@pytest.mark.parametrize("pol", ["huber", "weighted"])
def test_mutation_self_loop_without_transpose(man, pol):
    c, ld, bad, stray, gbad = _mutated("loops", man, pol, "loop_without_transpose")
    f = c.facts
    assert sorted(bad) == sorted(("diag", v, v) for v in (f.lonely, f.triple, f.tile_end)) and not gbad


@pytest.mark.parametrize("name", ["hub_hi", "hub_lo", "multi"])
def test_mutation_owner_is_the_smaller_endpoint(name):
    c, ld, bad, stray, gbad = _mutated(name, "se2", "huber", "owner_smaller")
    assert {(k, a, b) for k, a, b in bad} == {(k, int(h), int(l)) for k in ("lower", "upper") for h, l in ld.pairs} and not gbad
    if name == "multi":
        a, b, P = c.facts.pairs[-1]
        assert ("lower", b, a) in bad and ld.P_o[[tuple(p) == (b, a) for p in ld.pairs.tolist()]][0] == 257


@pytest.mark.parametrize("man", MANIFOLDS)
def test_mutation_vpt_off_by_one(man):
    c, ld, bad, stray, gbad = _mutated("straddle", man, "none", "vpt_off_by_one")
    moved = {v for _, a, b in bad for v in (a, b)}
    assert bad and min(max(a, b) for _, a, b in bad) == c.vpt - 1           # the first vertex h_block_ptr would misplace
    assert ("diag", c.vpt - 1, c.vpt - 1) in bad and ("diag", c.d.n_v - 1, c.d.n_v - 1) in bad
    assert not any(k == "diag" and a < c.vpt - 1 for k, a, b in bad) and moved


@pytest.mark.parametrize("man", MANIFOLDS)
def test_mutation_prior_run_cut_at_the_workgroup_boundary(man):
    c, ld, bad, stray, gbad = _mutated("priors_run", man, "none", "prior_run_cut")
    R = c.facts.run_vertex
    assert bad == [("diag", R, R)] and gbad == [R]
    for name in ("priors64", "priors65"):                                     # (their runs end before the boundary: nothing to cut)
        assert _mutated(name, man, "none", "prior_run_cut")[2] == []


@pytest.mark.parametrize("man", MANIFOLDS)
def test_mutation_stale_gradient_of_an_isolated_vertex(man):
    c, ld, bad, stray, gbad = _mutated("isolated", man, "none", "stale_gradient")
    assert not bad and gbad == sorted(c.facts.isolated)
    c, ld, bad, stray, gbad = _mutated("straddle", man, "tukey", "stale_gradient")
    assert c.facts.rejected_vertex in gbad and gbad == np.nonzero(ld.P_g == 0)[0].tolist()   # (every vertex Tukey left without a term)
