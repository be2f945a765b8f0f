"""Crafted pose graphs for the pose-graph assembly (tests/test_pg_asm_ref_host.py asserts their premises on the lists,
tests/test_gpu_pg_crafted.py runs them on the device) -- TEST INFRASTRUCTURE ONLY.

Every case is one description -- vertices, directed edges, prior blocks, written with vpt = 24 (SE3) | 48 (SE2) vertices per
144-row tile -- built for both manifolds.  The names sit on the case distinctions of csrc/pg_kernels.hip:
  straddle   2 vpt + 5 vertices (a partial last tile), a chain, multi-edges in both directions across both tile boundaries and
             between the first and the last vertex, an edge from the last vertex of tile 0 to the first of tile 2
  multi      pairs of vertices in different tiles joined by P = 1, 2, 64, 257 parallel edges (one graph holds the four pairs;
             the 257 are consecutive edges, so they span two workgroups of k_pg_edges and one incident list of k_pg2_assemble)
  hub_lo / hub_hi   601 vertices, one of degree 600: vertex 0 (in SE2 it owns none of its blocks) | vertex 600 (it owns all)
  loops      a self-loop on a vertex with no other edge, three on a vertex of the chain, one on the last vertex of a tile
  isolated   vertices without edge or prior, in the interior, at a tile's end and as the last vertex
  grid255 / 256 / 257   n_e (SE3, two tiles) and n_v = n_e (SE2) at a 256-thread workgroup boundary
  permuted   25 tiles in a chain plus one long-range edge: tile_order dissects only from 24 tiles on (plan_lists.cpp), so this is
             the smallest size at which the internal vertex order is not the caller's
  priors_run / priors64 / priors65   the straddle graph with prior blocks: runs of 1, 2 and 11 on single vertices, shuffled.
             priors_run has 75 blocks with the 11-run at sorted positions 60..70 (across k_pg2_priors's 64-lane boundary);
             priors64 / priors65 have exactly that many blocks, the run ending at position 62 | 63 and a single block on the last
             vertex at position 63 | 64 (the last lane of a workgroup | the first lane of the next one).  (A run at 60..70 needs
             71 blocks, so the two counts and that run cannot be one case.)
Poses and measurements are random and close to the identity (rotations below ~0.5 rad), so every residual is of order one and
far from the Log's branch; every eleventh edge is a gross outlier (translation moved by 8).  About every third chain or spoke
edge is turned round (info_graphs._inverse).  The losses: huber at the 0.6 quantile of the case's own (whitened) residual norms,
Cauchy, Tukey at the 0.85 quantile -- beyond it rho' = 0 --, and Cauchy with info_graphs.information matrices."""
from __future__ import annotations

import functools
from types import SimpleNamespace

import numpy as np

import apex_solver_amd as pkg
import info_graphs as ig
import loss_graphs as lg
import np_ref_info as ni
import np_ref_loss as nl
import pg_asm_ref as pr
from apex_solver_amd.pose_graph import PoseGraphProblem, create_loss_function, se2_as_vector, se3_as_vector

VPT = {"se3": 24, "se2": 48}
DOF = {"se3": 6, "se2": 3}
LAM = 0.5
MULTI_P = (1, 2, 64, 257)
HUB_NV = 601
PERMUTED_TILES = 25
PRIOR_LAYOUTS = {"priors_run": (75, 60), "priors64": (64, 52), "priors65": (65, 53)}   # name -> (n_prior, first position of the 11-run)

# case -> the policies it runs under (the ladders need the legacy policy and one general policy only)
POLICIES = {
    "straddle": ("none", "huber", "cauchy", "tukey", "weighted"),
    "multi": ("huber", "cauchy"),
    "hub_lo": ("huber", "weighted"), "hub_hi": ("huber", "weighted"),
    "loops": ("huber", "cauchy", "weighted"),
    "isolated": ("none", "tukey", "weighted"),          # (weighted: pg2_assemble_row_info has its own start of H_vv and g_v)
    "grid255": ("huber", "cauchy"), "grid256": ("huber", "cauchy"), "grid257": ("huber", "cauchy"),
    "permuted": ("none", "weighted"),
    "priors_run": ("none", "cauchy"), "priors64": ("none",), "priors65": ("none",),
}
KERNEL_POLICY = {"none": "legacy", "huber": "legacy", "cauchy": "general", "tukey": "general", "weighted": "weighted"}


def _chain(vs):
    return [(int(a), int(b), True) for a, b in zip(vs[:-1], vs[1:])]


@functools.lru_cache(maxsize=None)
def describe(name, vpt):
    """n_v, edges [(from, to, may be turned round)], facts the premises are asserted from"""
    f = SimpleNamespace()
    if name == "straddle" or name in PRIOR_LAYOUTS:
        n_v = 2 * vpt + 5
        f.straddling = [(vpt - 1, vpt), (2 * vpt - 1, 2 * vpt), (0, n_v - 1)]
        edges = _chain(np.arange(n_v))
        for a, b in f.straddling:
            edges += [(a, b, False), (b, a, False)]
        edges += [(vpt - 1, 2 * vpt, False)]
        f.rejected_vertex = vpt + 7                       # both of its (chain) edges are gross outliers: Tukey takes them all
        f.outliers = [f.rejected_vertex - 1, f.rejected_vertex]
    elif name == "multi":
        n_v = 2 * vpt
        f.pairs = [(3 + 2 * k, vpt + 3 + 2 * k, P) for k, P in enumerate(MULTI_P)]
        edges = _chain(np.arange(n_v))
        for a, b, P in f.pairs:
            f.first_parallel = len(edges)
            edges += [((a, b, False) if j % 3 else (b, a, False)) for j in range(P)]
    elif name in ("hub_lo", "hub_hi"):
        n_v = HUB_NV
        f.hub = 0 if name == "hub_lo" else n_v - 1
        edges = [(f.hub, v, True) for v in range(n_v) if v != f.hub]
    elif name == "loops":
        n_v = vpt + 6
        f.lonely, f.triple, f.tile_end = 2, 5, vpt - 1
        edges = _chain(np.array([v for v in range(n_v) if v != f.lonely]))
        edges += [(f.lonely, f.lonely, False)] + [(f.triple, f.triple, False)] * 3 + [(f.tile_end, f.tile_end, False)]
    elif name == "isolated":
        n_v = vpt + 4
        f.isolated = [3, vpt - 1, n_v - 1]
        edges = _chain(np.array([v for v in range(n_v) if v not in f.isolated])) + [(1, vpt + 1, False), (vpt + 2, 0, False)]
    elif name.startswith("grid"):
        k = int(name[4:])
        n_v = k if vpt == 48 else 2 * vpt                # SE2: n_v = n_e = k;  SE3: two tiles, n_e = k
        edges = _chain(np.arange(n_v))
        rng = np.random.default_rng(k)
        while len(edges) < k:
            a, b = (int(x) for x in rng.choice(n_v, 2, replace=False))
            edges.append((a, b, False))
    elif name == "permuted":
        n_v = PERMUTED_TILES * vpt
        f.long_range = (2 * vpt + 5, 20 * vpt + 7)
        edges = _chain(np.arange(n_v)) + [f.long_range + (False,), (20 * vpt + 9, 2 * vpt + 1, False)]
    else:
        raise KeyError(name)
    f.n_v, f.edges = n_v, edges
    return f


def prior_layout(name, n_v):
    """(vertex of every prior block in the CALLER's shuffled order, the run vertex): sorted by vertex the blocks are one on vertex
    0, two on vertex 1, one or more on each vertex up to the run vertex n_v - 2 with its 11, the rest on the last vertex."""
    n_prior, start = PRIOR_LAYOUTS[name]
    R = n_v - 2
    counts = np.zeros(n_v, dtype=np.int64)
    counts[0], counts[1] = 1, 2
    rest, m = start - 3, R - 2
    counts[2:R] = rest // m
    counts[2:2 + rest % m] += 1
    counts[R] = 11
    counts[n_v - 1] = n_prior - start - 11
    v = np.repeat(np.arange(n_v), counts)
    assert len(v) == n_prior and counts[n_v - 1] >= 1
    return np.random.default_rng(n_prior).permutation(v), R


def _random_poses(man, n, rng):
    if man == "se2":
        return np.column_stack([rng.standard_normal((n, 2)), rng.uniform(-0.5, 0.5, n)])
    q = np.column_stack([np.ones(n), 0.15 * rng.standard_normal((n, 3))])
    return np.column_stack([rng.standard_normal((n, 3)), q / np.linalg.norm(q, axis=1, keepdims=True)])


@functools.lru_cache(maxsize=None)
def build(name, man):
    """The graph of a case on a manifold with its uncorrected numpy linearisation: once, read-only."""
    vpt = VPT[man]
    f = describe(name, vpt)
    rng = np.random.default_rng(sum(map(ord, name + man)))
    ef = np.array([e[0] for e in f.edges], dtype=np.uint32); et = np.array([e[1] for e in f.edges], dtype=np.uint32)
    n_e = len(ef)
    poses = _random_poses(man, f.n_v, rng)
    meas = _random_poses(man, n_e, rng)
    out = np.zeros(n_e, dtype=bool)
    out[np.arange(5, n_e, 11)] = True
    out[getattr(f, "outliers", [])] = True
    out[ef == et] = False
    k = 2 if man == "se2" else 3
    shift = rng.standard_normal((n_e, k))
    meas[out, :k] += 8.0 * shift[out] / np.linalg.norm(shift[out], axis=1, keepdims=True)
    may = np.array([e[2] for e in f.edges], dtype=bool)
    turn = may & (np.arange(n_e) % 3 == 1)
    ef2, et2 = ef.copy(), et.copy()
    ef2[turn], et2[turn] = et[turn], ef[turn]
    meas[turn] = ig._inverse(meas[turn])
    d = pkg.synthetic.PoseGraphData(ids=np.arange(f.n_v, dtype=np.int64), poses=poses, e_from=ef2, e_to=et2, meas=meas, name=name)
    r, J = lg.linearize(d)
    W = ig_information(d)
    rw, Jw = ni.whiten(r, J, W)
    priors = []
    if name in PRIOR_LAYOUTS:
        pv, run_vertex = prior_layout(name, f.n_v)
        f.run_vertex = run_vertex
        deltas = [None, 0.05, 1e3]                       # none | scaled (every |r| here is above 0.05) | not scaled
        for j, v in enumerate(pv):
            x = se2_as_vector(poses[v]) if man == "se2" else se3_as_vector(poses[v])
            priors.append((int(v), x + 0.3 * rng.standard_normal(x.shape), deltas[j % 3]))
    for a in (d.poses, d.meas, d.e_from, d.e_to, r, J, W, rw, Jw):
        a.setflags(write=False)
    return SimpleNamespace(name=name, man=man, D=DOF[man], vpt=vpt, facts=f, d=d, r=r, J=J, W=W, rw=rw, Jw=Jw, outlier=out, turned=turn, priors=priors)


def ig_information(d, seed=11):
    """info_graphs.information's matrices (its own assertions ask for exactly one self-loop, which these graphs need not have)"""
    D = DOF[d.manifold]
    rng = np.random.default_rng(seed)
    out = np.zeros((d.n_e, D, D))
    for e in range(d.n_e):
        Q, R = np.linalg.qr(rng.standard_normal((D, D)))
        Q = Q * np.sign(np.diag(R))[None, :]
        sigma = np.exp(rng.uniform(np.log(ig.SIGMA_LO), np.log(ig.SIGMA_HI), D))
        Wm = (Q * sigma[None, :]) @ Q.T
        out[e] = 0.5 * (Wm + Wm.T)
    return out


@functools.lru_cache(maxsize=None)
def policy(name, man, pol):
    """(problem, kernel policy, loss as np_ref_loss takes it, information or None) of a case under a policy"""
    c = build(name, man)
    kw, info = {}, None
    if pol == "huber":
        kw["huber_delta"] = float(lg.scale_between(c.r, 0.6))
    elif pol == "cauchy":
        kw["loss"] = create_loss_function("cauchy")
    elif pol == "tukey":
        kw["loss"] = create_loss_function("tukey", float(lg.scale_between(c.r, 0.85)))
    elif pol == "weighted":
        kw["loss"] = create_loss_function("cauchy"); kw["information"] = info = c.W
    elif pol != "none":
        raise KeyError(pol)
    prob = PoseGraphProblem(c.d, **kw)                    # nothing fixed: H is what the kernels assemble
    prob.priors = list(c.priors)
    return SimpleNamespace(prob=prob, kernel=KERNEL_POLICY[pol], loss=ni.loss_of(prob), info=info, pol=pol)


@functools.lru_cache(maxsize=None)
def numpy_blocks(name, man, pol):
    """What the numpy references give for the exports: corrected (r~, J~) per edge, the corrector's (sqrt_rho1,
    residual_scaling, alpha_sq_norm, s) per edge, rho' per edge, the prior blocks (vertex, r~, sc) in the caller's order."""
    c, p = build(name, man), policy(name, man, pol)
    r0, J0 = (c.rw, c.Jw) if p.info is not None else (c.r, c.J)
    rt, Jt, arms, ss = nl.correct_edges(r0, J0, p.loss)
    corr = np.array([[float(x) for x in nl.corrector(p.loss, s)[:3]] + [s] for s in ss]).reshape(-1, 4)
    rho1 = np.array([float(nl.evaluate(p.loss, s)[1]) for s in ss])
    P = (nl.Se2LossProblem if man == "se2" else nl.Se3LossProblem).from_problem(p.prob)
    pres, psc = P.prior_blocks() if c.priors else (np.zeros((0, c.D)), np.zeros(0))
    pv = np.array([q[0] for q in c.priors], dtype=np.int64)
    return SimpleNamespace(r=rt, J=Jt, corr=corr.T, rho1=rho1, s=ss, priors=(pv, pres, psc) if c.priors else None)


def magnitudes(name, man, pol, J, r):
    """The per-edge magnitudes of pg_asm_ref.edge_magnitudes for the policy's kernel; J, r: the exported corrected blocks"""
    c, p = build(name, man), policy(name, man, pol)
    if p.kernel == "legacy":
        return pr.edge_magnitudes(c.D, J, r)
    nb = numpy_blocks(name, man, pol)
    return pr.edge_magnitudes(c.D, J, r, raw=(c.r, c.J), corr=nb.corr, info=p.info)


def reference(name, man, pol, J, r, priors, lam=LAM, scaling=None):
    c = build(name, man)
    return pr.pair(c.D, c.d.n_v, c.d.e_from, c.d.e_to, J, r, lam, priors=priors, mags=magnitudes(name, man, pol, J, r), scaling=scaling)


def all_runs():
    """(case, policy, manifold) of every device run"""
    return [(n, p, m) for n, pols in POLICIES.items() for p in pols for m in ("se3", "se2")]
