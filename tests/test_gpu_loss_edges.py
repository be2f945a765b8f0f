"""The robust-loss correction of every pose-graph device path, edge by edge (needs a real MI355X: `pytest -m gpu`).

The cases, the long-double reference, its fp64 restatement and the rule are those of tests/loss_edge_cases.py
(tests/test_loss_edge_cases_host.py proves the premises and holds the host builds of the same code to the same rule): graphs of
disjoint vertex pairs, so that every block of the dense export belongs to one edge, under the general and the weighted policy.
Per edge: the exports r~ and the literal J~ (k_pg_export), H_aa, H_bb, the cross block and both rows of g at lambda = 0.5 (the
corrected-as-formed blocks of k_pg_edges | k_pg6_assemble | k_pg2_assemble; a self-loop's single block too), the three sums of
jv_gram with a and b non-zero on that edge's pair only (edge_jv), and compute_cost on sub-graphs whose terms lie within a factor
1e3 of each other.  A pair whose edge has rho' == 0 holds exactly lambda I, zero rows and zero exports.  Every run prints one
LOSSEDGE line per policy: per band of s the worst error, the restatement's and the ratio to the bound."""
import numpy as np
import pytest

import loss_edge_cases as lc
from apex_solver_amd import capi
from apex_solver_amd.pose_graph import GpuSparseCholeskySolver, Loss, PoseGraphProblem

pytestmark = pytest.mark.gpu
PATHS = ["se3", "se3-row", "se2", "so3"]
KIND_IDS = [lc.kind_id(k) for k in lc.KINDS]


def handle(path, d, info, loss=None, huber_delta=None):
    prob = PoseGraphProblem(d, huber_delta, loss=loss, information=info)
    s = GpuSparseCholeskySolver(0)
    if path == "se3-row":
        s.with_option("row_owned_assembly", 1)
    s.initialize_structure(prob)
    s.set_parameters(d.poses)
    return s, prob.pose_col


def exports(path, cs, loss=None, huber_delta=None):
    """everything a handle on the whole graph gives, in the per-edge form of loss_edge_cases.KEYS (without cost)"""
    d, info = lc.graph_of(cs)
    D = cs.D
    s, col = handle(path, d, info, loss, huber_delta)
    got = dict(r=s.get_residual(), J=s.get_jacobian_blocks(), gram=np.zeros((cs.n, 3)))
    H, g = s.get_hessian(lc.LAMBDA)
    for e in range(cs.n):
        a = np.zeros(D * d.n_v); b = np.zeros(D * d.n_v)
        for v, half in ((int(cs.e_from[e]), slice(0, D)), (int(cs.e_to[e]), slice(D, 2 * D))):
            a[col[v]:col[v] + D] = cs.a[e, half]; b[col[v]:col[v] + D] = cs.b[e, half]
        got["gram"][e] = s.jv_gram(a, b)
    whole = s.compute_cost()
    s.close()
    got.update(lc.blocks_from_dense(cs, H, g, lc.LAMBDA, col))
    return got, H, g, whole, col


def sub_cost(path, cs, group, loss=None, huber_delta=None):
    d, info = lc.graph_of(cs, group)
    s, _ = handle(path, d, info, loss, huber_delta)
    cost = s.compute_cost()
    s.close()
    return cost


@pytest.mark.parametrize("kind", lc.KINDS, ids=KIND_IDS)
@pytest.mark.parametrize("path", PATHS)
def test_every_edge_meets_the_rule(path, kind):
    man = path.split("-")[0]
    loss = Loss(capi.LOSS_KINDS.index(kind[0]), float(kind[1]), float(kind[2]))
    for policy in lc.POLICIES:
        cs = lc.cases(man, kind, policy)
        ld, f64, meta = lc.reference(man, kind, policy)
        tag = f"{path} {lc.kind_id(kind)} {policy}"
        got, H, g, whole, col = exports(path, cs, loss)
        errs = lc.check(tag, cs, got, ld, f64, meta)
        D = cs.D
        for e in np.nonzero(meta["rho1"] == 0.0)[0]:        # exactly lambda I on the pair of an edge the loss has switched off
            for v in {int(cs.e_from[e]), int(cs.e_to[e])}:
                blk = H[col[v]:col[v] + D, col[v]:col[v] + D]
                assert np.array_equal(blk, lc.LAMBDA * np.eye(D)) and not g[col[v]:col[v] + D].any(), (tag, cs.label[e])
        cw = 0.0
        total = 0.0
        for grp in lc.cost_groups(ld):
            c = sub_cost(path, cs, grp, loss)
            total += c
            eg, e64, bound = lc.cost_error(c, grp, ld, f64, meta)
            print(f"  cost sub-graph n={len(grp)} ref={float(0.5 * ld['cost'][grp].sum()):.3e} e={eg:.1e} e_f64={e64:.1e} bound={bound:.1e}")
            assert eg <= bound, (tag, "cost of the sub-graph", [cs.label[i] for i in grp[:3]], eg, e64, bound)
            if (ld["cost"][grp] == 0).all():
                assert c == 0.0
            cw = max(cw, eg / bound)
        assert abs(whole - total) <= 1e-13 * max(1.0, total)     # the whole graph's cost is the sum of its parts
        lc.report(tag, meta, errs, cw)


@pytest.mark.parametrize("path", PATHS)
def test_huber_through_the_loss_is_the_legacy_delta_to_the_bit(path):
    kind = next(k for k in lc.KINDS if k[0] == "HUBER")
    cs = lc.cases(path.split("-")[0], kind, "general")
    _, _, meta = lc.reference(path.split("-")[0], kind, "general")
    assert (meta["s"] > kind[1] ** 2).sum() >= 4 and (meta["s"] < kind[1] ** 2).sum() >= 10      # both sides of delta^2 (SO3: s < pi^2)
    a, Ha, ga, ca, _ = exports(path, cs, Loss(capi.LOSS_HUBER, float(kind[1])))
    b, Hb, gb, cb, _ = exports(path, cs, None, float(kind[1]))
    for k in a:
        assert np.array_equal(a[k], b[k]), k
    assert np.array_equal(Ha, Hb) and np.array_equal(ga, gb) and ca == cb
