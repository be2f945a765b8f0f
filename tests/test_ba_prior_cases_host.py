"""The crafted prior sets of tests/ba_prior_cases.py and the long double reference of tests/ba_prior_ld.py.  No GPU needed.

Three groups: the reference against the existing fp64 model (tests/ba_prior_ref.py), the premises every case is named after,
and what the rule of tests/test_gpu_ba_prior_crafted.py rejects -- with the fp64 restatement standing in for the device, one
defect injected at a time, and beside each verdict whether the whole-array criteria of tests/test_gpu_ba_priors.py would have
let it through (printed as a table, recorded in DESIGN.md §17; evidence, not an assertion about that file)."""
import numpy as np
import pytest

import ba_prior_cases as pc
import ba_prior_ld as pl
import ba_prior_ref as br
import fixed_masks as fm
import np_ref_ba_tr as bt
from apex_solver_amd import capi
from apex_solver_amd.layout import reference_column_layout
from apex_solver_amd.solver import OptimizationType

OPT = {pc.SELFCAL: OptimizationType.SelfCalibration, pc.BA: OptimizationType.BundleAdjustment}


def cols_of(lay, n_cam):
    return np.concatenate([lay.pose_col[:n_cam, None] + np.arange(6)[None], lay.intr_col[:n_cam, None] + np.arange(3)[None]], axis=1)


@pytest.mark.parametrize("name", pc.CASES)
def test_reference_against_the_existing_model(name):
    mode, d, pp, ip = pc.case(name)
    ld, f64 = pl.pair(d.poses, d.intr, pp, ip)
    lay = reference_column_layout(d.n_cam, d.n_pt)
    r, J = br.prior_system(d.poses, d.intr, pp, ip, lay)
    cols = cols_of(lay, d.n_cam)
    p_ref = np.asarray(J.multiply(J).sum(axis=0)).ravel()[cols]
    q_ref = (J.T @ r)[cols]
    P = br.PriorBaProblem(d, OPT[mode], None, fm.empty(d.n_cam, d.n_pt), pose_priors=pp, intr_priors=ip)
    wp, wi = P.prior_residuals()
    for ref in (ld, f64):
        # (the long double side normalises the quaternion in long double: q sees that through j^2 |x|, |x| <= 1)
        assert (pl.dist(ref.p, p_ref) <= 1e-13 * ref.pmag).all()
        assert (pl.dist(ref.q, q_ref) <= 1e-13 * (ref.qmag + ref.pmag)).all()
        assert (pl.dist(ref.rp, wp) <= 1e-13 * (np.abs(wp) + np.abs(np.asarray(ref.P.j, dtype=np.float64))[:, None])).all()
        assert (pl.dist(ref.ri, wi) <= 1e-13 * np.abs(wi)).all()
        total, _ = ref.total_cost()
        assert abs(float(total) - float(r @ r)) <= 1e-13 * float(r @ r)
    assert (ld.p[:, 6:] == 0).all() or mode == pc.SELFCAL
    # away from the Huber boundary everywhere but in `threshold`: the decision does not hang on the device's last bit of s
    if name != "threshold":
        for B in (ld.P, ld.I):
            h = B.delta > 0
            assert (np.abs(B.s64[h] - B.delta[h] ** 2) > 1e-9 * B.delta[h] ** 2).all()


def test_premises_of_the_shapes():
    for name in pc.CASES:
        if name != "permuted":
            assert np.array_equal(pc.host_structure(name)["cmap"], np.arange(pc.case(name)[1].n_cam)), name
    for n in pc.EDGE_COUNTS:
        for w in (9, 6):
            mode, d, pp, ip = pc.case(f"edge{n}_{w}")
            cams = sorted({q[0] for q in pp})
            assert d.n_cam == n and cams[0] == 0 and 63 in cams and cams[-1] == n - 1 and (w == 9) == bool(ip)
            groups = {c // 64 for c in cams}
            assert groups == set(range((n + 63) // 64))                   # a prior in every workgroup of k_ba_prior_eval
            if n > 64:
                assert 64 in cams and (n - 1) % 64 == 0                   # the last camera is lane 0 of its workgroup, alone in it
    mode, d, pp, ip = pc.case("cost257")
    assert mode == pc.BA and d.n_cam == 257 == len(pp) and sorted(q[0] for q in pp) == list(range(257))
    assert [c for c in range(257) if c >= 256] == [256] and 6 * 257 == 1542 and (1542 + 143) // 144 == 11
    mode, d, pp, ip = pc.case("straddle")
    assert d.n_cam == 29 and 9 * 28 < 256 < 9 * 29 and 9 * 16 == 144 and {q[0] for q in pp} == {q[0] for q in ip} == {15, 16, 28}
    # the arms of k_ba_prior_eval
    for name, want in (("pose_only", (3, 0)), ("intr_only", (0, 3)), ("disjoint", (3, 3))):
        mode, d, pp, ip = pc.case(name)
        assert mode == pc.SELFCAL and (len(pp), len(ip)) == want and not {q[0] for q in pp} & {q[0] for q in ip}
    mode, d, pp, ip = pc.case("unobserved")
    seen = set(d.cam_idx.tolist())
    assert 3 not in seen and 6 not in seen and {q[0] for q in pp} >= {3} and 3 in {q[0] for q in ip} and 6 not in {q[0] for q in pp + ip}
    ld = pl.PriorRef(d.poses, d.intr, pp, ip)
    assert (ld.k[3] > 0).all() and (ld.k[6] == 0).all()
    mode, d, pp, ip = pc.case("run200")
    ld = pl.PriorRef(d.poses, d.intr, pp, ip)
    assert ld.runs[2, 0] == pc.RUN and ld.runs[2, 1] == 5
    on2 = ld.P.cam == 2
    frac = ld.P.out[on2].mean()
    w = ld.P.w[on2]
    assert 0.3 < frac < 0.7 and w.min() == 2.0 ** -6 and w.max() == 2.0 ** 6, (frac, w.min(), w.max())


def test_premise_of_the_internal_camera_order():
    mode, d, pp, ip = pc.case("permuted")
    hs = pc.host_structure("permuted")
    cmap = hs["cmap"]
    assert hs["hub_cameras"] == 1 and cmap[pc.HUB] == d.n_cam - 1 and hs["tile_rows"] == 24
    assert sorted(cmap.tolist()) == list(range(d.n_cam))
    for lst in (pp, ip):
        cams = np.array([q[0] for q in lst])
        assert (cmap[cams] != cams).sum() >= len(set(cams.tolist())) - 1            # (camera 0 may keep its place)
        order = np.argsort(cmap[cams], kind="stable")
        assert not np.array_equal(order, np.arange(len(cams)))                       # the stable sort changes the caller's order
        assert not np.array_equal(order, np.argsort(cams, kind="stable"))            # and not into the caller's camera order
        assert len(set(cams.tolist())) < len(cams)                                   # runs of two: their order is the caller's


def test_premises_of_the_threshold_blocks():
    mode, d, pp, ip = pc.case("threshold")
    ld = pl.PriorRef(d.poses, d.intr, pp, ip)
    six = pl.PriorRef(d.poses, d.intr, pp, ip, s_rows=6)
    seen = set(d.cam_idx.tolist())
    d2 = pc.DELTA_T ** 2
    k_pose = k_intr = 0
    for label, (c, kind, row, side) in pc.THRESHOLD_BLOCKS.items():
        assert c not in seen
        B, k = (ld.P, k_pose) if kind == "pose" else (ld.I, k_intr)
        assert B.cam[k] == c and B.delta[k] == pc.DELTA_T and B.w[k] == 1.0
        r = np.asarray(B.r[k], dtype=np.float64)
        if row is not None:
            assert np.count_nonzero(r) == 1 and r[row] > 0
            if side == 0:
                assert r[row] == pc.DELTA_T and B.s64[k] == d2 and not B.out[k] and B.sc[k] == 1.0      # bitwise on the boundary
            else:
                assert r[row] > pc.DELTA_T and B.s64[k] > d2 and B.s64[k] <= d2 * (1 + 2.0 ** -40) and B.out[k] and B.sc[k] < 1.0
        else:
            assert np.count_nonzero(r) == 2 and r[0] == 0.125 and six.P.s64[k] == 2.0 ** -6 < d2 and not six.P.out[k]
            assert B.out[k] == bool(side) and (B.s64[k] == 5 * 2.0 ** -6 if side else B.s64[k] == 2.0 ** -5)
        if kind == "pose":
            k_pose += 1
        else:
            k_intr += 1
    # the qz blocks: no column takes them -- zero p's gradient, a nonzero cost
    for label in ("qz_on", "qz_over"):
        c = pc.THRESHOLD_BLOCKS[label][0]
        assert not ld.q[c].any() and ld.cost[c] > 0 and (ld.p[c, :6] > 0).all()


@pytest.mark.parametrize("name", pc.CASES)
def test_no_block_of_the_schur_reduction_adds_atomically(name):
    mode, d, _, _ = pc.case(name)
    dc = pc.width(name)
    for lists in (capi.pair_lists(d.n_cam, d.n_pt, dc, d.cam_idx, d.pt_idx), capi.pair_lists_queued(d.n_cam, d.n_pt, d.cam_idx, d.pt_idx, dc)):
        assert len(lists["blocks"]) and not (lists["blocks"][:, 3] & 1).any()


# ---- sensitivity ------------------------------------------------------------------------------------------------------------
class StandIn:
    """what a device with a defect would export: p, q, per-camera cost and the corrected residuals"""

    def __init__(self, ref):
        self.p, self.q, self.cost = (np.array(x, dtype=np.float64) for x in (ref.p, ref.q, ref.cost))
        self.rp, self.ri = np.array(ref.rp, dtype=np.float64), np.array(ref.ri, dtype=np.float64)


def _system_without_priors(name):
    """stand-ins for what the prior's part is added to: diag(H_cc) + lambda (>= S_ii's magnitude), g_c and sum r^2"""
    mode, d, _, _ = pc.case(name)
    P = bt.BaProblem(d, OPT[mode], bt.huber(1.0), fm.empty(d.n_cam, d.n_pt))
    r, J = P.jacobian()
    cols = cols_of(P.lay, d.n_cam)
    n2 = np.asarray(J.multiply(J).sum(axis=0)).ravel()[cols]
    return n2 + pc.LAM, (J.T @ r)[cols], float(r @ r)


def new_rule_rejects(dev, ld, f64, S0, g0, ss0):
    total, cost_b = ld.total_cost()
    ratios = dict(S=pl.check(dev.p, ld.p, f64.p, ld.pb, onto=S0 + dev.p), grad=pl.check(dev.q, ld.q, f64.q, ld.qb, onto=g0 + dev.q),
                  cost=pl.check(dev.cost.sum(), total, f64.total_cost()[0], cost_b, onto=ss0 + dev.cost.sum(), roundings=8),
                  rp=pl.check(dev.rp, ld.rp, f64.rp, pl.gam(pl.C0) * np.abs(dev.rp) + pl.gam(pl.QX) * np.abs(np.asarray(ld.P.j, dtype=np.float64))[:, None]),
                  ri=pl.check(dev.ri, ld.ri, f64.ri, pl.gam(pl.C0) * np.abs(dev.ri)))
    return {k: pl.worst(v) for k, v in ratios.items()}


def old_criteria_pass(dev, ld, S0, g0, ss0):
    """the whole-array norms of tests/test_gpu_ba_priors.py on the same numbers; every denominator is a LOWER bound of the norm
    that test divides by (the diagonal of S alone, the camera part of g alone), so 'passes' here is 'passes' there"""
    f = lambda a: np.asarray(a, dtype=np.float64)
    rel = lambda a, b, extra=0.0: float(np.linalg.norm(f(a) - f(b)) / max(np.sqrt(np.linalg.norm(f(b)) ** 2 + extra), 1e-300))
    p, q = f(ld.p), f(ld.q)
    total = float(ld.total_cost()[0])
    out = dict(S=np.linalg.norm(dev.p - p) / np.linalg.norm(S0 + p) < 1e-12, grad=np.linalg.norm(dev.q - q) / np.linalg.norm(g0 + q) < 1e-12,
               cost=abs(dev.cost.sum() - total) / (ss0 + total) < 1e-12, res=rel(dev.rp, ld.rp) < 1e-12 and (not len(dev.ri) or rel(dev.ri, ld.ri) < 1e-12),
               blocks=bool((np.abs(dev.p - p).max(axis=1) <= 1e-12 * (S0 - pc.LAM + p).max(axis=1)).all()))
    return out


def defects():
    """(label, case, the stand-in device)"""
    out = []
    for name in ("run200", "threshold"):
        mode, d, pp, ip = pc.case(name)
        out.append(("s over six rows", name, StandIn(pl.PriorRef(d.poses, d.intr, pp, ip, np.float64, s_rows=6))))
    mode, d, pp, ip = pc.case("run200")
    f64 = pl.PriorRef(d.poses, d.intr, pp, ip, np.float64)
    on2 = np.flatnonzero(f64.P.cam == 2)
    k = int(on2[np.argmin(np.asarray(f64.P.j, dtype=np.float64)[on2])])           # the block that weighs least
    dev = StandIn(pl.PriorRef(d.poses, d.intr, pp[:k] + pp[k + 1:], ip, np.float64))
    dev.rp = np.insert(dev.rp, k, f64.rp[k], axis=0)                               # (its residual is still exported)
    out.append((f"block {k} of 200 dropped (j = {float(f64.P.j[k]):.3g})", "run200", dev))
    mode, d, pp, ip = pc.case("edge65_9")
    dev = StandIn(pl.PriorRef(d.poses, d.intr, pp, ip, np.float64))
    for a in (dev.p, dev.q, dev.cost):
        a[[63, 64]] = a[[64, 63]]
    out.append(("cameras 63 and 64 swapped", "edge65_9", dev))
    mode, d, pp, ip = pc.case("straddle")
    dev = StandIn(pl.PriorRef(d.poses, d.intr, pp, ip, np.float64))
    dev.p[16, 8] *= 1.0 + 1e-9
    out.append(("p of one k2 column off by 1e-9", "straddle", dev))
    return out


def test_the_rule_rejects_every_injected_defect():
    print()
    print("| defect | case | new rule: worst ratio (quantity) | old criteria that still pass | old file passes |")
    print("|---|---|---|---|---|")
    for label, name, dev in defects():
        mode, d, pp, ip = pc.case(name)
        ld, f64 = pl.pair(d.poses, d.intr, pp, ip)
        S0, g0, ss0 = _system_without_priors(name)
        clean = new_rule_rejects(StandIn(f64), ld, f64, S0, g0, ss0)
        assert max(clean.values()) <= 1.0, (name, clean)                           # the restatement itself passes
        got = new_rule_rejects(dev, ld, f64, S0, g0, ss0)
        old = old_criteria_pass(dev, ld, S0, g0, ss0)
        k = max(got, key=got.get)
        print(f"| {label} | {name} | {got[k]:.3g} ({k}) | {', '.join(n for n, ok in old.items() if ok) or 'none'} | {'yes' if all(old.values()) else 'no'} |")
        assert got[k] > 1.0, (label, got)
