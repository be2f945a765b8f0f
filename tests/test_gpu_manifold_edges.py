"""The per-factor manifold math of the device (pg_device.hpp, pg2_device.hpp, the retraction of ba_device.hpp) at small
angles, near pi and on either side of every branch, through the C ABI (needs a real MI355X: `pytest -m gpu`).

The cases are those of tests/manifold_ref.py (tests/test_manifold_ref_host.py proves the reference and the premises on the
CPU): one graph of disjoint vertex pairs per manifold, one edge per case.  The rule is the project's referee rule per case
and per output array: with errors measured against the long-double reference as max |x - ref| / max(1, max |ref|),

    e_gpu <= max(8 e_oracle, floor)

e_oracle being the fp64 oracle's own error on that case (oracle/pg_oracle.c, tests/np_ref_se2.py) and the floors the
tolerances the suite already holds this math to: 1e-13 residuals, 1e-12 Jacobians (and J^T J, J^T r, scaled by
max(1, |J|max^2)), rtol 1e-13 + atol 1e-15 retracted poses.  Every test prints one MANIFOLD line: per band of the angle,
the worst e_gpu, e_oracle and device-versus-oracle difference (DESIGN.md section 2 quotes them)."""
import functools

import numpy as np
import pytest

import manifold_ref as mr
import np_ref_se2 as ref2
from apex_solver_amd.pose_graph import GpuSparseCholeskySolver, PoseGraphProblem
from apex_solver_amd.solver import GpuSchurComplementSolver, OptimizationType, Problem
from oracle import pg_oracle as po

pytestmark = pytest.mark.gpu
LD = mr.LD


def solver(prob, poses=None):
    s = GpuSparseCholeskySolver(0).initialize_structure(prob)
    s.set_parameters(prob.data.poses if poses is None else poses)
    return s


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


def check(tag, what, labels, e_gpu, e_oracle, floor):
    ok, at = mr.referee(e_gpu, e_oracle, floor)
    assert ok, (tag, what, labels[at] if labels is not None else at, "e_gpu", float(np.atleast_1d(e_gpu)[at]),
                "e_oracle", float(np.atleast_1d(e_oracle)[at]), "floor", floor)


def between_edges(name, data, dof):
    cs, r, J, ro, Jo = data
    n = len(r)
    d = mr.graph_of(cs)
    for delta in (None, mr.HUBER_DELTA):
        tag = f"{name} between {'huber' if delta else 'no loss'}"
        prob = PoseGraphProblem.pose_graph(d, delta)
        s = solver(prob)
        gr, gJ, cost = s.get_residual(), s.get_jacobian_blocks(), s.compute_cost()
        H, g = s.get_hessian(0.0)
        s.close()
        sc = mr.huber_scale(delta, (r * r).sum(-1))
        rr, JJ = r * sc[:, None], J * sc[:, None, None]
        sco = ref2.huber_scale(delta, np.einsum("ei,ei->e", ro, ro))
        rro, JJo = ro * sco[:, None], Jo * sco[:, None, None]
        if delta:
            assert (sc < 1).sum() >= 8 and (sc == 1).sum() >= 2          # both sides of the loss: at least the edges at the threshold
        e_r, o_r, e_J, o_J = mr.err(gr, rr), mr.err(rro, rr), mr.err(gJ, JJ), mr.err(JJo, JJ)
        # J^T J and J^T r per edge, formed in long double from the reference blocks; the lower triangle of the device's H
        cols = np.concatenate([prob.pose_col[d.e_from][:, None] + np.arange(dof)[None], prob.pose_col[d.e_to][:, None] + np.arange(dof)[None]], axis=1)
        Href = np.swapaxes(JJ, -1, -2) @ JJ
        gref = (np.swapaxes(JJ, -1, -2) @ rr[:, :, None])[:, :, 0]
        Ho = np.swapaxes(JJo, -1, -2) @ JJo
        go = np.einsum("eij,ei->ej", JJo, rro)
        scale = np.maximum(1.0, np.abs(JJ.astype(np.float64)).reshape(n, -1).max(-1) ** 2)
        Hg = np.stack([H[np.ix_(cols[e], cols[e])] for e in range(n)])
        low = cols[:, :, None] >= cols[:, None, :]                           # the entries of a block in H's lower triangle
        e_H = (np.abs(Hg.astype(LD) - Href) * low).reshape(n, -1).max(-1).astype(np.float64) / scale
        o_H = (np.abs(Ho.astype(LD) - Href) * low).reshape(n, -1).max(-1).astype(np.float64) / scale
        e_g = np.abs(g[cols].astype(LD) - gref).max(-1).astype(np.float64) / scale
        o_g = np.abs(go.astype(LD) - gref).max(-1).astype(np.float64) / scale
        rest = np.tril(H).copy()
        for e in range(n):
            rest[np.ix_(cols[e], cols[e])] = 0.0
        cref = 0.5 * (rr * rr).sum()
        e_c = float(abs(LD(cost) - cref) / max(LD(1), cref)); o_c = float(abs(LD(0.5 * np.sum(rro * rro)) - cref) / max(LD(1), cref))
        mr.report(tag, cs["angle"], gpu_r=e_r, ora_r=o_r, dev_vs_ora_r=mr.err(gr, rro), gpu_J=e_J, ora_J=o_J, dev_vs_ora_J=mr.err(gJ, JJo),
                  gpu_H=e_H, ora_H=o_H, gpu_g=e_g, ora_g=o_g)
        print(f"MANIFOLD {tag}: cost e_gpu={e_c:.1e} e_oracle={o_c:.1e}")
        assert np.isfinite(gr).all() and np.isfinite(gJ).all() and np.isfinite(H).all()
        check(tag, "residual", cs["label"], e_r, o_r, mr.FLOOR_R)
        check(tag, "jacobian", cs["label"], e_J, o_J, mr.FLOOR_J)
        check(tag, "hessian", cs["label"], e_H, o_H, mr.FLOOR_H)
        check(tag, "gradient", cs["label"], e_g, o_g, mr.FLOOR_H)
        check(tag, "cost", None, e_c, o_c, mr.FLOOR_R)
        assert not rest.any(), "H has entries outside the edges' blocks"


def test_se3_between_edges():
    between_edges("se3", se3(), 6)


def test_se2_between_edges():
    between_edges("se2", se2(), 3)


def retraction_bands(name, cases, plus, oracle_plus, dof, rot):
    prob, scal = mr.retraction_problem(cases)
    free = ~prob.fix.astype(bool).all(axis=1)
    vcols = prob.pose_col[:, None] + np.arange(dof)[None]
    labels = [f"vertex {v} ({cases['label'][v // 2]})" for v in range(prob.data.n_v)]

    def solved():
        s = solver(prob)
        s.apply_column_scaling(scal)
        y = s.solve_augmented_equation(mr.RETRACT_LAMBDA).copy()
        d = (y * scal)[vcols]                     # the unscaled step (scal holds powers of two: exact)
        d[~free] = 0.0                            # fixed DOF are zeroed when the step is applied
        return s, d

    s, d = solved()
    p0 = s.get_parameters()
    s.eval_step(); s.commit_step()
    got = s.get_parameters()
    s.close()
    norm = np.linalg.norm(d[:, rot], axis=1)
    counts = np.bincount(mr.band_of(norm[free]), minlength=5)
    assert (counts >= 8).all(), counts
    want = plus(p0, d)
    e_gpu, e_ora = mr.err(got, want), mr.err(oracle_plus(p0, d), want)
    mr.report(f"{name} retraction commit", norm[free], gpu=e_gpu[free], oracle=e_ora[free], dev_vs_ora=mr.err(got, oracle_plus(p0, d))[free])
    check(name, "committed poses", labels, e_gpu, e_ora, mr.FLOOR_POSE)
    assert np.array_equal(got[~free], p0[~free])
    # a rejected step on a fresh handle: x (+) d (+) -d
    s, d = solved()
    p0 = s.get_parameters()
    s.eval_step(); s.discard_step()
    back = s.get_parameters()
    s.close()
    want = plus(plus(p0, d), -d)
    e_gpu, e_ora = mr.err(back, want), mr.err(oracle_plus(oracle_plus(p0, d), -d), want)
    mr.report(f"{name} retraction discard", np.linalg.norm(d[:, rot], axis=1)[free], gpu=e_gpu[free], oracle=e_ora[free])
    check(name, "poses after a discarded step", labels, e_gpu, e_ora, mr.FLOOR_POSE)
    return p0, got, free


def _pgo_plus(p, d):
    return np.array([po.call("pgo_se3_plus", p[v], d[v], out_shape=7) for v in range(len(p))])


def test_se3_retraction_bands():
    retraction_bands("se3", se3()[0], mr.se3_plus, _pgo_plus, 6, slice(3, 6))


def test_se2_retraction_bands():
    p0, got, free = retraction_bands("se2", se2()[0], mr.se2_plus, ref2.plus, 3, slice(2, 3))
    crossed = (np.sign(got[free, 2]) != np.sign(p0[free, 2])) & (np.abs(got[free, 2]) > 3.0) & (np.abs(p0[free, 2]) > 3.0)
    assert crossed.sum() >= 2 and ((got[:, 2] > -np.pi) & (got[:, 2] <= np.pi)).all()      # theta was carried across +-pi


def test_ba_camera_retraction_bands(oracle):
    d = mr.ba_band_problem()
    prob = Problem.bundle_adjustment(d, OptimizationType.OnlyPose)
    s = GpuSchurComplementSolver(0).initialize_structure(prob)
    s.set_parameters(d.poses, d.intr, d.points)
    s.solve_augmented_equation(mr.BA_LAMBDA)
    step, _ = s.export_step()
    p0 = s.get_parameters()[0]
    s.eval_step(); s.commit_step()
    got = s.get_parameters()[0]
    s.close()
    dd = step[prob.layout.pose_col[:, None] + np.arange(6)[None]]
    dd = np.where(prob.fix_pose.astype(bool), 0.0, dd)
    free = ~prob.fix_pose.astype(bool).all(axis=1)
    norm = np.linalg.norm(dd[:, 3:], axis=1)
    counts = np.bincount(mr.band_of(norm[free]), minlength=5)
    print("MANIFOLD ba camera bands populated:", dict(zip(mr.BAND_NAMES, counts.tolist())))
    assert (counts > 0).sum() >= 3, counts
    want = mr.se3_plus(p0, dd)
    ora = np.zeros_like(p0)
    for c in range(len(p0)):
        oracle.lib().ora_se3_plus(np.ascontiguousarray(p0[c]), np.ascontiguousarray(dd[c]), ora[c])
    e_gpu, e_ora = mr.err(got, want), mr.err(ora, want)
    mr.report("ba camera retraction", norm[free], gpu=e_gpu[free], oracle=e_ora[free], dev_vs_ora=mr.err(got, ora)[free])
    check("ba", "committed camera poses", [f"camera {c}" for c in range(len(p0))], e_gpu, e_ora, mr.FLOOR_POSE)
    assert np.array_equal(got[~free], p0[~free])
