"""The Schur assembly (k_cam_reduce, k_landmark_reduce, k_schur_pairs_r in both list layouts, k_build_pair_recs_q,
k_back_substitute, k_implicit_cam) on crafted co-visibility structures (tests/schur_cases.py) against the long double
reference of tests/schur_ref.py, camera pair by camera pair: err_ij <= max(8 e_np_ij, gamma(P_ij) M_ij).  The premises of
every structure -- pieces, flags, carried heads, joins, tasks -- are asserted on the host lists by
tests/test_schur_ref_host.py.  Every case prints one SCHURREF line with the worst ratio of each checked quantity."""
import numpy as np
import pytest

import schur_cases as sc
import schur_ref as sr
from apex_solver_amd import capi
from apex_solver_amd.solver import GpuSchurComplementSolver, OptimizationType, Problem

pytestmark = pytest.mark.gpu
FORMS = {"selfcal": (4, 3), "ba": (3,)}
CASES = [(name, mode, form) for name in sc.DENSE_CASES for mode in sc.structure(name)[3] for form in FORMS[mode]]
_REF = {}     # (case, mode) -> (jc, jl, r, long double reference, fp64 restatement): one reference for both layouts


def _solver(d, mode, **options):
    ot = OptimizationType.SelfCalibration if mode == "selfcal" else OptimizationType.BundleAdjustment
    prob = Problem(d, ot, 1.0)                      # nothing fixed: the step is the solution of the damped system as it stands
    s = GpuSchurComplementSolver(0)
    for k, v in options.items():
        s.with_option(k, v)
    s.initialize_structure(prob)
    s.set_parameters(d.poses, d.intr, d.points)
    return prob, s


def _reference(key, d, s, lam, dense=True):
    jc, jl = s.get_jacobian_blocks()
    r = s.get_residual()
    if key in _REF:
        assert np.array_equal(_REF[key][0], jc) and np.array_equal(_REF[key][1], jl) and np.array_equal(_REF[key][2], r)
    else:
        _REF[key] = (jc, jl, r) + sr.pair(d.n_cam, d.n_pt, d.cam_idx, d.pt_idx, jc, jl, r, lam, dense=dense)
    ld, f64 = _REF[key][3:]
    assert ld.cond.max() <= 1e8, ld.cond.max()     # every landmark in the plain-inverse regime of the gate
    return ld, f64


def _vector_checks(ld, f64, cols, gred, hinv, gl):
    return dict(gred=sr.vec_check(gred[cols], ld.gred, f64.gred, ld.gred_mag, ld.gred_terms),
                hinv=sr.vec_check(hinv, ld.Hinv, f64.Hinv, ld.hinv_mag, ld.k_l),
                gl=sr.vec_check(gl, ld.gl, f64.gl, ld.gl_mag, ld.k_l))


def _matvec_checks(s, ld, f64, cols, lam, n, seed=3):
    x = np.random.default_rng(seed).normal(size=n)
    ye, yi = s.schur_matvec(lam, x)
    y_ld, mag = ld.matvec(x[cols])
    y_64, _ = f64.matvec(x[cols])
    rest = np.setdiff1d(np.arange(n), cols.ravel())          # six columns: the intrinsics exist, no factor touches them: S = lambda
    assert np.array_equal(ye[rest], lam * x[rest]) and np.array_equal(yi[rest], lam * x[rest])
    terms = ld.matvec_terms()
    return dict(mv_explicit=sr.vec_check(ye[cols], y_ld, y_64, mag, terms), mv_implicit=sr.vec_check(yi[cols], y_ld, y_64, mag, terms))


@pytest.mark.parametrize("name,mode,form", CASES, ids=[f"{n}-{m}-form{f}" for n, m, f in CASES])
def test_crafted_structure(name, mode, form):
    n_cam, lists, lam, _ = sc.structure(name)
    d = sc.problem(name)
    dc = 9 if mode == "selfcal" else 6
    prob, s = _solver(d, mode, schur_form=form)
    assert s.info()["schur_form"] == form
    lay, n = prob.layout, prob.layout.cam_dof
    cols = sr.cam_cols(lay, n_cam, dc)
    step = s.solve_augmented_equation(lam)
    S, gred = s.get_schur()
    S, gred = S.copy(), gred.copy()
    hinv, gl = s.get_landmark_blocks()
    ld, f64 = _reference((name, mode), d, s, lam)

    # every block of S; pairs of cameras without a common landmark exactly zero; S exactly symmetric
    S4 = sr.blocks_of(S, cols)
    ratios = {}
    ratios["S"], bad = sr.block_check(S4, ld, f64)
    ratios.update(_vector_checks(ld, f64, cols, gred, hinv, gl))
    # back-substitution on its own: the device's camera step through the reference's back-substitution
    dcam = step[cols]
    dl_ld, dl_mag = ld.back_substitute(dcam)
    dl_64, _ = f64.back_substitute(dcam)
    ratios["dl"] = sr.vec_check(step[lay.pt_col[:, None] + np.arange(3)[None]], dl_ld, dl_64, dl_mag, 2 * ld.k_l)
    ratios.update(_matvec_checks(s, ld, f64, cols, lam, n))
    # a second assembly on the same handle: the same bits unless a block adds atomically, and within the bound then
    S2, g2 = s.get_schur()
    ci, pi = d.cam_idx, d.pt_idx
    pl = capi.pair_lists_queued(n_cam, d.n_pt, ci, pi, 9) if form == 4 else capi.pair_lists(n_cam, d.n_pt, dc, ci, pi)
    atomic = bool(len(pl["blocks"])) and bool((pl["blocks"][:, 3] & 1).any())
    ratios["S_again"], bad2 = sr.block_check(sr.blocks_of(S2, cols), ld, f64)
    sr.report(f"{name} {mode} form {form}" + (" (atomic)" if atomic else ""), ratios)
    s.close()

    assert not bad, [(b, float(ratios["S"][b]), int(ld.P[b])) for b in bad[:8]]
    assert (S4[(ld.P == 0) & ~np.eye(n_cam, dtype=bool)] == 0.0).all()     # (a camera nobody observes keeps lambda I on its diagonal block)
    assert np.array_equal(S, S.T)
    rest = np.setdiff1d(np.arange(n), cols.ravel())
    off = S.copy(); off[rest, rest] = 0.0
    assert (S[rest, rest] == lam).all() and not off[rest].any() and not off[:, rest].any()
    for k in ("gred", "hinv", "gl", "dl", "mv_explicit", "mv_implicit"):
        v, at = sr.worst(ratios[k])
        assert v <= 1.0, (k, v, at)
    assert not bad2, [(b, float(ratios["S_again"][b])) for b in bad2[:8]]
    if not atomic:
        assert np.array_equal(S, S2) and np.array_equal(gred, g2)


def test_wide_row():
    """A row of S with more than kRecsLdsPartners = 2048 partners: k_build_pair_recs_q counts in global memory there.  The device's
    records are the host's slot for slot; assembly only, no dense S: g_red, H_ll^-1, g_l and both forms of S x against the
    reference's matrix-free product."""
    n_cam, lists, lam, _ = sc.structure("wide")
    d = sc.problem("wide")
    recs = []
    for dev in (0, 1):
        # (S is dense at tile granularity here, 129 tile rows: the cost rule would hand this structure to the matrix-free PCG and
        # build no pair list at all; it is switched off)
        prob, s = _solver(d, "selfcal", device_pair_list=dev, variant_cost_permille=0)
        assert s.variant_info()["variant_used"] == "Sparse" and s.info()["schur_form"] == 4
        recs.append(s.pair_records())
        if dev == 0:
            s.close()
    assert recs[0].shape == recs[1].shape and recs[0].shape[0] % 64 == 0
    real = [r[:, 0] != 0xFFFFFFFF for r in recs]       # (a padding slot is padding by its first word; the rest of it is not read)
    assert int(real[0].sum()) == sum(len(c) * (len(c) - 1) // 2 for c in lists)
    assert np.array_equal(real[0], real[1]) and np.array_equal(recs[0][real[0]], recs[1][real[1]])
    lay, n = prob.layout, prob.layout.cam_dof
    cols = sr.cam_cols(lay, n_cam, 9)
    s.assemble(lam)
    _, gred = s.get_schur(want_S=False)
    hinv, gl = s.get_landmark_blocks()
    ld, f64 = _reference(("wide", "selfcal"), d, s, lam, dense=False)
    ratios = _vector_checks(ld, f64, cols, gred, hinv, gl)
    ratios.update(_matvec_checks(s, ld, f64, cols, lam, n))
    sr.report("wide selfcal form 4", ratios)
    s.close()
    for k, r in ratios.items():
        v, at = sr.worst(r)
        assert v <= 1.0, (k, v, at)
