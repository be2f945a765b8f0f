"""Every device form of the BAL projection factor on the crafted observations of tests/projection_cases.py against the long
double reference of tests/projection_ref.py, entry by entry: err <= max(8 e_np, gamma(k) M), schur_ref.vec_check's rule with
the reference's own magnitudes.  The reference, the bounds and every premise of the cases are proven on the CPU by
tests/test_projection_ref_host.py against the host build of the same header.

Isolated scenes (observation i = camera i = landmark i; nothing is assembled or solved): linearize_obs through
get_residual / get_jacobian_blocks / compute_column_norms, jv_obs through jv_gram, residual_obs through compute_cost, before and
after a second set_parameters, for every OptimizationType and every loss.  Braced scenes (every H_ll + lambda I and S with
cond <= 1e8, asserted on the reference before any device call): H_ll^-1, g_l, every block of S, g_red and both forms of S x
against schur_ref fed with the REFERENCE's blocks -- which ties the projection record (jac_from_rec, rec_inz, the w = 0 record
of an invalid observation) to the truth --, then one solve: the landmark step through the reference's back-substitution of the
device's camera step, and eval_step against the long double cost at the retracted point to 1e-9, with eager_step_eval on and off.

After assemble() the back-substitution always reads the projection records, so the general (linearize_obs) form of
k_back_substitute is not run by these tests: both settings of eager_step_eval go through k_back_substitute<REC = true>, with and
without the pts_trial write.

Every bound is vec_check's / block_check's own with the term counts of the issue: an entry's own sum (projection_ref.TERMS: 2 for
r, 3 for Jl, 6 for Jc), 2 for a column norm and for a unit-vector Gram value, 2 n N for the random-vector Gram, n for the cost;
C0 = 114 unchanged, so every floor is gamma(116 .. 400) M.  No form needed a larger factor.  The one multiplier beside the rule
is schur_ref.SchurRef's `mags` factor kap on H_ll^-1 alone, the relative magnitude of H_ll itself from the reference's M_Jl
(reasoned there, not fitted): between 1 and 763 on these scenes (printed by tests/test_projection_ref_host.py).  Measured on an MI355X, worst ratio
err / bound over all scenes, modes and losses: r 1.4e-2, Jc 3.7e-2, Jl 3.0e-2, column norms 3.0e-2, unit-vector Gram 5.9e-2,
random-vector Gram 1.7e-4, cost 2.4e-2 (5.9e-2 at the second point); braced scenes S 4.9e-2, g_red 1.3e-2, H_ll^-1 2.5e-2,
g_l 8.4e-3, S x 2.9e-2 (both forms), landmark step 2.2e-2, trial cost 4.5e-13 relative.  The floor of an entry's bound is about
120 roundings of its magnitude: it separates a wrong formula, sign, mask or classification from a right one, and an error of
a few tens of roundings (a reciprocal short of a Newton step, ~1e-14) only on the entries that carry no cancellation.
Every test prints PROJREF lines with the worst ratio of each checked quantity."""
import numpy as np
import pytest

import np_ref
import projection_cases as pc
import projection_ref as pr
import schur_ref as sr
from apex_solver_amd.solver import GpuSchurComplementSolver, Problem
from tile_ref import LD

pytestmark = pytest.mark.gpu
SCENES = list(pc.SCENES)
BRACED_LOSSES = ("huber_delta", "tukey")
BRACED = [(sc, mode, form, eager) for sc in SCENES for mode, (_, dc, _) in pc.MODES.items() for form in ((4, 3) if dc == 9 else (3,))
          for eager in (1, 0)]
_REFS = {}


def refs(d, key, loss, params=None):
    if key not in _REFS:
        p = params if params is not None else (d.poses, d.intr, d.points)
        a = (*p, d.cam_idx, d.pt_idx, d.obs_uv)
        _REFS[key] = (pr.reference(*a, loss=loss), pr.restatement(*a, loss=loss))
    return _REFS[key]


def _solver(d, mode, **options):
    prob = Problem(d, pc.MODES[mode][0], pc.SCALE)      # nothing fixed; the legacy huber_delta until a set_loss
    s = GpuSchurComplementSolver(0)
    for k, v in options.items():
        s.with_option(k, v)
    s.initialize_structure(prob)
    s.set_parameters(d.poses, d.intr, d.points)
    return prob, s


def _set_loss(s, loss):
    if not isinstance(loss, tuple):          # (the legacy double is what initialize_structure left)
        s.set_loss(loss)


def _scalar_ratio(dev, ld, f64, mag, terms):
    return sr.vec_check(np.array([dev]), np.array([ld], dtype=LD), np.array([f64]), np.array([mag]), terms)


def _columns(lay, n, dc):
    """(n, dc + 3) global columns of observation i's [camera | landmark] entries in an isolated scene"""
    cols = sr.cam_cols(lay, n, dc)
    return np.concatenate([cols, lay.pt_col[:n, None] + np.arange(3)[None]], axis=1)


def _gram(J, a, b):
    """(|J a|^2, J a . J b, |J b|^2) over all observations; J (n, 2, N), a, b (n, N)"""
    u, w = np.einsum("krc,kc->kr", J, a), np.einsum("krc,kc->kr", J, b)
    return np.array([(u * u).sum(), (u * w).sum(), (w * w).sum()])


def _gram_check(s, total, cols, ld, f64, a, b, terms):
    av, bv = np.zeros(total), np.zeros(total)
    av[cols] = a; bv[cols] = b
    dev = np.array(s.jv_gram(av, bv))
    J = lambda r, pre="": np.concatenate([getattr(r, pre + "Jc"), getattr(r, pre + "Jl")], axis=2)
    g_ld = _gram(J(ld).astype(LD), a.astype(LD), b.astype(LD))
    g_64 = _gram(np.asarray(J(f64), dtype=np.float64), a, b)
    mag = _gram(J(ld, "M_"), np.abs(a), np.abs(b))
    mag[1] = np.sqrt(mag[0] * mag[2])
    return dev, sr.vec_check(dev, g_ld, g_64, np.maximum(mag, 0.0), terms)


@pytest.mark.parametrize("mode", list(pc.MODES))
@pytest.mark.parametrize("scene", SCENES)
def test_isolated_scene(scene, mode):
    d, obs = pc.isolated(scene)
    _, dc, mask = pc.MODES[mode]
    n = d.n_obs
    prob, s = _solver(d, mode)
    lay, total = prob.layout, prob.total_dof
    cols = _columns(lay, n, dc)
    p2 = pc.second_point(d)
    rng = np.random.default_rng(11)
    a_rand, b_rand = rng.normal(size=(n, dc + 3)), rng.normal(size=(n, dc + 3))
    cm = np.array([mask & 4] * 6 + [mask & 1] * 3)[:dc] != 0
    worst, failures = {}, []
    for lname, loss in pc.LOSSES.items():
        ld7, f647 = refs(d, ("iso", scene, lname), loss)
        ld, f64 = pr.masked(ld7, mask, dc), pr.masked(f647, mask, dc)
        _set_loss(s, loss)
        s.set_parameters(d.poses, d.intr, d.points)
        r = s.get_residual().reshape(n, 2)
        jc, jl = s.get_jacobian_blocks()
        ratios = dict(r=pr.entry_ratio(r, ld, f64, "r"), Jc=pr.entry_ratio(jc, ld, f64, "Jc"), Jl=pr.entry_ratio(jl, ld, f64, "Jl"))
        inv = ~ld.valid
        assert not r[inv].any() and not jc[inv].any() and not jl[inv].any(), (lname, "invalid observations are exact zeros")
        assert not jc[:, :, ~cm].any() and (mask & 2 or not jl.any()), (lname, "masked columns are exact zeros")
        # column norms: each column is touched by one observation
        J = lambda x, pre="": np.concatenate([getattr(x, pre + "Jc"), getattr(x, pre + "Jl")], axis=2)
        nrm = lambda x: np.sqrt((x * x).sum(axis=1))
        norms = s.compute_column_norms()
        ratios["norms"] = sr.vec_check(norms[cols].reshape(-1), nrm(J(ld).astype(LD)).reshape(-1), nrm(np.asarray(J(f64), dtype=np.float64)).reshape(-1),
                                       nrm(J(ld, "M_")).reshape(-1), 2).reshape(n, dc + 3)       # (a column's norm: two terms)
        rest = np.setdiff1d(np.arange(total), cols.ravel())
        assert not norms[rest].any()
        # jv_gram, observation by observation: a = e_c, b = e_(N-1-c) over every column c of the observation's [Jc | Jl] (every
        # entry of jv_obs' Jacobian is seen as a and as b; each Gram value is a sum of two terms), then two random vectors
        # over the whole scene (2 n rows of N terms each)
        N = dc + 3
        Jl_, J6, JM = J(ld).astype(LD), np.asarray(J(f64), dtype=np.float64), J(ld, "M_")
        pair = lambda X: np.stack([(X * X).sum(axis=1), (X * X[:, :, ::-1]).sum(axis=1), (X[:, :, ::-1] * X[:, :, ::-1]).sum(axis=1)], -1)
        dev = np.zeros((n, N, 3))
        for o in range(n):
            for c in range(N):
                av, bv = np.zeros(total), np.zeros(total)
                av[cols[o, c]] = 1.0; bv[cols[o, N - 1 - c]] = 1.0
                dev[o, c] = s.jv_gram(av, bv)
        ratios["jv_unit"] = sr.vec_check(dev.reshape(-1), pair(Jl_).reshape(-1), pair(J6).reshape(-1), pair(JM).reshape(-1), 2).reshape(n, N, 3)
        assert not dev[inv].any(), (lname, "jv_obs linearises an observation linearize_obs refuses")
        kJ = 2 * n * N
        ratios["jv_gram"] = _gram_check(s, total, cols, ld, f64, a_rand, b_rand, kJ)[1]
        # the validity decisions coincide form by form: zero Gram rows exactly where the rows of J are zero
        if inv.any():
            a0 = a_rand * inv[:, None]
            dev0, _ = _gram_check(s, total, cols, ld, f64, a0, b_rand, kJ)
            assert dev0[0] == 0.0 and dev0[1] == 0.0, (lname, "jv_obs linearises an observation linearize_obs refuses", dev0)
        # cost here and at a second point (cameras prepared afresh); a cost term the rows do not have would show in both
        c_ld, c_mag, c_terms = pr.cost_terms(ld)
        c_64 = 0.5 * float((f64.r * f64.r).sum())
        ratios["cost"] = _scalar_ratio(s.compute_cost(), c_ld, c_64, c_mag, c_terms)
        ld2, f642 = refs(d, ("iso2", scene, lname), loss, p2)
        s.set_parameters(*p2)
        c_ld, c_mag, c_terms = pr.cost_terms(ld2)
        ratios["cost_2"] = _scalar_ratio(s.compute_cost(), c_ld, 0.5 * float((f642.r * f642.r).sum()), c_mag, c_terms)
        for q, v in ratios.items():
            val, at = sr.worst(v)
            if val >= worst.get(q, (-1.0,))[0]:
                worst[q] = (val, lname, at)
            if not val <= 1.0:
                failures.append((lname, q, val, at, obs[at[0]].name if q in ("r", "Jc", "Jl", "norms", "jv_unit") else ""))
    s.close()
    print(f"PROJREF isolated {scene} {mode}: " + "  ".join(f"{q} {v[0]:.3g}@{v[1]},{','.join(map(str, v[2]))}" for q, v in worst.items()))
    assert not failures, failures[:10]


@pytest.mark.parametrize("scene,mode,form,eager", BRACED, ids=[f"{a}-{b}-form{c}-eager{e}" for a, b, c, e in BRACED])
def test_braced_scene(scene, mode, form, eager):
    d, edge, obs = pc.braced(scene)
    _, dc, mask = pc.MODES[mode]
    lam = pc.LAMBDA
    prob, s = _solver(d, mode, schur_form=form, eager_step_eval=eager)
    assert s.info()["schur_form"] == form
    lay, n = prob.layout, prob.layout.cam_dof
    cols = sr.cam_cols(lay, d.n_cam, dc)
    failures = []
    for lname in BRACED_LOSSES:
        loss = pc.LOSSES[lname]
        ld7, f647 = refs(d, ("braced", scene, lname), loss)
        key = ("braced-schur", scene, lname, mode)
        if key not in _REFS:
            _REFS[key] = pr.schur_pair(d, ld7, f647, dc, mask, lam)
        ld, f64 = _REFS[key]
        S_ld = np.asarray(sr.dense_of(ld.S4, np.arange(d.n_cam * dc).reshape(d.n_cam, dc), d.n_cam * dc), dtype=np.float64)
        assert ld.cond.max() <= 1e8 and np.linalg.cond(S_ld) <= 1e8          # before any device call on this system
        _set_loss(s, loss)
        s.set_parameters(d.poses, d.intr, d.points)
        s.assemble(lam)
        hinv, gl = s.get_landmark_blocks()
        S, gred = s.get_schur()
        S, gred = S.copy(), gred.copy()
        ratios = {}
        ratios["S"], bad = sr.block_check(sr.blocks_of(S, cols), ld, f64)
        ratios["gred"] = sr.vec_check(gred[cols], ld.gred, f64.gred, ld.gred_mag, ld.gred_terms)
        ratios["hinv"] = sr.vec_check(hinv, ld.Hinv, f64.Hinv, ld.hinv_mag, ld.k_l)
        ratios["gl"] = sr.vec_check(gl, ld.gl, f64.gl, ld.gl_mag, ld.k_l)
        x = np.random.default_rng(3).normal(size=n)
        ye, yi = s.schur_matvec(lam, x)
        y_ld, mag = ld.matvec(x[cols]); y_64, _ = f64.matvec(x[cols])
        terms = ld.matvec_terms()
        ratios["mv_explicit"] = sr.vec_check(ye[cols], y_ld, y_64, mag, terms)
        ratios["mv_implicit"] = sr.vec_check(yi[cols], y_ld, y_64, mag, terms)
        if lname == BRACED_LOSSES[0]:
            step = s.solve_augmented_equation(lam)
            dl_ld, dl_mag = ld.back_substitute(step[cols])
            dl_64, _ = f64.back_substitute(step[cols])
            ratios["dl"] = sr.vec_check(step[lay.pt_col[:, None] + np.arange(3)[None]], dl_ld, dl_64, dl_mag, 2 * ld.k_l)
            trial = s.eval_step()
            at = np_ref.retract(d.poses, d.intr, d.points, step, lay)
            ref_t = pr.reference(*at, d.cam_idx, d.pt_idx, d.obs_uv, loss=loss)
            zt = np.asarray(ref_t.pc[:, 2], dtype=np.float64)        # the trial point classifies unambiguously too
            assert (np.abs(zt + 1e-6) >= 1e3 * 2.0 ** -53 * np.asarray(ref_t.M_z, dtype=np.float64)).all()
            t_ld = pr.cost_terms(ref_t)[0]
            rel = abs(trial - float(t_ld)) / float(t_ld)
            print(f"PROJREF braced {scene} {mode} form {form} eager {eager}: trial cost rel {rel:.3g}")
            if not rel <= 1e-9:
                failures.append((lname, "trial", rel))
            s.discard_step()
        pr.report(f"braced {scene} {mode} form {form} eager {eager} {lname}", ratios)
        if bad:
            failures.append((lname, "S", [(b, float(ratios["S"][b])) for b in bad[:6]]))
        for q, v in ratios.items():
            if q != "S" and not sr.worst(v)[0] <= 1.0:
                failures.append((lname, q) + sr.worst(v))
    s.close()
    assert not failures, failures[:10]
