"""The reference of the projection factor (tests/projection_ref.py) and the crafted observations (tests/projection_cases.py),
proven without a GPU:

  * the long double reference against central finite differences of its own residual, taken in long double with a step per
    column, to 1e-6 of the column's size (plus 1e-12 of the block's, for the columns that are exactly zero) on every valid
    observation of every class -- a reference wrong in the same way as the kernels does not pass this;
  * the fp64 restatement classifies like the reference and stays within the rule;
  * the host build of apex-solver_amd/csrc/ba_device.hpp (tests/host_harness_projection.cpp: linearize_obs, residual_obs, jv_obs, each
    mask, width, template form and loss) within err <= max(8 e_np, gamma(k) M) per entry on every case: the inputs leave the
    reference alone inside the bound;
  * every premise of every case: classification margins, finite inputs and outputs, and on the braced scenes cond(H_ll + lambda I)
    <= 1e8 and cond(S) <= 1e8.
Every test prints PROJREF lines with the worst ratio of each checked quantity."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import projection_cases as pc
import projection_ref as pr
import schur_ref as sr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_f = np.ctypeslib.ndpointer(dtype=np.float64, flags="C_CONTIGUOUS")
SCENES = list(pc.SCENES)
BRACED_LOSSES = ("huber_delta", "tukey")
WIDTHS = [(dc, mask, masked) for dc in (6, 9) for mask in range(1, 8) for masked in (1, 0) if masked or mask == (7 if dc == 9 else 6)]


@pytest.fixture(scope="module")
def hp():
    out = os.path.join(ROOT, "tests", "_build")
    os.makedirs(out, exist_ok=True)
    so = os.path.join(out, "libhost_harness_projection.so")
    subprocess.run(["g++", "-O2", "-ffp-contract=off", "-std=c++17", "-shared", "-fPIC", "-I", os.path.join(ROOT, "apex-solver_amd", "csrc"),
                    os.path.join(ROOT, "tests", "host_harness_projection.cpp"), "-o", so], check=True)
    L = C.CDLL(so)
    L.hp_linearize.argtypes = [C.c_int, C.c_int, C.c_int, _f, _f, _f, _f, C.c_int, C.c_double, C.c_double, _f, _f, _f, _f]
    L.hp_residual.argtypes = [_f, _f, _f, _f, C.c_int, C.c_double, C.c_double, _f]
    L.hp_jv.argtypes = [C.c_int, C.c_int, C.c_int, _f, _f, _f, _f, C.c_int, C.c_double, C.c_double, _f, _f, _f, _f]
    return L


def _kind(loss):
    """(kind, p0, p1) of the harness: kind < 0 is the huber_delta form"""
    if loss is None:
        return -1, -1.0, 0.0
    if isinstance(loss, tuple):
        return -1, float(loss[1]), 0.0
    return int(loss.kind), float(loss.p0), float(loss.p1)


_REFS = {}


def braced_system(d, ld, f64, dc, mask):
    return pr.schur_pair(d, ld, f64, dc, mask, pc.LAMBDA)


def refs(d, key, loss):
    """(long double reference, fp64 restatement) at mask 7, dc 9, once per (scene, loss)"""
    if key not in _REFS:
        a = (d.poses, d.intr, d.points, d.cam_idx, d.pt_idx, d.obs_uv)
        _REFS[key] = (pr.reference(*a, loss=loss), pr.restatement(*a, loss=loss))
    return _REFS[key]


def host_linearize(hp, d, loss, dc, mask, masked):
    """(valid, r, Jc, Jl, rec) of hp_linearize on every observation of d"""
    n = len(d.cam_idx)
    ok = np.zeros(n, dtype=bool); r = np.zeros((n, 2)); Jc = np.zeros((n, 2, dc)); Jl = np.zeros((n, 2, 3)); rec = np.zeros((n, 4))
    k = _kind(loss)
    for i in range(n):
        c, l = int(d.cam_idx[i]), int(d.pt_idx[i])
        rc = hp.hp_linearize(dc, masked, mask, d.poses[c], d.intr[c], d.points[l], d.obs_uv[i], *k, r[i], Jc[i].reshape(-1), Jl[i].reshape(-1), rec[i])
        assert rc in (0, 1), (rc, loss)
        ok[i] = bool(rc)
    return ok, r, Jc, Jl, rec


@pytest.mark.parametrize("scene", SCENES)
def test_reference_matches_its_own_finite_differences(scene):
    d, obs = pc.isolated(scene)
    ld, _ = refs(d, ("iso", scene, "none"), None)
    worst = 0.0
    n_valid = 0
    for i, o in enumerate(obs):
        if not ld.valid[i]:
            continue
        n_valid += 1
        fd = pr.finite_differences(d.poses[i], d.intr[i], d.points[i])
        J = np.concatenate([ld.Jc[i], ld.Jl[i]], axis=1)                    # w = 1: no loss
        for lo, hi in ((0, 3), (3, 6), (6, 9), (9, 12)):
            blk = np.abs(J[:, lo:hi]).max()
            tol = 1e-6 * np.abs(J[:, lo:hi]).max(axis=0) + 1e-12 * blk
            err = np.abs(fd[:, lo:hi] - J[:, lo:hi]).max(axis=0)
            worst = max(worst, float((err[tol > 0] / tol[tol > 0]).max(initial=0.0)))
            assert (err <= tol).all(), (o.name, lo, err, tol)
    assert n_valid == sum(o.valid for o in obs)
    print(f"PROJREF fd {scene}: worst err / tol {worst:.3g} over {n_valid} valid observations")


@pytest.mark.parametrize("scene", SCENES)
def test_premises_and_restatement(scene):
    d, obs = pc.isolated(scene)
    db, edge, obs_b = pc.braced(scene)
    assert d.n_obs <= 40 and db.n_obs <= 45
    for lname, loss in pc.LOSSES.items():
        ld, f64 = refs(d, ("iso", scene, lname), loss)
        pc.premises(d, obs, np.arange(len(obs)), ld)
        assert np.array_equal(ld.valid, f64.valid)
        ratios = {q: pr.entry_ratio(getattr(f64, q), ld, f64, q) for q in pr.QUANTITIES}
        assert all(sr.worst(r)[0] <= 1.0 for r in ratios.values())
        for q in ("r", "Jc", "Jl"):
            assert not np.asarray(getattr(ld, q), dtype=np.float64)[~ld.valid].any()
    # a second crafted point classifies as unambiguously
    p2 = pc.second_point(d)
    ld2 = pr.reference(*p2, d.cam_idx, d.pt_idx, d.obs_uv, loss=pc.LOSSES["huber_delta"])
    z = np.asarray(ld2.pc[:, 2], dtype=np.float64)
    assert (np.abs(z + 1e-6) >= 1e3 * 2.0 ** -53 * np.asarray(ld2.M_z, dtype=np.float64)).all()
    # the braced scene: the edge observations' claims, and the conditioning of what is solved on it
    kap = 1.0
    for lname in BRACED_LOSSES:
        ldb, f64b = refs(db, ("braced", scene, lname), pc.LOSSES[lname])
        pc.premises(db, obs_b, edge, ldb)
        rest = np.setdiff1d(np.arange(db.n_obs), edge)
        assert ldb.valid[rest].all() and (np.abs(np.asarray(ldb.pc[rest, 2], dtype=np.float64) + 1.2) < 0.4).all()
        for mode, (_, dc, mask) in pc.MODES.items():
            a, _ = braced_system(db, ldb, f64b, dc, mask)
            assert a.cond.max() <= 1e8, (mode, a.cond.max())
            kap = max(kap, float(a.kap.max()))
            S = np.asarray(sr.dense_of(a.S4, np.arange(db.n_cam * dc).reshape(db.n_cam, dc), db.n_cam * dc), dtype=np.float64)
            assert np.linalg.cond(S) <= 1e8, (mode, np.linalg.cond(S))
    print(f"PROJREF premises {scene}: largest relative magnitude of H_ll (kap) {kap:.3g}")


@pytest.mark.parametrize("scene", SCENES)
def test_host_build_within_bound(hp, scene):
    d, obs = pc.isolated(scene)
    n = d.n_obs
    worst = {}
    for lname, loss in pc.LOSSES.items():
        ld7, f647 = refs(d, ("iso", scene, lname), loss)
        k = _kind(loss)
        # residual_obs: the corrected residual and the validity
        r = np.zeros((n, 2)); ok_r = np.zeros(n, dtype=bool)
        for i in range(n):
            ok_r[i] = bool(hp.hp_residual(d.poses[i], d.intr[i], d.points[i], d.obs_uv[i], *k, r[i]))
        assert np.array_equal(ok_r, ld7.valid)
        ratios = {"residual_obs": pr.entry_ratio(r, ld7, f647, "r")}
        for dc, mask, masked in WIDTHS:
            ld, f64 = pr.masked(ld7, mask, dc), pr.masked(f647, mask, dc)
            ok, rl, Jc, Jl, rec = host_linearize(hp, d, loss, dc, mask, masked)
            assert np.array_equal(ok, ld.valid), (lname, dc, mask)
            assert not rl[~ok].any() and not Jc[~ok].any() and not Jl[~ok].any() and not rec[~ok][:, [0, 1, 3]].any()
            cm = np.array([mask & 4] * 6 + [mask & 1] * 3)[:dc] != 0
            assert not Jc[:, :, ~cm].any() and (mask & 2 or not Jl.any())
            got = dict(r=pr.entry_ratio(rl, ld, f64, "r"), Jc=pr.entry_ratio(Jc, ld, f64, "Jc"), Jl=pr.entry_ratio(Jl, ld, f64, "Jl"),
                       w=pr.entry_ratio(rec[:, 3], ld, f64, "w"))
            # jv_obs with unit vectors: every entry of [Jc | Jl] once more, and the same validity
            N = dc + 3
            Jv = np.zeros((n, 2, N))
            for i in range(n):
                for c in range(N):
                    a = np.zeros(N); a[c] = 1.0
                    b = np.zeros(N); b[N - 1 - c] = 1.0
                    u, w2 = np.zeros(2), np.zeros(2)
                    assert bool(hp.hp_jv(dc, masked, mask, d.poses[i], d.intr[i], d.points[i], d.obs_uv[i], *k, a, b, u, w2)) == ok[i]
                    Jv[i, :, c] = u
                    assert np.array_equal(w2, np.concatenate([Jc[i], Jl[i]], axis=1)[:, N - 1 - c])
            got["jv_Jc"] = pr.entry_ratio(Jv[:, :, :dc], ld, f64, "Jc"); got["jv_Jl"] = pr.entry_ratio(Jv[:, :, dc:], ld, f64, "Jl")
            for q, v in got.items():
                key = f"{q}"
                ratios[key] = np.maximum(ratios.get(key, 0.0), v) if q in ("r", "Jl", "w", "jv_Jl") else max(float(np.max(v)), float(np.max(ratios.get(key, 0.0))))
        for q, v in ratios.items():
            if float(np.max(v)) >= worst.get(q, (-1.0, ""))[0]:
                worst[q] = float(np.max(v)), lname
            assert float(np.max(v)) <= 1.0, (scene, lname, q, sr.worst(np.asarray(v)))
    print(f"PROJREF host {scene}: " + "  ".join(f"{q} {v:.3g}@{l}" for q, (v, l) in worst.items()))


@pytest.mark.parametrize("scene", SCENES)
def test_host_build_on_the_braced_scene(hp, scene):
    """The host build's blocks through the fp64 Schur arithmetic stay within the block rule against the reference's: the check the
    GPU test makes of the device's assembly, with the conditioning of this scene."""
    d, edge, obs = pc.braced(scene)
    for lname in BRACED_LOSSES:
        loss = pc.LOSSES[lname]
        ld7, f647 = refs(d, ("braced", scene, lname), loss)
        for mode, (_, dc, mask) in pc.MODES.items():
            ld, f64 = braced_system(d, ld7, f647, dc, mask)
            ok, r, Jc, Jl, _ = host_linearize(hp, d, loss, dc, mask, 1)
            dev = sr.SchurRef(d.n_cam, d.n_pt, d.cam_idx, d.pt_idx, Jc, Jl, r, pc.LAMBDA, np.float64)
            ratios = {}
            ratios["S"], bad = sr.block_check(dev.S4, ld, f64)
            ratios["gred"] = sr.vec_check(dev.gred, ld.gred, f64.gred, ld.gred_mag, ld.gred_terms)
            ratios["hinv"] = sr.vec_check(dev.Hinv, ld.Hinv, f64.Hinv, ld.hinv_mag, ld.k_l)
            ratios["gl"] = sr.vec_check(dev.gl, ld.gl, f64.gl, ld.gl_mag, ld.k_l)
            pr.report(f"host braced {scene} {lname} {mode}", ratios)
            assert not bad, [(b, float(ratios["S"][b])) for b in bad[:6]]
            for q in ("gred", "hinv", "gl"):
                assert sr.worst(ratios[q])[0] <= 1.0, (mode, q, sr.worst(ratios[q]))
