"""The landmark covariance reference (tests/landmark_cov_ref.py) proved on the CPU before it judges the kernel: against the
landmark blocks of a long double inverse of the FULL damped matrix, against seven injected faults of a kernel-shaped fp64
restatement, and the premises of the crafted structures (tests/landmark_cov_cases.py) from the host lists.  No GPU."""
import functools

import numpy as np
import pytest

import landmark_cov_cases as lc
import landmark_cov_ref as lr
import np_ref
import np_ref_ba_loss as nb
import schur_ref as sr
import tile_ref as tr
from apex_solver_amd import capi
from apex_solver_amd.loss import create_loss_function

LOSSES = ("none", "huber", "cauchy")


def np_blocks(d, dc, loss="huber"):
    """The corrected blocks of the numpy restatement at the problem's initial parameters, in the handle's export format."""
    if loss == "cauchy":
        r, jp, jl, ji, _, _ = nb.linearize(d.poses, d.intr, d.points, d.cam_idx.astype(int), d.pt_idx.astype(int), d.obs_uv,
                                              create_loss_function("cauchy", 2.0))
    else:
        r, _, jp, jl, ji = np_ref.jacobian_blocks(d.poses, d.intr, d.points, d.cam_idx, d.pt_idx, d.obs_uv, 1.0 if loss == "huber" else 0)
    return (np.concatenate([jp, ji], axis=2) if dc == 9 else jp), jl, r.ravel()


def jacobi_scales(d, jc, jl):
    """1 / (1 + column norm) per camera and landmark column: the scaling the device test applies"""
    nc2 = np.zeros((d.n_cam, jc.shape[2])); np.add.at(nc2, d.cam_idx.astype(int), (jc ** 2).sum(1))
    nl2 = np.zeros((d.n_pt, 3)); np.add.at(nl2, d.pt_idx.astype(int), (jl ** 2).sum(1))
    return 1.0 / (1.0 + np.sqrt(nc2)), 1.0 / (1.0 + np.sqrt(nl2))


@functools.lru_cache(maxsize=None)
def reference(name, mode, loss="huber", scaled=False):
    d = lc.problem(name)
    dc = 9 if mode == "selfcal" else 6
    jc, jl, r = np_blocks(d, dc, loss)
    s_c, s_l = jacobi_scales(d, jc, jl) if scaled else (None, None)
    ld, f64 = lr.pair(d.n_cam, d.n_pt, d.cam_idx, d.pt_idx, jc, jl, r, lc.lam_of(name, mode, scaled), s_c, s_l)
    return d, ld, f64, s_l


def library_order(d, dc):
    """per landmark: the caller's observation indices in the library's landmark-major order"""
    o_index = capi.pair_lists(d.n_cam, d.n_pt, dc, d.cam_idx, d.pt_idx)["o_index"]
    k = np.bincount(d.pt_idx.astype(int), minlength=d.n_pt)
    ptr = np.concatenate([[0], np.cumsum(k)])
    out = [o_index[ptr[l]:ptr[l + 1]].astype(np.int64) for l in range(d.n_pt)]
    assert all((d.pt_idx[o] == l).all() for l, o in enumerate(out))
    return out


# ---- the Schur formula against the inverse of the full matrix -----------------------------------------------------------------
@pytest.mark.parametrize("name,mode,scaled", [("groups_17", "selfcal", False), ("dup", "selfcal", False), ("dup", "ba", True),
                                              ("tiles_17", "selfcal", True), ("tiles_25", "ba", False)])
def test_schur_formula_against_the_full_inverse(name, mode, scaled):
    d, ld, f64, _ = reference(name, mode, "huber", scaled)
    dc, nc = ld.dc, d.n_cam * ld.dc
    n = nc + 3 * d.n_pt
    assert n <= 600
    # the full matrix from the Jacobian blocks themselves, J^T J + lambda I with J dense: nothing of SchurRef in it
    jc, jl, _ = np_blocks(d, dc, "huber")
    s_c, s_l = jacobi_scales(d, jc, jl) if scaled else (None, None)
    jc, jl = lr.scaled_blocks(jc, jl, d.cam_idx, d.pt_idx, s_c, s_l, lr.LD)
    J = np.zeros((2 * d.n_obs, n), dtype=lr.LD)
    for k in range(d.n_obs):
        c, l = int(d.cam_idx[k]), int(d.pt_idx[k])
        J[2 * k:2 * k + 2, c * dc:(c + 1) * dc] = jc[k]
        J[2 * k:2 * k + 2, nc + 3 * l:nc + 3 * l + 3] = jl[k]
    M = J.T @ J + lr.LD(lc.lam_of(name, mode, scaled)) * np.eye(n, dtype=lr.LD)
    Li = tr.tri_inv_ld(tr.chol_ld(M))
    Minv = Li.T @ Li
    kappa = float(np.linalg.cond(np.asarray(M, dtype=np.float64)))
    eps = float(np.finfo(lr.LD).eps)
    worst = 0.0
    for l in range(d.n_pt):
        blk = Minv[nc + 3 * l:nc + 3 * l + 3, nc + 3 * l:nc + 3 * l + 3]
        worst = max(worst, float(np.abs(blk - ld.Sigma[l]).max() / np.abs(blk).max()))
    print(f"full inverse {name} {mode} scaled {scaled}: worst {worst:.2e}, kappa(M) {kappa:.2e}, eps kappa {eps * kappa:.2e}")
    # (two long double inversions by Cholesky, each within c n eps kappa of the inverse -- Higham, Accuracy and Stability,
    # section 14.3; n is the dimension, at most 600: 1e-16 kappa at the outside, still three digits below fp64)
    assert worst <= n * eps * kappa
    # and the camera blocks of the same inverse are the diagonal blocks of Z
    Zd, _ = ld.cam_blocks()
    for c in range(d.n_cam):
        blk = Minv[c * dc:(c + 1) * dc, c * dc:(c + 1) * dc]
        assert float(np.abs(blk - Zd[c]).max() / np.abs(blk).max()) <= n * eps * kappa


# ---- a kernel-shaped fp64 restatement and its faults --------------------------------------------------------------------------
def kernel_shaped(f64, obs, l, fault=None, dl=None):
    """Landmark l as the kernel forms it, in fp64 from the restatement's U and Z: chunks of 32, unordered pairs with the half
    weight, the orientation by camera order, X + X^T.  fault: one of FAULTS."""
    dc, cpt = f64.dc, lr.NB // f64.dc
    o = obs[l]
    if fault == "second observation of a duplicate camera dropped":
        _, first = np.unique(f64.ci[o], return_index=True)
        o = o[np.sort(first)]
    k = len(o)
    large = k > lr.SMALL_K
    if fault == "ragged last chunk truncated" and large and k > lr.CHUNK:
        k = (k // lr.CHUNK) * lr.CHUNK
    ch = lr.CHUNK if large else lr.SMALL_K
    nch = (k + ch - 1) // ch
    U, cam = f64.TW[o], f64.ci[o]

    def z(ci, cj):
        if fault == "Z block one camera off at a tile boundary" and ci % cpt == 0 and ci > 0:
            ci = ci - 1
        return f64.Z4[ci, cj]

    X = np.zeros((3, 3))
    for ca in range(nch):
        for cb in range(ca, nch):
            if fault == "chunk pair (0, 2) dropped" and (ca, cb) == (0, 2):
                continue
            for i in range(ca * ch, min(k, (ca + 1) * ch)):
                for j in range(cb * ch, min(k, (cb + 1) * ch)):
                    if ca == cb and i > j:
                        continue
                    w = 0.5 if i == j and fault != "weight 1 on i == j" else 1.0
                    if cam[i] >= cam[j]:
                        X += w * U[i].T @ z(cam[i], cam[j]) @ U[j]
                    elif fault == "swapped pair not transposed":
                        X += w * U[i].T @ z(cam[j], cam[i]) @ U[j]
                    else:
                        X += w * U[j].T @ z(cam[j], cam[i]) @ U[i]
    out = f64.Hinv[l] + (X + X.T)
    if fault == "pt_scale applied once":       # the record form divided by d_p only: Sigma_pq d_q
        out = out * dl[l][None, :]
    return out


FAULTS = {"weight 1 on i == j": ("k_ladder", False), "swapped pair not transposed": ("k_ladder", False),
          "chunk pair (0, 2) dropped": ("k_ladder", False), "ragged last chunk truncated": ("k_ladder", False),
          "second observation of a duplicate camera dropped": ("dup", False),
          "Z block one camera off at a tile boundary": ("k_ladder", False), "pt_scale applied once": ("dup", True)}


def _shaped_ratios(name, scaled, fault):
    d, ld, f64, s_l = reference(name, "selfcal", "huber", scaled)
    obs = library_order(d, 9)
    dev = np.stack([kernel_shaped(f64, obs, l, fault, s_l) for l in range(d.n_pt)])
    return d, ld, lr.landmark_check(dev, ld, f64)


@pytest.mark.parametrize("name,scaled", [("k_ladder", False), ("dup", False), ("dup", True)])
def test_unmutated_restatements_pass_everywhere(name, scaled):
    d, ld, ratio = _shaped_ratios(name, scaled, None)
    lr.report(f"kernel-shaped fp64 {name} scaled {scaled}", ratio, ld)
    assert ratio.max() <= 1.0
    _, ld, f64, _ = reference(name, "selfcal", "huber", scaled)
    assert lr.landmark_check(f64.Sigma, ld, f64).max() <= 1.0 and lr.camera_check(f64.cam_blocks()[0], ld, f64).max() <= 1.0


@pytest.mark.parametrize("fault", list(FAULTS))
def test_rule_sees_the_fault(fault):
    name, scaled = FAULTS[fault]
    d, ld, ratio = _shaped_ratios(name, scaled, fault)
    bad = np.nonzero(ratio > 1.0)[0]
    print(f"{fault}: {len(bad)} landmarks fail, worst ratio {ratio.max():.3g} at k {int(ld.k_l[int(np.argmax(ratio))])}")
    assert len(bad) >= 1
    k = ld.k_l[bad]
    if fault == "chunk pair (0, 2) dropped":
        assert (k > 2 * lr.CHUNK).all() and set(k) == {65, 96, 97}
    if fault == "ragged last chunk truncated":
        assert set(k) == {33, 63, 65, 97}


# ---- premises -----------------------------------------------------------------------------------------------------------------
def _k(d):
    return np.bincount(d.pt_idx.astype(int), minlength=d.n_pt)


@pytest.mark.parametrize("name", lc.CASES)
def test_camera_order_and_conditioning(name):
    """The caller's camera order is the internal one; kappa(S) <= 1e6 and every landmark in the plain-inverse regime of the
    gate, for every mode, loss and scaling a device run may take."""
    n_cam, lists, modes = lc.structure(name)
    d = lc.problem(name)
    for mode in modes:
        dc = 9 if mode == "selfcal" else 6
        hs = capi.host_structure(n_cam, d.n_pt, d.cam_idx, d.pt_idx, mode=1 if mode == "selfcal" else 0, schur_form=4)
        assert np.array_equal(hs["cmap"], np.arange(n_cam)), name
        for loss in (("none",) if name == "gate" else LOSSES):
            jc, jl, r = np_blocks(d, dc, loss)
            for scaled in ((False,) if name == "gate" else (False, True)):
                s_c, s_l = jacobi_scales(d, jc, jl) if scaled else (None, None)
                a, b = lr.scaled_blocks(jc, jl, d.cam_idx, d.pt_idx, s_c, s_l, np.float64)
                ref = sr.SchurRef(n_cam, d.n_pt, d.cam_idx, d.pt_idx, a, b, r, lc.lam_of(name, mode, scaled), np.float64)
                if name == "gate":       # (kappa(S) with the gated block: test_premises_of_the_gate)
                    assert ref.cond[-1] > 1e10 and ref.cond[:-1].max() <= 1e8, (mode, ref.cond[-1])
                    continue
                assert ref.cond.max() <= 1e8, (name, mode, loss, scaled, ref.cond.max())
                S = ref.S4.transpose(0, 2, 1, 3).reshape(n_cam * dc, n_cam * dc)
                assert np.linalg.cond(S) <= 1e6, (name, mode, loss, scaled, np.linalg.cond(S))


def test_premises_of_the_k_ladder():
    d = lc.problem("k_ladder")
    k = _k(d)
    assert tuple(k[:len(lc.LADDER_K)]) == lc.LADDER_K and (k[len(lc.LADDER_K):] == 3).all()
    obs = library_order(d, 9)
    # The caller's factor order is shuffled, but the library orders a landmark's observations by INTERNAL camera
    # (ba_structure.hip): for i < j the kernel always sees c(i) < c(j) and takes the pair as (j, i); c(i) >= c(j) is reached
    # with i == j and with a camera observing the landmark twice only (the `dup` case).
    for l in range(len(lc.LADDER_K)):
        c = d.cam_idx[obs[l]].astype(int)
        assert (np.diff(c) > 0).all()
        assert not (np.diff(d.cam_idx[np.nonzero(d.pt_idx == l)[0]].astype(int)) > 0).all() or len(c) < 3


@pytest.mark.parametrize("name,small,large,last", [("groups_15", 15, 0, 15), ("groups_16", 16, 0, 0), ("groups_17", 17, 0, 1),
                                                   ("only_large", 0, 7, 0), ("large_first", 17, 1, 1)])
def test_premises_of_the_group_counts(name, small, large, last):
    k = _k(lc.problem(name))
    assert int((k <= lr.SMALL_K).sum()) == small and int((k > lr.SMALL_K).sum()) == large and (k >= 1).all()
    assert small % lr.GROUPS == last
    if name == "large_first":
        assert k[0] > lr.CHUNK and (k[1:] <= lr.SMALL_K).all()
    if name == "only_large":
        assert sorted(k) == [9, 9, 12, 20, 33, 34, 40]


def test_premises_of_the_duplicates():
    d = lc.problem("dup")
    k = _k(d)
    assert k[0] == 3 and k[1] == 4 and k[2] >= 34
    for dc in (9, 6):
        obs = library_order(d, dc)
        assert sorted(d.cam_idx[obs[0]]) == [5, 5, 9] and sorted(d.cam_idx[obs[1]]) == [4, 4, 4, 8]
        c = d.cam_idx[obs[2]].astype(int)
        at = np.nonzero(c == d.n_cam - 1)[0]
        assert list(at) == [30, 31, 32, 33] and lr.CHUNK == 32      # the same camera twice in the first chunk and twice in the second
        assert list(np.nonzero(c == 5)[0]) == [5, 6]                  # and one twice inside a chunk


@pytest.mark.parametrize("mode,n", [(m, n) for m in lc.BOTH for n in lc.TILE_CASES[m]])
def test_premises_of_the_tile_boundaries(mode, n):
    cpt = lr.NB // (9 if mode == "selfcal" else 6)
    n_cam, lists, modes = lc.structure(f"tiles_{n}")
    have = {tuple(c) for c in lists}
    for b in range(cpt, n, cpt):                     # (the internal order is the caller's: test_camera_order_and_conditioning)
        assert (b - 1, b) in have and any(c[0] == b - 2 and b in c for c in lists)
    assert (0, n - 1) in have
    assert any(len({c // cpt for c in cams}) == 1 and len(cams) == 3 for cams in lists)
    assert ((n + cpt - 1) // cpt > 1) == (n > cpt)


def test_premises_of_the_fill():
    n_cam, lists, _ = lc.structure("fill")
    d = lc.problem("fill")
    hs = capi.host_structure(n_cam, d.n_pt, d.cam_idx, d.pt_idx, mode=1, schur_form=4)
    assert hs["tiles"] > hs["touched_tiles"] and hs["etree_levels"] >= 3 and n_cam > 16 * 3
    cols = {min(a, b) // 16 for cams in lists for a in cams for b in cams if a // 16 != b // 16}
    assert len(cols) > 1                              # covisible pairs off the diagonal in more than one tile column


def test_premises_of_the_observations_behind():
    d = lc.problem("behind")
    for dc in (9, 6):
        jc, jl, r = np_blocks(d, dc, "none")
        zero = ~jl.reshape(d.n_obs, -1).any(axis=1)
        assert np.array_equal(zero, d.cam_idx == lc.BEHIND_CAM) and not jc[zero].any()
        for l in lc.BEHIND_LANDMARKS:
            assert int((zero & (d.pt_idx == l)).sum()) == 1
    k = _k(d)
    assert k[0] <= lr.SMALL_K < lr.CHUNK < k[1]


@pytest.mark.parametrize("mode", lc.BOTH)
def test_premises_of_the_gate(oracle, mode):
    """The gate fires on the close landmark (the oracle's restatement of the gate stands in for the device's); with that
    inverse taken as given the reference's S is positive definite with 1e6 < kappa(S) <= GATE_KAPPA; no block of S adds
    atomically, so the device's export has the factorised bits.  With an fp64-assembled S given as the matrix (what the device
    test does with the device's S) the fp64 restatement passes the rule on every landmark, and a faulty kernel does not: the
    gated landmark and the landmarks of its camera all fail under `weight 1 on i == j`, every landmark under `pt_scale`-free
    faults of the pair sum."""
    d = lc.problem("gate")
    g = lc.gated_landmark("gate", d)
    dc = 9 if mode == "selfcal" else 6
    jc, jl, r = np_blocks(d, dc, "none")
    lam = lc.lam_of("gate", mode)
    o = np.nonzero(d.pt_idx == g)[0]
    B = np.einsum("kra,krb->ab", jl[o], jl[o]) + lam * np.eye(3)
    hinv = np.empty((1, 9))
    assert oracle.lib().ora_invert_landmark_blocks(1, np.ascontiguousarray(B.reshape(1, 9)), 0.0, hinv) == 0
    hinv, plain = hinv.reshape(3, 3), np.linalg.inv(B)
    assert np.abs(hinv - plain).max() > 1e-3 * np.abs(plain).max()
    pl = capi.pair_lists_queued(d.n_cam, d.n_pt, d.cam_idx, d.pt_idx, dc)
    assert not (pl["blocks"][:, 3] & 1).any()
    own = lr.LandmarkCovRef(d.n_cam, d.n_pt, d.cam_idx, d.pt_idx, jc, jl, r, lam, np.float64, hinv_dev={g: hinv})
    assert 1e6 < own.kappa <= lc.GATE_KAPPA and own.gated == [g]
    S64 = 0.5 * (own.S + own.S.T)                       # an fp64 assembly: the stand-in for the device's S
    ld, f64 = lr.pair(d.n_cam, d.n_pt, d.cam_idx, d.pt_idx, jc, jl, r, lam, hinv_dev={g: hinv}, S_given=S64)
    print(f"gate {mode}: kappa(S) {ld.kappa:.3g}")
    assert abs(ld.kappa - own.kappa) <= 1e-4 * own.kappa       # (of the reference's own S, not of the given one)
    assert lr.landmark_check(f64.Sigma, ld, f64).max() <= 1.0 and lr.camera_check(f64.cam_blocks()[0], ld, f64).max() <= 1.0
    obs = library_order(d, dc)
    cam_g = int(d.cam_idx[o[0]])
    near = np.unique(d.pt_idx[d.cam_idx == cam_g]).astype(int)
    assert g in near and len(near) > 3
    ok = lr.landmark_check(np.stack([kernel_shaped(f64, obs, l) for l in range(d.n_pt)]), ld, f64)
    assert ok.max() <= 1.0
    for fault in ("weight 1 on i == j", "swapped pair not transposed"):
        ratio = lr.landmark_check(np.stack([kernel_shaped(f64, obs, l, fault) for l in range(d.n_pt)]), ld, f64)
        print(f"gate {mode} {fault}: {int((ratio > 1).sum())} of {d.n_pt} fail, gated landmark {ratio[g]:.3g}, its camera's least {ratio[near].min():.3g}")
        if fault.startswith("weight"):
            assert (ratio[near] > 1.0).all() and (ratio > 1.0).all()
        else:
            assert (ratio[_k(d) > 1] > 1.0).all()
    frac = lr.landmark_floor(ld).max(axis=(1, 2)) / np.abs(np.asarray(ld.Sigma - ld.Hinv, dtype=np.float64)).max(axis=(1, 2))
    print(f"gate {mode}: floor / correction at most {frac.max():.2e}, gated landmark {frac[g]:.2e}")
    # (the gated landmark's own terms cancel -- its U holds the 2e5 of a camera 4e-3 away -- so its floor is about 1e-2 of its
    # correction term; the faults above change that term by tens of per cent and fail on it)
    assert np.delete(frac, g).max() <= 1e-3 and frac[g] <= 5e-2
    zero = lr.landmark_check(np.zeros((d.n_pt, 3, 3)), ld, f64)
    assert (zero > 1.0).all() and (lr.camera_check(np.zeros((d.n_cam, dc, dc)), ld, f64) > 1.0).all()


@pytest.mark.parametrize("name", [c for c in lc.CASES if c != "gate"])       # (gate: in test_premises_of_the_gate, with the gated inverse)
def test_floor_is_a_small_fraction_of_the_correction_term(name):
    """floor_l against Sigma_l - Hinv_l, the term the kernel computes, largest entry against largest entry: at most 1e-3 on
    every landmark with a correction term (a camera none of whose observations is in front contributes none)."""
    n_cam, lists, modes = lc.structure(name)
    d = lc.problem(name)
    for mode in modes:
        dc = 9 if mode == "selfcal" else 6
        for scaled in (False, True):
            jc, jl, r = np_blocks(d, dc, "huber")
            s_c, s_l = jacobi_scales(d, jc, jl) if scaled else (None, None)
            f64 = lr.LandmarkCovRef(n_cam, d.n_pt, d.cam_idx, d.pt_idx, jc, jl, r, lc.lam_of(name, mode, scaled), np.float64, s_c, s_l)
            corr = np.abs(f64.Sigma - f64.Hinv).max(axis=(1, 2))
            floor = lr.landmark_floor(f64).max(axis=(1, 2))
            has = corr > 0
            frac = floor[has] / corr[has]
            print(f"{name} {mode} scaled {scaled}: floor / correction at most {frac.max():.2e}")
            assert has.sum() >= d.n_pt - 1 and frac.max() <= 1e-3
