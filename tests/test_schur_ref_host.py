"""The Schur reference (tests/schur_ref.py) against the oracle, the sensitivity of its block check, and the premises of the
crafted structures (tests/schur_cases.py) read from the host pair lists.  No GPU: a structure that loses its edge after a
change to the list builder fails here, not quietly on the device."""
import math

import numpy as np
import pytest

import apex_solver_amd as pkg
import np_ref
import schur_cases as sc
import schur_ref as sr
from apex_solver_amd import capi
from apex_solver_amd.layout import reference_column_layout
from ba_custom import custom_problem

NB = 144
ATOMIC, DIAG, FLUSH, CARRY, JOIN = 1, 2, 4, 8, 16


def rel(a, b):
    a = np.ravel(np.asarray(a, dtype=np.float64)); b = np.ravel(np.asarray(b, dtype=np.float64))
    return float(np.linalg.norm(a - b) / max(np.linalg.norm(b), 1e-300))


def np_blocks(d, dc):
    """The corrected blocks of the numpy restatement at the problem's initial parameters, in the handle's export format."""
    rt, _, jp, jl, ji = np_ref.jacobian_blocks(d.poses, d.intr, d.points, d.cam_idx, d.pt_idx, d.obs_uv, 1.0)
    jc = np.concatenate([jp, ji], axis=2) if dc == 9 else jp
    return jc, jl, rt.ravel()


# ---- reference against oracle ------------------------------------------------------------------------------------------------
def _generator():
    return pkg.synthetic.make_problem(12, 300, 3, 6, config_id=7)


def _ragged():
    rng = np.random.default_rng(9)
    lists = [[], [5, 5, 9], list(range(30)), [7, 8, 7, 8, 20], [39, 0, 39]] + [[3, 7]] * 80
    lists += [sorted(rng.choice(40, size=int(rng.integers(2, 8)), replace=False).tolist()) for _ in range(150)]
    return custom_problem(40, lists, seed=11, outlier_every=5)


@pytest.mark.parametrize("mode", ["selfcal", "ba"])
@pytest.mark.parametrize("make", [_generator, _ragged], ids=["generator", "ragged"])
def test_reference_against_oracle(oracle, make, mode):
    d = make()
    lay = reference_column_layout(d.n_cam, d.n_pt)
    dc = 9 if mode == "selfcal" else 6
    lam = 1e-3
    o = oracle.from_data(d, lay, mode=mode)
    _, r, oJp, oJl, oJi = o.linearize()
    ostep, ograd, oS, ogred = o.solve_augmented(lam, 0, want_schur=True)
    jc = np.concatenate([oJp, oJi], axis=2) if dc == 9 else oJp
    ld, f64 = sr.pair(d.n_cam, d.n_pt, d.cam_idx, d.pt_idx, jc, oJl, r, lam)
    assert ld.cond.max() <= 1e8
    cols = sr.cam_cols(lay, d.n_cam, dc)
    n = lay.cam_dof
    S = sr.dense_of(f64.S4, cols, n, fill_diag=lam)
    gred = np.zeros(n); gred[cols] = f64.gred
    # (the oracle drops entries of S below 1e-12 as the reference's CSC conversion does; two fp64 evaluations of H_ll^-1 differ
    # by u cond(H_ll), and so do the products built on them)
    assert np.abs(S - oS).max() <= 1e-12 + 8 * sr.U * ld.cond.max() * np.abs(oS).max() and rel(S, oS) < 1e-12
    assert rel(gred, ogred) < 1e-12
    # the oracle's S, an independent fp64 evaluation, passes the block rule of the long double reference
    ratio, bad = sr.block_check(sr.blocks_of(oS, cols), ld, f64)
    keep = [b for b in bad if np.abs(ld.S4[b]).max() > 1e-9]      # (blocks with entries the oracle dropped)
    sr.report(f"oracle {make.__name__[1:]} {mode}", dict(S=ratio))
    assert not keep, keep
    hinv = np.empty((d.n_pt, 9))
    assert oracle.lib().ora_invert_landmark_blocks(d.n_pt, np.ascontiguousarray(f64.Hll.reshape(-1, 9)), 0.0, hinv) == 0
    assert rel(f64.Hinv, hinv) < 1e-15 * ld.cond.max() + 1e-14
    # the step: the oracle's camera step solves the reference's system, and goes through the reference's back-substitution
    dcam = ostep[cols]
    y, _ = f64.matvec(dcam)
    assert rel(y, f64.gred) < 1e-9 and rel(S @ ostep[:n], ogred) < 1e-9
    dl, _ = f64.back_substitute(dcam)
    assert rel(dl, ostep[lay.pt_col[:, None] + np.arange(3)[None]]) < 1e-10
    # long double and fp64 restatements agree to fp64 rounding of the terms
    assert np.all(np.abs(np.asarray(f64.S4, dtype=sr.LD) - ld.S4).max(axis=(2, 3)) <= 64 * sr.U * ld.cond.max() * np.maximum(ld.M, 1e-300))


# ---- sensitivity of the block check ----------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def mutable():
    """A structure with a 2,600-pair block (7, 3) beside a one-pair block (1, 0), a 600-pair block (11, 10), a diagonal block
    (5, 5) and a block (15, 14) next to the tile boundary at camera 16 whose neighbour (16, 14) has no landmark."""
    lists = [[3, 7]] * 2600 + [[0, 1]] + [[10, 11]] * 600 + [[5, 5, 9]] * 5 + [[14, 15]] * 4 + [[15, 16], [16, 17, 18], [2, 19], [12, 13, 8]]
    d = custom_problem(20, lists, seed=31, outlier_every=5)
    jc, jl, r = np_blocks(d, 9)
    ld, f64 = sr.pair(20, d.n_pt, d.cam_idx, d.pt_idx, jc, jl, r, 1e-3)
    assert ld.cond.max() <= 1e8
    assert ld.P[7, 3] == 2600 and ld.P[1, 0] == 1 and ld.P[11, 10] == 600 and ld.P[16, 14] == 0
    ratio, bad = sr.block_check(f64.S4, ld, f64)
    assert not bad and ratio.max() <= 1.0
    return d, ld, f64


def _term(ld, a, b):
    return np.asarray(ld.TW[a] @ ld.W[b].T, dtype=np.float64)


def _obs(d, cam, partner):
    """One observation of `cam` whose landmark is also seen by `partner`, and that partner observation."""
    for a in np.nonzero(d.cam_idx == cam)[0]:
        for b in np.nonzero((d.pt_idx == d.pt_idx[a]) & (d.cam_idx == partner))[0]:
            if a != b:
                return int(a), int(b)
    raise AssertionError


def _bad(S4, ld, f64):
    return set(sr.block_check(S4, ld, f64)[1])


def test_check_sees_a_dropped_pair(mutable):
    d, ld, f64 = mutable
    a, b = _obs(d, 11, 10)
    S = f64.S4.copy(); S[11, 10] += _term(ld, a, b); S[10, 11] += _term(ld, a, b).T
    assert _bad(S, ld, f64) == {(11, 10), (10, 11)}


def test_check_sees_a_pair_added_twice(mutable):
    d, ld, f64 = mutable
    a, b = _obs(d, 11, 10)
    S = f64.S4.copy(); S[11, 10] -= _term(ld, a, b); S[10, 11] -= _term(ld, a, b).T
    assert _bad(S, ld, f64) == {(11, 10), (10, 11)}


def test_check_sees_a_diagonal_block_flushed_without_its_transpose(mutable):
    d, ld, f64 = mutable
    B = np.zeros((9, 9))
    for l in np.unique(d.pt_idx[d.cam_idx == 5]):
        ks = np.nonzero((d.pt_idx == l) & (d.cam_idx == 5))[0]
        if len(ks) == 2:
            B += _term(ld, ks[1], ks[0])
    S = f64.S4.copy(); S[5, 5] += B.T                      # S holds -(B + B^T): take B^T out again
    assert _bad(S, ld, f64) == {(5, 5)}


def test_check_sees_a_transposed_block(mutable):
    d, ld, f64 = mutable
    S = f64.S4.copy(); S[7, 3] = S[7, 3].T.copy()
    assert _bad(S, ld, f64) == {(7, 3)}


def test_check_sees_a_block_one_camera_across_a_tile_boundary(mutable):
    d, ld, f64 = mutable
    S = f64.S4.copy(); S[16, 14] = S[15, 14]; S[15, 14] = 0.0
    assert _bad(S, ld, f64) == {(15, 14), (16, 14)}


def test_check_sees_a_small_block_beside_a_large_one(mutable):
    """1e4 ulp of the one-pair block's own magnitude: invisible to a global norm beside the 2,600-pair block."""
    d, ld, f64 = mutable
    S = f64.S4.copy(); S[1, 0, 2, 4] += 1e4 * sr.U * ld.M[1, 0]
    assert _bad(S, ld, f64) == {(1, 0)}
    assert rel(S, f64.S4) < 1e-13 and ld.M[7, 3] > 100 * ld.M[1, 0]


# ---- premises of every crafted structure ------------------------------------------------------------------------------------
def _indices(name):
    n_cam, lists, lam, modes = sc.structure(name)
    cam_idx = np.asarray([c for cams in lists for c in cams], dtype=np.uint32)
    pt_idx = np.asarray([l for l, cams in enumerate(lists) for _ in cams], dtype=np.uint32)
    return n_cam, len(lists), cam_idx, pt_idx


def _pieces(pl):
    """{(ci, cj): [flags of every piece]} of either layout's block table."""
    out = {}
    for dst, ci, cj, fl in pl["blocks"]:
        out.setdefault((int(ci), int(cj)), []).append(int(fl) & 3)
    return out


def _lists(name, dc):
    n_cam, n_pt, ci, pi = _indices(name)
    q = capi.pair_lists_queued(n_cam, n_pt, ci, pi, 9) if dc == 9 else None
    return q, capi.pair_lists(n_cam, n_pt, dc, ci, pi)


def _tasks_of_row(q, ci):
    return [(int(c0), int(n)) for c0, n in q["tasks"] if int(q["qdesc"][c0, 7, 1]) == ci]


def _max_blocks_in_a_chunk(pl3):
    return max(1 + bin(int(np.uint32(m)) & ~1).count("1") for m in pl3["chunks"][:, 0])


@pytest.mark.parametrize("name", [c for c in sc.DENSE_CASES])
def test_small_structures_keep_the_callers_camera_order_and_the_plain_inverse(name):
    """The host lists below are built in the caller's camera order; the device's are too as long as neither the hub reordering
    nor nested dissection sets in (fewer than 23 tile rows).  And every landmark is in the plain-inverse regime of the gate."""
    n_cam, n_pt, ci, pi = _indices(name)
    lam, modes = sc.structure(name)[2:]
    d = sc.problem(name)
    for mode in modes:
        hs = capi.host_structure(n_cam, n_pt, ci, pi, mode=1 if mode == "selfcal" else 0, schur_form=4)
        assert np.array_equal(hs["cmap"], np.arange(n_cam)), name
        dc = 9 if mode == "selfcal" else 6
        jc, jl, r = np_blocks(d, dc)
        ref = sr.SchurRef(n_cam, d.n_pt, d.cam_idx, d.pt_idx, jc, jl, r, lam, np.float64, dense=False)
        assert ref.cond.max() <= 1e8, (name, ref.cond.max())
        assert (np.linalg.norm(np_ref.residuals(d.poses, d.intr, d.points, d.cam_idx, d.pt_idx, d.obs_uv, -1.0)[0], axis=1) > 1.0).sum() > 0


@pytest.mark.parametrize("name,lengths", [("ladder_a", sc.LADDER_A), ("ladder_b", sc.LADDER_B)])
def test_premises_of_the_length_ladders(name, lengths):
    q, p3 = _lists(name, 9)
    _, p6 = _lists(name, 6)
    pq, n_tasks64 = _pieces(q), 0
    for k, P in enumerate(lengths):
        key = (2 * k + 1, 2 * k)
        assert pq[key] == [ATOMIC if P > 576 else 0] * math.ceil(P / 576), (key, pq[key])
        for p in (_pieces(p3), _pieces(p6)):
            assert p[key] == ([ATOMIC] * math.ceil(P / 4096) if P > 4096 else [0]), (key, p[key])
    assert max(int(n) for _, n in q["tasks"]) == 64                      # a piece of 576 pairs: a task of 64 chunks
    assert any(len(v) > 1 for v in (_pieces(q)[k] for k in _pieces(q))) == (max(lengths) > 576)
    assert len(_pieces(q)) > len(lengths)                                # rows with several blocks
    if name == "ladder_b":
        assert len(_tasks_of_row(q, 9)) > 1                              # 4096 pairs = 456 nonets: more than one task in a row
        for p in (p3, p6):
            assert max(int(n) for _, n in p["tasks"]) == 64              # the 4096-slot block alone in a task of 64 chunks


def test_premises_of_the_cuts_inside_a_row():
    q, p3 = _lists("cuts", 9)
    tasks = _tasks_of_row(q, 12)
    assert len(tasks) == 1 and tasks[0][1] == 12
    c0, n = tasks[0]
    fl = q["qdesc"][c0:c0 + n, :7, 2]
    assert int(((fl & CARRY) != 0).sum()) >= 1 and int(((fl & JOIN) != 0).sum()) >= 1
    assert int(((fl & CARRY) != 0).sum()) == int(((fl & JOIN) != 0).sum())
    for j, P in enumerate(sc.CUT_LENGTHS):
        assert _pieces(q)[(12, j)] == [0] and _pieces(p3)[(12, j)] == [0]     # cut or not: stored once, no atomics


@pytest.mark.parametrize("count", sc.DIAG_COUNTS)
def test_premises_of_the_diagonal_blocks(count):
    q, p3 = _lists(f"diag_{count}", 9)
    _, p6 = _lists(f"diag_{count}", 6)
    assert _pieces(q)[(5, 5)] == [ATOMIC | DIAG] * math.ceil(count / 576)
    assert _pieces(q)[(4, 4)] == [ATOMIC | DIAG]
    for p in (p3, p6):
        assert _pieces(p)[(5, 5)] == [ATOMIC | DIAG] and _pieces(p)[(4, 4)] == [ATOMIC | DIAG]
        assert _pieces(p)[(9, 5)] == [0]
    n_cam, n_pt, ci, pi = _indices(f"diag_{count}")
    real = q["recs"][:, 0] != 0xFFFFFFFF
    assert int(real.sum()) == 3 * count + 6 + 1 + 3 + 3 + 1 + 3        # [5,5,9]: 3 pairs; [4,4,4,8]: 6; the ordinary ones


def test_premises_of_the_duplicated_camera_in_a_long_block():
    q, p3 = _lists("diag_long", 9)
    assert _pieces(q)[(3, 3)] == [ATOMIC | DIAG] * 2 and _pieces(q)[(7, 3)] == [ATOMIC] * 3      # 700 and 1,400 pairs
    assert _pieces(p3)[(3, 3)] == [ATOMIC | DIAG] and _pieces(p3)[(7, 3)] == [0]


@pytest.mark.parametrize("mode,n", [(m, n) for m in sc.BOTH for n in sc.TILE_COUNTS[m]])
def test_premises_of_the_tile_boundaries(mode, n):
    dc = 9 if mode == "selfcal" else 6
    cpt = NB // dc
    q, p3 = _lists(f"tiles_{n}", dc)
    if n == 1:
        assert len(p3["tasks"]) == 0 and len(p3["recs"]) == 0 and len(q["tasks"]) == 0
        return
    for pl in (p3,) + ((q,) if q is not None else ()):
        where = {(int(ci), int(cj)): int(dst) for dst, ci, cj, fl in pl["blocks"]}
        want = [(n - 1, 0)] + [(b, b - 1) for b in range(cpt, n, cpt)] + [(b + 1, b - 2) for b in range(cpt, n - 1, cpt)]
        for ci, cj in want:
            I, J = ci // cpt, cj // cpt
            assert where[(ci, cj)] == (I * (I + 1) // 2 + J) * NB * NB + (ci % cpt) * dc * NB + (cj % cpt) * dc
        assert sum(1 for ci, cj in want if ci // cpt != cj // cpt) == len(want) - (1 if n <= cpt else 0)
    assert (n * dc + NB - 1) // NB == (n + cpt - 1) // cpt and (n % cpt != 0) == (n not in (16, 24))   # a last partial tile


def test_premises_of_the_many_tiny_blocks():
    q, p3 = _lists("tiny", 9)
    _, p6 = _lists("tiny", 6)
    assert _max_blocks_in_a_chunk(p3) > 4 and _max_blocks_in_a_chunk(p6) > 4       # kPairDmaBlocks: cameras gathered from memory
    assert len(_pieces(q)) == 40 * 39 // 2 and all(v == [0] for v in _pieces(q).values())


def test_premises_of_the_wide_row():
    n_cam, n_pt, ci, pi = _indices("wide")
    q = capi.pair_lists_queued(n_cam, n_pt, ci, pi, 9)
    partners = np.bincount(q["blocks"][:, 1].astype(np.int64), minlength=n_cam)
    assert partners.max() >= 2049 and int((partners > 2048).sum()) == n_cam - 2049      # kRecsLdsPartners = 2048
    d = sc.problem("wide")
    jc, jl, r = np_blocks(d, 9)
    assert sr.SchurRef(n_cam, d.n_pt, d.cam_idx, d.pt_idx, jc, jl, r, 1e-3, np.float64, dense=False).cond.max() <= 1e8
    assert n_cam - 2049 <= 16                                                              # the smallest such structure, give or take a tile
