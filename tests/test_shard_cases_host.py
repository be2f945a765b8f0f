"""Premises of the crafted shard cases (tests/shard_cases.py), on the host-arithmetic entries and the references alone -- no
GPU: where shard_range cuts, which ranks are empty, how partition_columns cuts the arrow trees and who owns what, the
conditioning the bounds assume; and that the bounds of tests/test_gpu_shard_crafted.py reject the faults they are there for:
the unperturbed reference is held against a reference with the fault and must fail by a factor of at least 1e3."""
import numpy as np
import pytest

import shard_cases as shc
import schur_ref as sr
from apex_solver_amd import capi

SENSITIVITY = 1e3


def _owned(name, world, tree=1):
    return np.stack([shc.host(name, world, r, tree)["owned"] for r in range(world)])


@pytest.mark.parametrize("cut", shc.CUTS)
def test_two_rank_cut_positions(cut):
    d = shc.problem(f"boundary_{cut}")
    assert shc.ranges(d, 2) == [(0, cut), (cut, 2 * cut)]
    owned = _owned(f"boundary_{cut}", 2)
    assert not shc.host(f"boundary_{cut}", 2, 0)["tree_sharded"]
    assert np.array_equal(np.flatnonzero(owned[0]), np.arange(cut)) and (owned.sum(axis=0) == 1).all()


@pytest.mark.parametrize("key", list(shc.CUTS3))
def test_three_rank_cut_positions(key):
    a, b, n = shc.CUTS3[key]
    d = shc.problem(f"boundary3_{key}")
    assert d.n_pt == n and shc.ranges(d, 3) == [(0, a), (a, b), (b, n)]
    assert (_owned(f"boundary3_{key}", 3).sum(axis=0) == 1).all()


def test_every_named_cut_and_workgroup_premise_is_covered():
    cuts = {2: set(), 3: set()}
    for name in shc.BOUNDARY_CASES:
        world = shc.structure(name)[4][0]
        cuts[world] |= {lo for lo, hi in shc.ranges(shc.problem(name), world)[1:]}
    assert cuts[2] == set(shc.CUTS) and set(shc.CUTS) <= cuts[3] | {2}
    wg = lambda l: l // shc.LM_WG
    # a whole range inside one workgroup that it shares with both neighbours (rank 1 of 129 | 255), two ranks in one workgroup
    (_, h0), (l1, h1), (l2, _) = shc.ranges(shc.problem("boundary3_129_257"), 3)[:3]
    assert wg(l1) == wg(h0 - 1) == 1 and wg(h1 - 1) == wg(l2) == 2
    (l0, h0), (l1, h1) = shc.ranges(shc.problem("boundary_1"), 2)
    assert wg(l0) == wg(h0 - 1) == wg(l1) == wg(h1 - 1) == 0
    (l0, h0), (l1, h1), _ = shc.ranges(shc.problem("boundary3_127_255"), 3)
    assert wg(l1) == 0 and wg(h1 - 1) == 1 and wg(h1) == 1
    lo, hi = shc.ranges(shc.problem("boundary_127"), 2)[0]
    assert hi - lo == 127 and wg(hi) == 0                     # rank 0 within workgroup 0, which rank 1 enters at its last landmark


def test_empty_ranks():
    d = shc.problem("empty_heavy")
    assert np.bincount(d.pt_idx, minlength=d.n_pt)[5] * 4 > d.n_obs and np.bincount(d.pt_idx, minlength=d.n_pt)[6] == 0
    assert shc.ranges(d, 4) == [(0, 5), (5, 6), (6, 6), (6, 12)]         # rank 2 is empty; landmark 6 (no observation) sits at the cut
    owned = _owned("empty_heavy", 4)
    assert owned.sum(axis=1).tolist() == [5, 1, 0, 6] and (owned.sum(axis=0) == 1).all()
    d = shc.problem("empty_world8")
    assert d.n_pt == 3
    assert shc.ranges(d, 8) == [(0, 1), (1, 1), (1, 1), (1, 2), (2, 2), (2, 2), (2, 3), (3, 3)]
    owned = _owned("empty_world8", 8)
    assert owned.sum(axis=1).tolist() == [1, 0, 0, 1, 0, 0, 1, 0] and (owned.sum(axis=0) == 1).all()


def test_six_column_cases_are_range_sharded_and_25_cameras_cross_a_tile():
    for name, world in (("six_20", 2), ("six_25", 3)):
        hs = shc.host(name, world, 1)
        assert not hs["tree_sharded"] and hs["top_columns"] == 0
        assert (_owned(name, world).sum(axis=0) == 1).all()
    assert shc.host("six_25", 3, 0)["tile_rows"] == 2 and shc.host("six_20", 2, 0)["tile_rows"] == 1
    assert shc.ranges(shc.problem("six_20"), 2) == [(0, 128), (128, 256)]


def _present(name):
    n_cam, lists = shc.structure(name)[:2]
    nt = (9 * n_cam + 143) // 144
    pr = np.zeros((nt, nt), dtype=np.uint8)
    for cams in lists:
        t = np.unique(np.asarray(cams, dtype=int) // 16)
        pr[np.ix_(t, t)] = 1
    return np.tril(pr)


ARROW_OWNERS = {"arrow_2": [0, 1, -1], "arrow_3": [0, 1, 2, -1], "arrow_pad_2": [0, 1, 0, -1, 1], "arrow_pad_3": [0, 1, 2, 0, -1, 1]}


@pytest.mark.parametrize("name", list(shc.ARROWS))
def test_arrow_partition(name):
    """One root with k leaf subtrees (and, in the pad cases, a second root: the partial last tile on a rank other than 0)."""
    k, tail = shc.ARROWS[name]
    n_cam, lists, lam, mode, (world,) = shc.structure(name)
    pr = _present(name)
    nt = len(pr)
    assert nt == k + 1 + (tail > 0) and nt < 23
    assert all(pr[k, g] and pr[:, g].sum() == 2 for g in range(k))             # a leaf column: itself and the hub tile
    owner, n_top = capi.tile_partition(pr, world)
    assert n_top == 1 and owner.tolist() == ARROW_OWNERS[name]
    if tail:
        assert (9 * n_cam) % 144 != 0 and owner[-1] > 0
    for r in range(world):
        for tree in (1, 0):
            hs = shc.host(name, world, r, tree)
            assert hs["top_columns"] == 1 and hs["tree_sharded"] == tree and hs["tile_owner"].tolist() == ARROW_OWNERS[name]
            assert np.array_equal(hs["cmap"], np.arange(n_cam))
    for tree in (1, 0):
        assert (_owned(name, world, tree).sum(axis=0) == 1).all()
    # tree sharding: a landmark belongs to the owner of the first owned tile it touches; top-only landmarks to the least loaded
    owned = _owned(name, world, 1)
    top_only = [l for l, cams in enumerate(lists) if cams and all(owner[c // 16] < 0 for c in cams)]
    assert len(top_only) == 4
    for l, cams in enumerate(lists):
        ows = {int(owner[c // 16]) for c in cams if owner[c // 16] >= 0}
        assert len(ows) <= 1
        if ows:
            assert owned[ows.pop(), l]
    assert any(len(set(c)) < len(c) for c in lists) == (name == "arrow_3")        # a camera that sees a landmark twice
    lam_cams = np.stack([shc.lambda_cameras(name, world, r) for r in range(world)])
    assert (lam_cams.sum(axis=0) == 1).all() and lam_cams[1:].any()


@pytest.mark.parametrize("loss", ["huber", "cauchy"])
@pytest.mark.parametrize("name", shc.ALL_CASES)
def test_conditioning(name, loss):
    n_cam, lists, lam, mode, worlds = shc.structure(name)
    d = shc.problem(name)
    dc = 9 if mode == "selfcal" else 6
    jc, jl, r = shc.np_blocks(d, dc, shc.LOSSES[loss])
    ref = sr.SchurRef(n_cam, d.n_pt, d.cam_idx, d.pt_idx, jc, jl, r, lam, np.float64, dense=name in shc.ARROWS)
    assert ref.cond.max() <= 1e8, ref.cond.max()
    if name in shc.ARROWS:
        S = sr.dense_of(ref.S4, np.arange(n_cam * dc).reshape(n_cam, dc), n_cam * dc)
        assert np.linalg.cond(S) <= 1e8, np.linalg.cond(S)


# ---- sensitivity: the device bounds see the faults they are meant for -------------------------------------------------------------
@pytest.fixture(scope="module")
def rank1():
    """Rank 1 of 129 | 257: its range [129, 257) starts one landmark into workgroup 1 and ends one landmark into workgroup 2."""
    name = "boundary3_129_257"
    d = shc.problem(name)
    jc, jl, r = shc.np_blocks(d, 9, shc.LOSSES["huber"])
    owned = _owned(name, 3)[1]
    lam_cams = shc.lambda_cameras(name, 3, 1)
    assert not lam_cams.any()
    good = shc.rank_reference(d, jc, jl, r, shc.LAM, owned, lam_cams)
    ratio, bad = sr.block_check(good[1].S4, *good)
    assert not bad
    return d, (jc, jl, r), owned, lam_cams, good


def _worst_block(good, faulty):
    """the largest ratio of the unperturbed fp64 partial S held against the faulty reference"""
    ratio, bad = sr.block_check(good[1].S4, *faulty)
    return ratio.max(), bad


def test_bound_sees_a_boundary_landmark_on_the_wrong_rank(rank1):
    d, blocks, owned, lam_cams, good = rank1
    for l in (128, 257):                                        # the neighbours' last / first landmark
        moved = owned.copy(); moved[l] = True
        worst, bad = _worst_block(good, shc.rank_reference(d, *blocks, shc.LAM, moved, lam_cams))
        cams = set(shc.structure("boundary3_129_257")[1][l])
        assert worst >= SENSITIVITY and {i for ij in bad for i in ij} == cams, (l, worst)
        # and the landmark's own record: H_ll^-1 of a landmark with its observations against lambda^-1 I without them
        faulty = shc.rank_reference(d, *blocks, shc.LAM, moved, lam_cams, dense=False)
        v = sr.vec_check(good[1].Hinv, faulty[0].Hinv, faulty[1].Hinv, faulty[0].hinv_mag, faulty[0].k_l)
        assert v[l] >= SENSITIVITY and (np.delete(v, l) <= 1.0).all()


def test_bound_sees_lambda_on_every_rank(rank1):
    d, blocks, owned, lam_cams, good = rank1
    faulty = shc.rank_reference(d, *blocks, shc.LAM, owned, np.ones_like(lam_cams))
    ratio, bad = sr.block_check(good[1].S4, *faulty)
    assert set(bad) == {(c, c) for c in range(d.n_cam)} and np.diag(ratio).min() >= SENSITIVITY, np.diag(ratio).min()
    x = np.random.default_rng(3).normal(size=(d.n_cam, 9))
    y, mag = faulty[0].matvec(x)
    v = sr.vec_check(good[1].matvec(x)[0], y, faulty[1].matvec(x)[0], mag, faulty[0].matvec_terms())
    print("lambda on every rank: S", np.diag(ratio).min(), "S x", v.max())


def test_bound_sees_a_non_owned_landmark_of_a_boundary_workgroup_with_its_observations(rank1):
    d, blocks, owned, lam_cams, good = rank1
    for l in (3 * 128 - 1, 260):                                # workgroup 2 holds rank 1's landmark 256 and rank 2's 257 .. 383
        assert not owned[l] and l // shc.LM_WG == 2
        given = owned.copy(); given[l] = True
        worst, bad = _worst_block(good, shc.rank_reference(d, *blocks, shc.LAM, given, lam_cams))
        assert worst >= SENSITIVITY and bad, (l, worst)
        faulty = shc.rank_reference(d, *blocks, shc.LAM, given, lam_cams, dense=False)
        g = sr.vec_check(good[1].gred, faulty[0].gred, faulty[1].gred, faulty[0].gred_mag, faulty[0].gred_terms)
        assert g.max() >= SENSITIVITY
