"""Crafted structures for the sharded bundle-adjustment path (tests/test_shard_cases_host.py checks their
premises through the host-arithmetic entries, tests/test_gpu_shard_crafted.py runs them rank by rank on the device).  A case is
(n_cam, per-landmark camera lists, lambda, mode, worlds); the numbers in the names are the decision points they sit on:
kLmWg = 128 landmarks per workgroup of the landmark-major kernels (cuts at 1, 127 .. 129, 255 .. 257), shard_range's
observation-balanced cut (a heavy landmark, world > n_pt, a landmark without observations at a cut), 16 (nine columns) / 24 (six
columns) cameras per tile, partition_columns' cut of the tile elimination tree (one root, k leaves)."""
import functools

import numpy as np

import np_ref_ba_loss as nb
import schur_ref as sr
from apex_solver_amd import capi
from apex_solver_amd.loss import Loss
from ba_custom import custom_problem

LAM = 1e-3
LM_WG = 128
CUTS = (1, 127, 128, 129, 255, 256, 257)
# world = 3: (first cut, second cut, n_pt); every cut of CUTS is also hit at this world
CUTS3 = {"1_2": (1, 2, 3), "127_255": (127, 255, 383), "128_256": (128, 256, 384), "129_257": (129, 257, 385)}
LOSSES = {"huber": Loss(capi.LOSS_HUBER, 1.0), "cauchy": Loss(capi.LOSS_CAUCHY, 2.0)}    # (Huber as schur_cases; Cauchy redescends)
ARROWS = {"arrow_2": (2, 0), "arrow_3": (3, 0), "arrow_pad_2": (3, 5), "arrow_pad_3": (4, 5)}     # name -> (leaf groups, tail cameras)


def _spread(total, n):
    """n observation counts in 2 .. 4 that sum to `total`"""
    assert 2 * n <= total <= 4 * n, (total, n)
    out = np.full(n, total // n)
    out[: total - out.sum()] += 1
    return out.tolist()


def _cams(rng, n_cam, k, lo=0):
    return sorted((lo + rng.choice(n_cam, size=k, replace=False)).tolist())


def _boundary(segments, rng, n_cam=20):
    """segments: [(landmarks, observations)], one per rank: every segment carries the same number of observations, so that
    shard_range's targets n_obs r / world fall exactly on the segment ends."""
    lists = []
    for n, total in segments:
        lists += [_cams(rng, n_cam, k) for k in _spread(total, n)]
    return n_cam, lists


def _arrow(k, tail):
    """k leaf groups of 16 cameras whose landmarks stay inside the group, then a hub group of 16 that shares landmarks with every
    leaf group (one leaf group per landmark: no leaf-leaf tile), then `tail` cameras of a capture of their own (a second root,
    the partial last tile).  A few landmarks are seen by hub cameras only; in arrow_3 one camera sees one landmark twice."""
    lists = []
    hub = 16 * k
    ring = lambda j, offs, n, lo: sorted(lo + (j + o) % n for o in offs)
    for g in range(k):
        # every camera of the group in two to five landmarks: the largest eigenvalue of S grows with the observations of one
        # camera, the smallest is lambda, and the whole S has to stay under cond 1e8 at lambda = 1e-3
        lists += [ring(j, (0, 5, 11)[: 2 + j % 2], 16, 16 * g) for j in range(16)]
        lists += [ring(2 * j, (0, 1), 16, 16 * g) + ring(2 * j + g, (0, 7)[: 1 + j % 2], 16, hub) for j in range(8)]
    lists += [ring(4 * j, (0, 5, 10), 16, hub) for j in range(4)]          # top cameras only
    if k == 3 and not tail:
        lists += [[3, 3, 9]]                                               # arrow_3: camera 3 twice (its assembly adds atomically)
    if tail:
        lists += [ring(j, (0, 2, 3)[: 2 + j % 2], tail, hub + 16) for j in range(8)]
    return hub + 16 + tail, lists


@functools.lru_cache(maxsize=None)
def structure(name):
    """(n_cam, lists, lambda, mode, worlds) of a named case."""
    rng = np.random.default_rng(41)
    if name.startswith("boundary3_"):
        a, b, n = CUTS3[name[10:]]
        total = 3 * max(a, b - a, n - b)
        return _boundary([(a, total), (b - a, total), (n - b, total)], rng) + (LAM, "selfcal", (3,))
    if name.startswith("boundary_"):
        c = int(name[9:])
        return _boundary([(c, 3 * c), (c, 3 * c)], rng) + (LAM, "selfcal", (2,))
    if name == "empty_heavy":
        # landmark 5 holds half the observations, landmark 6 none: at world = 4 the cuts are 5, 6, 6
        lists = [_cams(rng, 20, 2) for _ in range(5)] + [list(range(20))] + [[]] + [_cams(rng, 20, 2) for _ in range(5)]
        return 20, lists, LAM, "selfcal", (4,)
    if name == "empty_world8":
        return 20, [_cams(rng, 20, 3) for _ in range(3)], LAM, "selfcal", (8,)
    if name == "six_20":
        return _boundary([(128, 384), (128, 384)], rng) + (LAM, "ba", (2,))
    if name == "six_25":
        return _boundary([(40, 120), (40, 120), (40, 120)], rng, n_cam=25) + (LAM, "ba", (3,))
    if name in ARROWS:
        k, tail = ARROWS[name]
        return _arrow(k, tail) + (LAM, "selfcal", (3,) if name.endswith("3") else (2,))
    raise KeyError(name)


BOUNDARY_CASES = [f"boundary_{c}" for c in CUTS] + [f"boundary3_{k}" for k in CUTS3]
RANGE_CASES = BOUNDARY_CASES + ["empty_heavy", "empty_world8", "six_20", "six_25"]
ALL_CASES = RANGE_CASES + list(ARROWS)


@functools.lru_cache(maxsize=None)
def problem(name):
    """The case as problem data: noisy observations, every fifth factor an outlier far beyond the Huber threshold."""
    n_cam, lists, lam, mode, worlds = structure(name)
    # (arrows: the whole S must stay under cond 1e8 at lambda = 1e-3.  Its smallest eigenvalue is lambda, its largest at least
    # |J_c|^2 of one observation, which reaches 1e5 on the generator's cameras: the seed is one whose largest stays below that)
    return custom_problem(n_cam, lists, seed=48 if name in ARROWS else 29, outlier_every=5)


def ranges(d, world):
    """shard_range's [lo, hi) of every rank"""
    return [capi.shard_range(d.pt_idx, d.n_pt, r, world) for r in range(world)]


def host(name, world, rank, tree=1):
    n_cam, lists, lam, mode, worlds = structure(name)
    d = problem(name)
    return capi.host_structure(d.n_cam, d.n_pt, d.cam_idx, d.pt_idx, mode=1 if mode == "selfcal" else 0, rank=rank, world=world,
                               tree_sharding=tree, schur_form=4 if mode == "selfcal" else 3)


def lambda_cameras(name, world, rank, tree=1):
    """Boolean (n_cam): the cameras whose diagonal block of the rank's partial S carries lambda -- rank 0 under range sharding,
    the owner of the camera's tile column under tree sharding (rank 0 for the shared top)."""
    hs = host(name, world, rank, tree)
    n_cam, mode = structure(name)[0], structure(name)[3]
    if not hs["tree_sharded"]:
        return np.full(n_cam, rank == 0)
    assert np.array_equal(hs["cmap"], np.arange(n_cam))          # (under 23 tile rows: the caller's camera order)
    owner = hs["tile_owner"][np.arange(n_cam) // (16 if mode == "selfcal" else 24)]
    return (owner == rank) | ((owner < 0) & (rank == 0))


def np_blocks(d, dc, loss):
    """The corrected blocks of the numpy restatement at the problem's initial parameters, in the handle's export format."""
    r, jp, jl, ji, _, _ = nb.linearize(d.poses, d.intr, d.points, d.cam_idx.astype(int), d.pt_idx.astype(int), d.obs_uv, loss)
    return (np.concatenate([jp, ji], axis=2) if dc == 9 else jp), jl, r.ravel()


def rank_reference(d, jc, jl, r, lam, owned, lam_cams, dense=True):
    """(long double, fp64) reference of ONE rank's partial system: schur_ref.pair over the observations of the owned landmarks
    only, lambda on H_ll of every landmark and on the diagonal blocks of the cameras in lam_cams only."""
    sel = np.asarray(owned, dtype=bool)[d.pt_idx.astype(int)]
    return sr.pair(d.n_cam, d.n_pt, d.cam_idx[sel], d.pt_idx[sel], jc[sel], jl[sel], np.asarray(r).reshape(-1, 2)[sel], lam, dense=dense,
                   lam_cams=lam_cams)


def rank_cost(d, owned, loss):
    sel = np.asarray(owned, dtype=bool)[d.pt_idx.astype(int)]
    if not sel.any():
        return 0.0
    return nb.cost(d.poses, d.intr, d.points, d.cam_idx[sel].astype(int), d.pt_idx[sel].astype(int), d.obs_uv[sel], loss)


def block_bound(ld, f64):
    """schur_ref.block_check's bound of every camera pair: max(8 e_np, gamma(P) M), zero where no term is summed"""
    e_np = np.abs(np.asarray(f64.S4, dtype=sr.LD) - ld.S4).max(axis=(2, 3)).astype(np.float64)
    bound = np.maximum(8.0 * e_np, sr.gamma(ld.P) * ld.M)
    bound[ld.P == 0] = 0.0
    return bound


def sum_check(S4_sum, whole_ld, rank_refs):
    """Ratios of the summed partial S against the whole-problem reference under the sum of the ranks' own bounds."""
    err = np.abs(np.asarray(S4_sum, dtype=sr.LD) - whole_ld.S4).max(axis=(2, 3)).astype(np.float64)
    return sr._ratio(err, sum(block_bound(ld, f64) for ld, f64 in rank_refs))
