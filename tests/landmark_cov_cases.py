"""Crafted structures for the landmark covariance pass (k_landmark_cov, csrc/cov_kernels.hip; lc_setup, csrc/solver.hip):
tests/test_landmark_cov_ref_host.py asserts their premises on the host, tests/test_gpu_landmark_cov_crafted.py runs them.  A
case is (n_cam, per-landmark camera lists, modes); the numbers in the names are the decision points they sit on: kLcSmallK = 8
observations (8-lane groups, sixteen per workgroup) against a 64-lane workgroup per landmark in chunks of kLcChunk = 32, and
16 (nine columns) / 24 (six columns) cameras per tile of Z.

lambda is LAMBDA below for every case and mode: 1 without the Jacobi scaling (kappa(S) of the fp64 restatement 1e5 .. 4e5
under every loss; at 0.1 it passes 1e6) and 1e-3 with it (the scaled columns have norm < 1: kappa(S) 2e3 .. 6e3; at 1 the
correction term would vanish beside H_ll^-1).  Measured on the CPU; asserted <= 1e6 by the host test and again by the device
test on the device's own linearisation.

The one exception is `gate`: the landmark the eigenvalue gate regularises has max_ev > 1e10 lambda (4.2e10 here), its camera
keeps about (1 + |p|^2) 1e-6 max_ev of that in S (|p| ~ 10: the landmark sits at the camera, ten units from the origin) and the
gauge directions of S stay at lambda: kappa(S) > 1e6 whenever the gate fires, 101 x 4.2e4 = 4e6 here.  That case asserts
kappa(S) <= GATE_KAPPA = 1e7 instead (no base was found where the gate fires below 1e6: with forty times the landmarks and
max_ev at 1.7e10 the self-calibration S still has lambda_min = 1.01 lambda and kappa 2.8e6), the floor of the rule carries the
kappa it has -- 4e-7 of M_l, and the host test shows that it still rejects a faulty kernel on the gated landmark and on its
camera's neighbours -- and the case runs without a loss and without scaling only: a robust weight or the scaling takes the
block out of the gate's reach.  The reference of this case takes the device's exported S as the matrix (landmark_cov_ref,
S_given); the host test asserts that no block of it adds atomically, so the export has the factorised bits."""
import functools

import numpy as np

import apex_solver_amd as pkg
import schur_cases as sc
from ba_custom import custom_problem

LADDER_K = (1, 2, 7, 8, 9, 10, 31, 32, 33, 63, 64, 65, 96, 97)
LADDER_CAMS = 100
GROUP_COUNTS = (15, 16, 17)
TILE_CASES = {"selfcal": (16, 17, 33), "ba": (24, 25, 49)}
FILL_CAMS = 52
BOTH = ("selfcal", "ba")
GATE_FRAC, GATE_KAPPA = 4e-4, 1e7


def spread(n, k, off):
    """k distinct cameras spread evenly over the ring of n, starting at off: wide baselines at every k"""
    cams = sorted({(off + (j * n) // k) % n for j in range(k)})
    assert len(cams) == k
    return cams


def _ring(n, step=1):
    """three cameras a seventh and a third of the ring apart per starting camera: S connected, H_ll well conditioned"""
    return [sorted({c, (c + max(n // 7, 1)) % n, (c + max(n // 3, 2)) % n}) for c in range(0, n, step)]


def _small_lists(n, count, seed):
    """`count` small landmarks with k cycling through 1 .. 8"""
    rng = np.random.default_rng(seed)
    return [spread(n, 1 + i % 8, int(rng.integers(n))) for i in range(count)]


@functools.lru_cache(maxsize=None)
def structure(name):
    """(n_cam, per-landmark camera lists, modes the case runs in) of a named case."""
    if name == "k_ladder":
        n = LADDER_CAMS
        lists = [spread(n, k, 7 * r) for r, k in enumerate(LADDER_K)]
        assert len({tuple(c) for c in lists}) == len(lists)
        return n, lists + _ring(n), BOTH
    if name.startswith("groups_"):
        return 12, _small_lists(12, int(name[7:]), 3), BOTH
    if name == "only_large":
        n = 40
        return n, [spread(n, k, 5 * r) for r, k in enumerate((9, 12, 33, 40, 20, 9, 34))], BOTH
    if name == "large_first":                      # landmark 0 is the one large landmark; 17 small ones: one active group in the last workgroup
        n = 40
        return n, [spread(n, 40, 0)] + _small_lists(n, 17, 5), BOTH
    if name == "dup":
        n = 30
        # the library orders a landmark's observations by camera: 0 .. 5, 5, .. 28 fill positions 0 .. 29, camera 29 sits at
        # positions 30 .. 33 -- twice in the first chunk of 32 and twice in the second
        big = list(range(n - 1)) + [5] + [n - 1] * 4
        lists = [[5, 5, 9], [4, 4, 4, 8], big, [0, 1], [1, 2, 9], [5, 6, 7], [2, 8], [0, 9, 4]] + _ring(n, 3)
        return n, lists, BOTH
    if name.startswith("tiles_"):
        n = int(name[6:])
        mode = "selfcal" if n in TILE_CASES["selfcal"] else "ba"
        return sc._tiles(n, 16 if mode == "selfcal" else 24) + ((mode,),)
    if name == "fill":                             # a banded chain (every landmark inside 16 cameras) and three landmarks from the first tile to the last
        n = FILL_CAMS
        lists = [[c, c + 1, c + 2] for c in range(n - 2)] + [[c, c + 5, c + 11] for c in range(0, n - 11, 2)]
        lists += [[0, n - 2], [3, n - 3], [1, 2, n - 1]]
        return n, lists, ("selfcal",)
    if name == "behind":                           # landmarks 0 (k = 4) and 1 (k = 40) and one ring landmark hold camera 10
        n = 40
        return n, [spread(n, 4, 0), spread(n, 40, 0)] + _small_lists(n, 12, 7) + _ring(n, 2), BOTH
    if name == "gate":                             # plus one landmark close to a camera: problem()
        return 12, _small_lists(12, 20, 11) + _ring(12), BOTH
    raise KeyError(name)


CASES = (["k_ladder"] + [f"groups_{c}" for c in GROUP_COUNTS] + ["only_large", "large_first", "dup"]
         + [f"tiles_{n}" for m in BOTH for n in TILE_CASES[m]] + ["fill", "behind", "gate"])
BEHIND_LANDMARKS, BEHIND_CAM = (0, 1), 10   # of `behind`: a small and a large landmark that camera 10 sees from behind
LAMBDA = {False: 1.0, True: 1e-3}  # by Jacobi scaling off / on: see the module docstring


def lam_of(name, mode, scaled=False):
    """lambda of a run.  Chosen per case and mode from the kappa(S) measured at powers of ten; the same two values came out for
    every one of them (test_camera_order_and_conditioning asserts the premise case by case)."""
    return LAMBDA[bool(scaled)]


def with_close_landmark(d, frac):
    """d plus one landmark seen by ONE camera, on the ray of an observation in front of its camera but `frac` of the way from
    the camera centre: H_ll of rank 2 and 1 / frac^2 larger (as in tests/test_gpu_landmark_covariance.py)."""
    import np_ref
    for i in range(d.n_obs):
        c, p = int(d.cam_idx[i]), int(d.pt_idx[i])
        R = np_ref.quat_to_R(d.poses[c:c + 1, 3:7])[0]
        if (R @ d.points[p] + d.poses[c, 0:3])[2] < -0.5:     # in front (the camera looks down -z)
            break
    centre = -R.T @ d.poses[c, 0:3]
    newp = centre + frac * (d.points[p] - centre)
    return pkg.synthetic.BAProblemData(
        poses=d.poses, intr=d.intr, points=np.vstack([d.points, newp[None]]),
        cam_idx=np.append(d.cam_idx, d.cam_idx[i]).astype(d.cam_idx.dtype),
        pt_idx=np.append(d.pt_idx, d.n_pt).astype(d.pt_idx.dtype),
        obs_uv=np.vstack([d.obs_uv, d.obs_uv[i][None]]), name=d.name)


def _turn_round(poses, cam):
    """camera `cam` turned by pi about its own x axis: p_cam -> diag(1, -1, -1) p_cam, everything it saw is behind it now"""
    w, x, y, z = poses[cam, 3:7]
    poses[cam, 3:7] = (-x, w, -z, y)              # (0, 1, 0, 0) (x) q
    poses[cam, 1:3] *= -1.0


@functools.lru_cache(maxsize=None)
def problem(name):
    """The case as problem data: noisy observations, every fifth factor an outlier far beyond the Huber threshold."""
    n_cam, lists, modes = structure(name)
    d = custom_problem(n_cam, lists, seed=23, outlier_every=5)
    if name == "behind":
        d = pkg.synthetic.BAProblemData(d.poses.copy(), d.intr, d.points, d.cam_idx, d.pt_idx, d.obs_uv)
        _turn_round(d.poses, BEHIND_CAM)
    if name == "gate":
        d = with_close_landmark(d, GATE_FRAC)
    return d


def gated_landmark(name, d):
    """the one landmark of the one case that may leave the plain-inverse regime of the gate"""
    return d.n_pt - 1 if name == "gate" else None
