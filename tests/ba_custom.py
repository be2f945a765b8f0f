"""Bundle-adjustment problems built from explicit per-landmark camera lists (shared by tests/test_gpu_parity.py,
tests/test_gpu_ba_loss.py, tests/test_schur_ref_host.py and tests/test_gpu_schur_crafted.py)."""
import numpy as np

import apex_solver_amd as pkg


def custom_problem(n_cam, cam_lists, seed=5, n_pt=None, noise=0.7, outlier_every=0, outlier_sigma=25.0):
    """A problem with explicit per-landmark camera lists (duplicates allowed; landmark l is seen by cam_lists[l]), on the
    cameras and points of the seeded generator.  The factor order is shuffled: the caller's order is arbitrary, the library
    sorts by landmark.  Observations are the truth's projections plus N(0, noise) pixels; with outlier_every = m > 0 every
    m-th factor gets N(0, outlier_sigma) on top (far beyond a Huber threshold of one pixel)."""
    n_pt = len(cam_lists) if n_pt is None else n_pt
    base = pkg.synthetic.make_problem(n_cam, n_pt, 3, 3, config_id=seed)
    cam_idx, pt_idx = [], []
    for l, cams in enumerate(cam_lists):
        cam_idx += list(cams); pt_idx += [l] * len(cams)
    cam_idx = np.asarray(cam_idx, dtype=np.uint32); pt_idx = np.asarray(pt_idx, dtype=np.uint32)
    rng = np.random.default_rng(seed)
    perm = rng.permutation(len(cam_idx))
    cam_idx, pt_idx = cam_idx[perm], pt_idx[perm]
    uv = pkg.synthetic.project_bal(base.truth_poses[cam_idx], base.truth_intr[cam_idx], base.truth_points[pt_idx])
    uv = uv + rng.normal(0, noise, uv.shape)
    if outlier_every > 0:
        uv[::outlier_every] += rng.normal(0, outlier_sigma, uv[::outlier_every].shape)
    return pkg.synthetic.BAProblemData(base.poses, base.intr, base.points, cam_idx, pt_idx, np.ascontiguousarray(uv))
