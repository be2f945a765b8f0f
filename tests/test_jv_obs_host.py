"""jv_obs (apex-solver_amd/csrc/ba_device.hpp: J_o a and J_o b without holding J_o, the Gram pass of Dog-Leg) against
linearize_obs, both compiled for the host.  With unit vectors jv_obs must reproduce every entry of Jc and Jl BIT FOR BIT -- the
column masks of every OptimizeParams combination, the zero rows of a point behind its camera and sqrt(rho') of both loss forms
included -- so that an edit to one of the two functions cannot leave the other behind unnoticed.  No GPU needed."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import apex_solver_amd as pkg
from apex_solver_amd import capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_f = np.ctypeslib.ndpointer(dtype=np.float64, flags="C_CONTIGUOUS")


@pytest.fixture(scope="module")
def hj():
    out = os.path.join(ROOT, "tests", "_build")
    os.makedirs(out, exist_ok=True)
    so = os.path.join(out, "libhost_harness_jv.so")
    subprocess.run(["g++", "-O2", "-ffp-contract=off", "-std=c++17", "-shared", "-fPIC", "-I", os.path.join(ROOT, "apex-solver_amd", "csrc"),
                    os.path.join(ROOT, "tests", "host_harness_jv.cpp"), "-o", so], check=True)
    L = C.CDLL(so)
    L.hj_compare.argtypes = [C.c_int, C.c_int, _f, _f, _f, _f, C.c_int, C.c_double, C.c_double, _f, _f]
    L.hj_jv.argtypes = [C.c_int, _f, _f, _f, _f, C.c_double, _f, _f, _f, _f]
    return L


@pytest.fixture(scope="module")
def data():
    d = pkg.synthetic.make_problem(9, 120, 3, 6, config_id=55, behind_frac=0.05)
    poses = d.poses.copy(); poses[:, 3:] *= (1 + 1e-9 * np.arange(9))[:, None]   # un-normalised quaternions, as after a retraction
    return d, poses


LOSSES = {"none": (-1, -1.0, 0.0), "huber": (-1, 1.0, 0.0), "cauchy": (capi.LOSS_CAUCHY, 2.0, 0.0), "tukey": (capi.LOSS_TUKEY, 3.0, 0.0)}


@pytest.mark.parametrize("loss", list(LOSSES))
@pytest.mark.parametrize("dc", [6, 9])
def test_unit_vectors_reproduce_every_entry_bit_for_bit(hj, data, dc, loss):
    d, poses = data
    kind, p0, p1 = LOSSES[loss]
    n_invalid = 0
    for mask in range(1, 8):
        for i in range(d.n_obs):
            c, l = int(d.cam_idx[i]), int(d.pt_idx[i])
            Jl, Jv = np.empty(2 * (dc + 3)), np.empty(2 * (dc + 3))
            bad = hj.hj_compare(dc, mask, poses[c], d.intr[c], d.points[l], d.obs_uv[i], kind, p0, p1, Jl, Jv)
            assert bad in (0, 1000), (mask, i, bad, Jl, Jv)
            assert np.array_equal(Jl, Jv)
            if bad == 1000:
                n_invalid += 1
                assert not Jl.any()
            elif mask == 7 and loss != "tukey":   # (Tukey cuts some observations: rho' = 0, an all-zero block)
                J = Jl.reshape(2, dc + 3)
                assert J[:, :6].any() and J[:, dc:].any()
            if mask in (1, 2, 4) and bad == 0:   # one group alone: the other columns are exact zeros
                J = Jl.reshape(2, dc + 3)
                groups = {4: J[:, :6], 2: J[:, dc:], 1: J[:, 6:dc]}
                for m, blk in groups.items():
                    assert (m == mask) or not blk.any()
    assert n_invalid >= 7   # points behind their camera took part, under every mask


def test_general_vectors_are_the_matrix_product(hj, data):
    d, poses = data
    rng = np.random.default_rng(1)
    for dc in (6, 9):
        n = dc + 3
        for i in range(0, d.n_obs, 7):
            c, l = int(d.cam_idx[i]), int(d.pt_idx[i])
            Jl, Jv = np.empty(2 * n), np.empty(2 * n)
            if hj.hj_compare(dc, 7, poses[c], d.intr[c], d.points[l], d.obs_uv[i], -1, 1.0, 0.0, Jl, Jv) != 0:
                continue
            a, b = rng.normal(size=n), rng.normal(size=n)
            u, w = np.empty(2), np.empty(2)
            assert hj.hj_jv(dc, poses[c], d.intr[c], d.points[l], d.obs_uv[i], 1.0, a, b, u, w) == 1
            J = Jl.reshape(2, n)
            scale = np.abs(J) @ np.abs(a), np.abs(J) @ np.abs(b)
            assert (np.abs(u - J @ a) <= 1e-14 * scale[0]).all() and (np.abs(w - J @ b) <= 1e-14 * scale[1]).all()
