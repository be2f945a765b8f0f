"""What GpuSchurComplementSolver (solver.py) and GpuSparseCholeskySolver (pose_graph.py) share: every call the library offers
under both prefixes with the same arguments, apexgpu_<name> and apexgpu_pg_<name>, written once against the handle's prefix
(capi._HandleBase._call).  tests/test_frontend_surface_host.py holds the two halves of capi.API to that condition for every
name used here.

A subclass supplies
  _need()        its handle, or _built(code): the LinAlgError of its own code before initialize_structure
  _total_dof()   the tangent dimension of the built problem
  _variant()     what an LM run puts into the C config's `variant`
  _STAGE_NAMES   the stages of its stage_times, in the library's order
"""
from __future__ import annotations

import ctypes as C
from typing import TYPE_CHECKING

import numpy as np

from . import capi
from .loss import Loss

if TYPE_CHECKING:
    from .pose_graph import DogLegConfig


class HandleSolver:
    _STAGE_NAMES: tuple = ()

    def __init__(self, device: int = 0):
        self.device = device
        self._h = None
        self._options: dict[str, int] = {}   # with_option: applied to the new handle by initialize_structure
        self._gradient = None                # of the last solve_augmented_equation
        self._scaling = None                 # of the last apply_column_scaling

    def with_option(self, name: str, value: int):
        """An implementation switch that must be set before initialize_structure (e.g. nested_dissection)."""
        self._options[name] = int(value)
        return self

    def _apply_options(self, h):
        for k, v in self._options.items():
            h._call("set_option", k.encode(), v)

    def _built(self, code: int):
        if self._h is None:
            raise capi.LinAlgError(code, "Block structure not built. Call initialize_structure() first.")
        return self._h

    def set_loss(self, loss: Loss | None):
        """The loss of every ProjectionFactor / BetweenFactor block from here on (None: no loss); replaces the problem's
        huber_delta until the next initialize_structure.  Bundle adjustment: InvalidInput for the kinds whose corrector needs more
        than one weight per observation (Andrews, lp with p > 2, Barron with alpha > 2); with several ranks every rank sets the
        same loss."""
        loss = Loss(capi.LOSS_NONE) if loss is None else loss
        self._need()._call("set_loss", int(loss.kind), float(loss.p0), float(loss.p1))

    def get_loss(self) -> Loss:
        k = C.c_int(); p = (C.c_double * 2)()
        self._need()._call("get_loss", C.byref(k), C.byref(p))
        return Loss(k.value, p[0], p[1])

    def compute_cost(self) -> float:
        c = C.c_double()
        self._need()._call("cost", C.byref(c))
        return c.value

    # LinearSolver::solve_normal_equation (solve_augmented_equation: the subclass)
    def solve_normal_equation(self):
        return self.solve_augmented_equation(0.0)

    def get_gradient(self):
        """+J^T r of the last solve (explicit_schur.rs:1240-1242); None before any solve."""
        return self._gradient

    # AssemblyBackend::compute_column_norms / apply_column_scaling / apply_inverse_scaling (linearizer/mod.rs:229-262)
    def compute_column_norms(self) -> np.ndarray:
        h = self._need()
        n = np.zeros(self._total_dof())
        h._call("column_norms", capi.ptr(n))
        return n

    def apply_column_scaling(self, scaling):
        """J -> J diag(scaling) for the following solves (None: off).  solve_augmented_equation then returns the
        scaled step and get_gradient the scaled gradient, like the reference's solver fed with the scaled Jacobian."""
        h = self._need()
        a = None if scaling is None else np.ascontiguousarray(scaling, dtype=np.float64)
        if a is not None and a.shape != (self._total_dof(),):
            raise ValueError("scaling must have total_dof entries")
        h._call("set_column_scaling", capi.ptr(a))
        self._scaling = a

    def apply_inverse_scaling(self, step):
        return step if self._scaling is None else step * self._scaling

    # the trial-step protocol: a solve leaves a trial point; eval_step prices it, commit_step / discard_step end it
    def step_stats(self):
        out = (C.c_double * 3)()
        self._need()._call("step_stats", C.byref(out))
        return tuple(out)

    def eval_step(self) -> float:
        c = C.c_double()
        self._need()._call("eval_step", C.byref(c))
        return c.value

    def commit_step(self):
        self._need()._call("commit_step")

    def discard_step(self):
        self._need()._call("discard_step")

    def parameter_norm(self) -> float:
        c = C.c_double()
        self._need()._call("parameter_norm", C.byref(c))
        return c.value

    def covariance_stats(self, group_cap: int = 0) -> dict:
        h = self._need()
        out = (C.c_double * 6)()
        ms = np.zeros(max(int(group_cap), 1))
        h._call("covariance_stats", C.byref(out), capi.ptr(ms), int(group_cap))
        return dict(extra_bytes=int(out[0]), y_products=int(out[1]), zoff_products=int(out[2]), zdiag_products=int(out[3]),
                    level_groups=int(out[4]), group_ms=ms[:int(out[5])].tolist())

    def counters(self) -> dict:
        """Events of this handle's life: dataflow triangular sweeps that timed out and were repeated level by level."""
        out = (C.c_int64 * 4)()
        self._need()._call("counters", C.byref(out))
        return dict(sweep_timeouts=int(out[0]), tri_dataflow=bool(out[1]), factor_flow_timeouts=int(out[2]), factor_flow_groups=int(out[3]))

    def set_option(self, name: str, value: int):
        self._need()._call("set_option", name.encode(), int(value))

    def enable_stage_timing(self, on=True):
        self._need()._call("enable_stage_timing", int(on))

    def reset_stage_times(self):
        self._need()._call("reset_stage_times")

    def stage_times(self) -> dict:
        k = len(self._STAGE_NAMES)
        ms = (C.c_double * k)(); n = (C.c_int64 * k)()
        self._need()._call("stage_times", C.byref(ms), C.byref(n))
        return {name: (ms[i], n[i]) for i, name in enumerate(self._STAGE_NAMES)}

    def _optimize(self, name: str, cfg, iter_type, variant: int | None = None):
        """One optimiser loop of the library (name: "lm_optimize", "gn_optimize", "dogleg_optimize") with cfg's C form:
        (result, history (iterations, fields of iter_type), the config as the loop left it)."""
        h = self._need()
        c = cfg.to_c()
        if variant is not None:
            c.variant = variant
        res = capi.LmResultC()
        cap = cfg.max_iterations + 2
        hist = (iter_type * cap)()
        h._call(name, C.byref(c), C.byref(res), C.cast(hist, C.c_void_p), cap)
        fields = [f for f, _ in iter_type._fields_]
        H = np.array([[getattr(hist[i], f) for f in fields] for i in range(min(res.iterations, cap))])
        return res, H.reshape(-1, len(fields)), c

    def lm_optimize(self, cfg):
        """LevenbergMarquardt's loop (levenberg_marquardt.rs:823-1031) on the device: (result, history (n, 8) in LmIterC's
        columns, the config as the loop left it -- damping holds its final value)."""
        return self._optimize("lm_optimize", cfg, capi.LmIterC, self._variant())

    # ---- Dog-Leg (dog_leg.rs) ----
    def dogleg_optimize(self, cfg: DogLegConfig):
        """DogLeg::optimize (dog_leg.rs:1143-1354) on the device: (result, history (n, 12) in DlIterC's columns, the config as
        the loop left it -- trust_region_radius and mu hold their final values).  LinAlgError: InvalidInput for cfg.variant != 0,
        InvalidState on a matrix-free or a sharded bundle-adjustment handle."""
        return self._optimize("dogleg_optimize", cfg, capi.DlIterC)

    def dogleg_step(self, mu: float, radius: float, reuse: bool = False) -> dict:
        """One Dog-Leg step and its trial point at the current parameters; eval_step / commit_step / discard_step follow.
        reuse: rebuild the step from the cached solve at the new radius (no assembly, factorisation, sweeps or
        back-substitution).  A failed factorisation raises FactorizationFailed / SingularMatrix without the ladder."""
        o = (C.c_double * 8)()
        self._need()._call("dogleg_step", float(mu), float(radius), 1 if reuse else 0, C.byref(o))
        return dict(gradient_norm=o[0], step_norm=o[1], predicted_reduction=o[2], step_type=int(o[3]), alpha=o[4], beta=o[5],
                    scaled_step_norm=o[6], reused=bool(o[7]))

    def jv_gram(self, a, b):
        """(|J a|^2, (J a).(J b), |J b|^2) at the current parameters, matrix-free; a, b in the global column order."""
        h = self._need()
        n = self._total_dof()
        a = np.ascontiguousarray(a, dtype=np.float64); b = np.ascontiguousarray(b, dtype=np.float64)
        if a.shape != (n,) or b.shape != (n,):
            raise ValueError("a and b must have total_dof entries")
        o = (C.c_double * 3)()
        h._call("jv_gram", capi.ptr(a), capi.ptr(b), C.byref(o))
        return o[0], o[1], o[2]

    def close(self):
        if self._h is not None:
            self._h.close()
            self._h = None
