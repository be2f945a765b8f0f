"""The robust loss family as both front ends take it (bundle adjustment: solver.py, pose graphs: pose_graph.py): `Loss`, one
loss of src/core/loss_functions.rs in the C ABI's terms, and `create_loss_function`, the names of bin/pose_graph_g2o.rs."""
from __future__ import annotations

import ctypes as C
from dataclasses import dataclass

import numpy as np

from . import capi


@dataclass(frozen=True)
class Loss:
    """One loss of src/core/loss_functions.rs as the C ABI takes it: kind = capi.LOSS_*, p0 = scale | p | nu | Barron's
    alpha, p1 = Barron's scale."""

    kind: int
    p0: float = 0.0
    p1: float = 0.0

    def evaluate(self, s: float) -> np.ndarray:
        """[rho, rho', rho'', sqrt_rho1, residual_scaling, alpha_sq_norm] at the squared norm s (host arithmetic of the
        library: LossFunction::evaluate and Corrector::new)."""
        o = (C.c_double * 6)()
        rc = capi.load().apexgpu_loss_evaluate(int(self.kind), float(self.p0), float(self.p1), float(s), C.byref(o))
        if rc != 0:
            raise capi.LinAlgError(rc, "loss parameters out of range")
        return np.array(o[:])


# create_loss_function of bin/pose_graph_g2o.rs:256-311: name -> (kind, default scale, how the scale becomes (p0, p1))
_LOSS_NAMES = {
    "huber": (capi.LOSS_HUBER, 1.345), "cauchy": (capi.LOSS_CAUCHY, 2.3849), "fair": (capi.LOSS_FAIR, 1.3999),
    "welsch": (capi.LOSS_WELSCH, 2.9846), "tukey": (capi.LOSS_TUKEY, 4.6851),
    "geman": (capi.LOSS_GEMAN_MCCLURE, 1.0), "gemanmcclure": (capi.LOSS_GEMAN_MCCLURE, 1.0),
    "andrews": (capi.LOSS_ANDREWS, 1.339), "ramsay": (capi.LOSS_RAMSAY, 0.3),
    "trimmed": (capi.LOSS_TRIMMED_MEAN, 2.0), "trimmedmean": (capi.LOSS_TRIMMED_MEAN, 2.0),
    "lp": (capi.LOSS_LP_NORM, 1.5),
    "t-distribution": (capi.LOSS_T_DISTRIBUTION, 5.0), "tdistribution": (capi.LOSS_T_DISTRIBUTION, 5.0),
}
_BARRON_ALPHA = {"barron0": 0.0, "barron1": 1.0, "barron-2": -2.0, "adaptive-barron": 0.0, "adaptivebarron": 0.0}


def create_loss_function(name: str, scale: float | None = None) -> Loss:
    """`--loss-function NAME --loss-scale SCALE` of bin/pose_graph_g2o.rs:256-311: the seventeen names, their aliases and
    default scales; case-insensitive.  lp takes the scale as p, t-distribution as nu; l2 and l1 take none."""
    low = name.lower()
    if low == "l2":
        return Loss(capi.LOSS_L2)
    if low == "l1":
        return Loss(capi.LOSS_L1)
    if low in _BARRON_ALPHA:
        loss = Loss(capi.LOSS_BARRON, _BARRON_ALPHA[low], 1.0 if scale is None else float(scale))
    elif low in _LOSS_NAMES:
        kind, default = _LOSS_NAMES[low]
        loss = Loss(kind, default if scale is None else float(scale))
    else:
        raise ValueError(f"Unknown loss function: {name}. Valid options: l2, l1, huber, cauchy, fair, welsch, tukey, geman, "
                         "andrews, ramsay, trimmed, lp, barron0, barron1, barron-2, t-distribution, adaptive-barron")
    loss.evaluate(0.0)   # (the constructor's check of the scale: InvalidInput)
    return loss
