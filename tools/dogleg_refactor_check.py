"""What two builds of the library must agree on when the Dog-Leg step moves (profiles/dogleg_backend_refactor.txt): run once per
build (APEXGPU_LIB selects it, as tools/ab_libs.sh does) and compare the outputs.

    steps         one fresh and one reused apexgpu_dogleg_step on a BA, an SE3 and an SE2 handle, Jacobi scaling on -- the run to
                  put under `rocprofv3 --kernel-trace`: the kernel name sequences of the two builds are compared
    bits PREFIX   the Dog-Leg loops of tools/ba_trust_region_bench.py and tools/trust_region_bench.py on their smallest shapes
                  (ladybug-1723; make_sphere(50, 50), make_manhattan(3500)), with and without Jacobi scaling: the history rows and
                  the final parameters as raw bytes in PREFIX.<handle>.<scaling>, the history alone beside it as .hist.npy, one
                  sha256 line per run on stdout

    python tools/dogleg_refactor_check.py steps | bits PREFIX
"""
import hashlib
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import apex_solver_amd as pkg                                                                                   # noqa: E402
from apex_solver_amd.pose_graph import DogLegConfig, GpuSparseCholeskySolver, PoseGraphProblem                    # noqa: E402
from apex_solver_amd.solver import GpuSchurComplementSolver, OptimizationType, Problem                            # noqa: E402

ZERO = dict(cost_tolerance=0.0, parameter_tolerance=0.0, gradient_tolerance=0.0)


def handles(small):
    d = pkg.synthetic.make_problem(40, 1500, 3, 7, config_id=1) if small else pkg.synthetic.make_named("ladybug-1723")
    s = GpuSchurComplementSolver(0).initialize_structure(Problem.bundle_adjustment(d, OptimizationType.SelfCalibration))
    yield "ba", s, (d.poses, d.intr, d.points)
    for name, g in (("se3", pkg.synthetic.make_sphere(10, 12) if small else pkg.synthetic.make_sphere(50, 50)),
                    ("se2", pkg.synthetic.make_manhattan(200) if small else pkg.synthetic.make_manhattan(3500))):
        s = GpuSparseCholeskySolver(0).initialize_structure(PoseGraphProblem(g).add_prior(f"x{int(g.ids[0])}"))
        yield name, s, (g.poses,)


def steps():
    for name, s, start in handles(small=True):
        s.set_parameters(*start)
        s.apply_column_scaling(1.0 / (1.0 + s.compute_column_norms()))
        fresh = s.dogleg_step(1e-4, 1e4)
        s.eval_step(); s.discard_step()
        reused = s.dogleg_step(1e-4, 0.25 * fresh["scaled_step_norm"], reuse=True)
        s.eval_step(); s.commit_step()
        print(name, fresh["step_type"], reused["step_type"], reused["reused"])
        s.close()


def bits(out):
    for name, s, start in handles(small=False):
        for scaling in (False, True):
            s.set_parameters(*start)
            res, hist, _ = s.dogleg_optimize(DogLegConfig(max_iterations=10, use_jacobi_scaling=scaling, **ZERO))
            final = s.get_parameters()
            blob = np.ascontiguousarray(hist).tobytes() + b"".join(np.ascontiguousarray(p).tobytes() for p in (final if isinstance(final, tuple) else (final,)))
            with open(f"{out}.{name}.{int(scaling)}", "wb") as f:   # one file per run: `cmp` them build against build
                f.write(blob)
            np.save(f"{out}.{name}.{int(scaling)}.hist.npy", hist)
            print(f"{name} scaling {int(scaling)}: {res.iterations} iterations, status {res.status}, {int(hist[:, 11].sum())} reused, "
                  f"final cost {float(res.final_cost).hex()}, history + parameters sha256 {hashlib.sha256(blob).hexdigest()[:16]}")
        s.close()


if __name__ == "__main__":
    steps() if sys.argv[1] == "steps" else bits(sys.argv[2])
