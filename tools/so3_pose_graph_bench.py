"""SO3 pose-graph (rotation averaging) measurement: make_rotation_graph at 2,500 and 10,000 vertices and two mean degrees --
chain-like (4) and view-graph-like (30, chords within a window of 200 vertices: what a capture sequence's view graph looks
like, and what keeps the tile structure banded) -- and beside each vertex count the SE2 make_manhattan graph of the same size
from the same process.  Per workload: set-up seconds, ms per LM iteration, the six stage times, tile rows / tiles / fill /
levels from apexgpu_pg_info.  Writes profiles/so3_pose_graph_bench.txt.  Records what was measured; gates nothing.

Method as tools/pose_graph2d_bench.py: an iteration is the wall time of one whole apexgpu_pg_lm_optimize call (it ends in a
device synchronise) divided by its iteration count, the figure is the median over five calls of 12 iterations from the same
start after a warm-up call, and the spread (min .. max of the five) is printed beside it.  Stage times come from a further call
with stage timing on (mean ms per call of each stage); timing serialises the stream, so they sum to more than the iteration.

Hypothesis the output confirms or refutes: at equal n_v and tile structure the factorisation time of an SO3 graph equals that of
an SE2 graph -- both run the same 48-vertex tiles -- and only assemble and cost differ.  To decide it every SO3 workload is
followed by an SE2 graph over the SAME vertex count and edge list (se2_twin: random SE2 poses, consistent measurements with
noise), so the two handles build the same tile plan; the report prints the two `factor` stages and their ratio side by side.

The VGPR line is what --vgprs is given: the tool has no compiler at hand where it runs.  Take it from the build's resource-usage
remarks (hipcc -Rpass-analysis=kernel-resource-usage on csrc/pg_kernels.hip, the k_pg2_assemble entries) of the SAME tree.

    python tools/so3_pose_graph_bench.py [--out profiles/so3_pose_graph_bench.txt] [--vgprs "<from the build>"]
"""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import apex_solver_amd as pkg                                                                   # noqa: E402
from apex_solver_amd.pose_graph import GpuSparseCholeskySolver, PoseGraphProblem               # noqa: E402
from apex_solver_amd.solver import LevenbergMarquardtConfig, LinearSolverType                  # noqa: E402

WINDOW = 200


def se2_twin(d, seed=1):
    """an SE2 graph over the vertex count and edge list of d: random poses in a 30 x 30 square, measurements = the true relative
    poses times Exp(N(0, 0.02^2)), a start 0.05 off the truth -- the structure is d's, so the tile plan is d's"""
    rng = np.random.default_rng(seed)
    truth = np.column_stack([rng.uniform(-15, 15, (d.n_v, 2)), rng.uniform(-np.pi, np.pi, d.n_v)])
    S = pkg.synthetic
    rel = S.se2_mul(S.se2_inv(truth[d.e_from]), truth[d.e_to])
    meas = S.se2_mul(rel, S.se2_exp(0.02 * rng.standard_normal((d.n_e, 3))))
    start = truth + 0.05 * rng.standard_normal(truth.shape)
    return S.PoseGraphData(ids=d.ids.copy(), poses=start, e_from=d.e_from.copy(), e_to=d.e_to.copy(), meas=meas, truth=truth, name="se2-twin")


def one(name, data, iters=12):
    prob = PoseGraphProblem.pose_graph(data)
    t0 = time.perf_counter()
    s = GpuSparseCholeskySolver(0).initialize_structure(prob)
    s.set_parameters(data.poses)
    setup = time.perf_counter() - t0
    cfg = (LevenbergMarquardtConfig.new().with_linear_solver_type(LinearSolverType.SparseCholesky).with_max_iterations(iters)
           .with_cost_tolerance(0.0).with_parameter_tolerance(0.0).with_gradient_tolerance(0.0))
    s.lm_optimize(cfg)                                       # warm-up (graph capture, first-use allocations)
    per_iter = []
    for _ in range(5):
        s.set_parameters(data.poses)
        t0 = time.perf_counter()
        res, hist, _ = s.lm_optimize(cfg)
        per_iter.append(1e3 * (time.perf_counter() - t0) / max(res.iterations, 1))
    accepted = int(hist[:, 3].sum())
    s.set_parameters(data.poses)
    s.enable_stage_timing(True); s.reset_stage_times()
    res, hist, _ = s.lm_optimize(cfg)
    st = s.stage_times()
    info = s.info()
    s.close()
    stages = {k: (ms / max(n, 1)) for k, (ms, n) in st.items()}
    return dict(name=name, n_v=data.n_v, n_e=data.n_e, setup_s=setup, ms_per_iter=float(np.median(per_iter)), lo=min(per_iter), hi=max(per_iter),
                iterations=res.iterations, accepted=accepted, stages=stages, info=info, final_cost=res.final_cost, initial_cost=res.initial_cost)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "so3_pose_graph_bench.txt"))
    ap.add_argument("--vgprs", default="not given", help="VGPRs of k_pg2_assemble per loss policy, from the compiler's resource-usage remarks")
    a = ap.parse_args()
    rows, pairs = [], []
    for n in (2500, 10000):
        for degree in (4, 30):
            d = pkg.synthetic.make_rotation_graph(n, degree, 0.05, 1, window=WINDOW)
            rows.append(one(f"SO3 make_rotation_graph({n}, {degree}, 0.05, 1, window={WINDOW})", d))
            rows.append(one(f"SE2 twin of it (same vertices and edge list)", se2_twin(d)))
            pairs.append((rows[-2], rows[-1]))
        rows.append(one(f"SE2 make_manhattan({n})", pkg.synthetic.make_manhattan(n)))
    lines = ["SO3 pose graphs (rotation averaging) on one MI355X: tools/so3_pose_graph_bench.py",
             "(ms per LM iteration: median [min .. max] of 5 runs of 12 iterations, wall time / iterations, after a warm-up run;",
             " stage times: mean ms per call inside one timed run -- timing serialises the stream, so the stages sum to more than the iteration)",
             f"k_pg2_assemble VGPRs (LossLegacy / LossGeneral / LossWeighted), 0 bytes of scratch each: {a.vgprs}", ""]
    for r in rows:
        i = r["info"]
        fill = i["tiles"] - i["touched_tiles"]
        lines.append(f"{r['name']}: {r['n_v']} vertices, {r['n_e']} edges, set-up {r['setup_s']:.3f} s, {r['ms_per_iter']:.3f} ms / LM iteration "
                     f"[{r['lo']:.3f} .. {r['hi']:.3f}] ({r['iterations']} iterations, {r['accepted']} accepted, cost {r['initial_cost']:.4g} -> {r['final_cost']:.4g})")
        lines.append(f"    tile rows {i['tile_rows']}, tiles {i['tiles']} (of H itself {i['touched_tiles']}, fill {fill}), levels {i['etree_levels']}, dof {i['total_dof']}")
        lines.append("    stages (ms / call): " + ", ".join(f"{k} {v:.3f}" for k, v in r["stages"].items()))
    lines += ["", "Hypothesis: equal n_v and tile structure => equal factorisation time (SO3 | its SE2 twin, `factor` ms per call):"]
    for a_, b_ in pairs:
        same = all(a_["info"][k] == b_["info"][k] for k in ("tile_rows", "tiles", "touched_tiles", "etree_levels"))
        fa, fb = a_["stages"]["factor"], b_["stages"]["factor"]
        lines.append(f"    {a_['n_v']} vertices, {a_['n_e']} edges, tiles {a_['info']['tiles']} | {b_['info']['tiles']} (same plan: {same}): "
                     f"factor {fa:.3f} | {fb:.3f} ms, ratio {fa / fb:.3f}; assemble {a_['stages']['assemble']:.3f} | {b_['stages']['assemble']:.3f}, "
                     f"cost {a_['stages']['cost']:.3f} | {b_['stages']['cost']:.3f}")
    txt = "\n".join(lines) + "\n"
    print(txt)
    with open(a.out, "w") as f:
        f.write(txt)


if __name__ == "__main__":
    main()
