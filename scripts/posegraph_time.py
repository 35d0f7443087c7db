"""Timing of the pose-graph optimiser (yag_slam_amd/posegraph.py, ym_graph_optimize): Levenberg-Marquardt steps, conjugate
gradient iterations and ms of one `compute(100, 1e-4, True, 1e-9, 50)` (the reference's call) on the graphs of DESIGN.md
("Pose-graph optimiser"): the 2000-node and the 10 000-node ring of tests/posegraph_ref.py (chain, skip-3 and two closing
edges, noise 0.02) and a 95 x 95 grid graph with 4-neighbour edges (the shape splicing.map_to_graphslam produces) at the
automatic band and at band 0.  Every repetition starts from the same poses on a handle that already holds the graph, so the
time is the optimisation alone: uploads of what changed, the launches and one small read-back a step.  --yardstick also
times the test-side scipy sparse-direct solver on the same graphs (context, not a competitor: one CPU thread).
Writes profiles/posegraph_time.json.  Development aid; bench.py is the judged benchmark.

    python scripts/posegraph_time.py [--reps 3] [--yardstick] [--out profiles/posegraph_time.json]
"""
import argparse
import json
import os
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
import numpy as np  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--yardstick", action="store_true")
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "posegraph_time.json"))
    args = ap.parse_args()
    from tests import posegraph_ref as ref
    from yag_slam_amd.posegraph import PoseGraphOptimizer
    cases = [("ring 2000", lambda: ref.ring(2000, noise=0.02, seed=2), -1), ("ring 10000", lambda: ref.ring(10000, noise=0.02, seed=2), -1),
             ("grid 95x95", lambda: ref.grid(95, 95, noise=0.02, seed=3), -1), ("grid 95x95", lambda: ref.grid(95, 95, noise=0.02, seed=3), 0)]
    rows = []
    for name, make, band in cases:
        g = make()
        opt = PoseGraphOptimizer()
        for i, p in enumerate(g["poses"]):
            opt.add_node(p[0], p[1], p[2], i)
        for (a, b), z, info in zip(g["edges"], g["means"], g["infos"]):
            opt.add_constraint(int(a), int(b), z[0], z[1], z[2], info)
        opt.band = band
        opt.chi2()  # (the handle, the uploads, the code object)
        ms = []
        for _ in range(args.reps):
            opt.set_poses(g["poses"])
            t = time.perf_counter()
            rep = opt.compute(100, 1.0e-4, True, 1.0e-9, 50)
            ms.append((time.perf_counter() - t) * 1e3)
        row = dict(graph=name, nodes=len(g["poses"]), constraints=len(g["edges"]), band=rep.band, lm_steps=rep.lm_steps,
                   accepted=rep.accepted, cg_iterations=rep.cg_iterations, status=rep.status, chi2_initial=rep.chi2_initial,
                   chi2_final=rep.chi2_final, ms=float(np.median(ms)), ms_all=[round(v, 3) for v in ms])
        line = "%-11s band %2d: %5d nodes, %5d constraints, %3d LM steps, %6d CG iterations, chi2 %.6g -> %.6g, %.1f ms" % (
            name, rep.band, row["nodes"], row["constraints"], rep.lm_steps, rep.cg_iterations, rep.chi2_initial, rep.chi2_final, row["ms"])
        if args.yardstick and band == -1:
            t = time.perf_counter()
            poses, want = ref.optimize(g)
            row["yardstick_ms"] = (time.perf_counter() - t) * 1e3
            row["yardstick_lm_steps"] = want["lm_steps"]
            d = opt.nodes_xyt - poses
            d[:, 2] = ref.wrap(d[:, 2])
            row["yardstick_pose_difference"] = float(np.abs(d).max())
            line += "; scipy sparse direct %.1f ms, %d LM steps, poses differ by %.2g" % (row["yardstick_ms"], want["lm_steps"],
                                                                                         row["yardstick_pose_difference"])
        print(line, flush=True)
        rows.append(row)
        opt.close()
    with open(args.out, "w") as f:
        json.dump(dict(call="compute(100, 1e-4, True, 1e-9, 50)", reps=args.reps, rows=rows), f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
