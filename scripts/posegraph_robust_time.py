"""What robust kernels cost the pose-graph optimiser: one `compute(100, 1e-4, True, 1e-9, 50)` (the
reference's call) on the 2000-ring of scripts/posegraph_time.py (tests/posegraph_ref.py: chain, skip-3 and two closing edges,
noise 0.02, seed 2) with 100 seeded long-range closures, three ways in the same process:

    plain            every constraint the plain square (the yardstick of this script)
    cauchy           every closure cauchy(5), no outlier among them
    cauchy, 1 % off  the same with 1 % of the closures replaced by constraints to a wrong place

Every repetition starts from the same poses on a handle that already holds the graph, so the time is the optimisation alone.
A run with other weights takes other steps, so the ratio to the plain run compares whole optimisations, not kernels: the
columns ms_per_step and ms_per_cg put the two side by side.  Writes profiles/posegraph_robust_time.json.  Development aid;
bench.py is the judged benchmark.

    python scripts/posegraph_robust_time.py [--reps 3] [--out profiles/posegraph_robust_time.json]
"""
import argparse
import json
import os
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
import numpy as np  # noqa: E402

EXTRA, C = 100, 5.0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "posegraph_robust_time.json"))
    args = ap.parse_args()
    from tests import posegraph_ref as ref
    from tests import posegraph_robust_ref as rr
    from yag_slam_amd.posegraph import PoseGraphOptimizer
    base = ref.ring(2000, noise=0.02, seed=2, extra=EXTRA)
    off, closures, wrong = rr.with_wrong_closures(base, EXTRA, 0.01, seed=0)
    cases = [("plain", base, None), ("cauchy", base, ("cauchy", C)), ("cauchy, 1 % off", off, ("cauchy", C))]
    rows = []
    for name, g, robust in cases:
        opt = PoseGraphOptimizer()
        for i, p in enumerate(g["poses"]):
            opt.add_node(p[0], p[1], p[2], i)
        for (a, b), z, info in zip(g["edges"], g["means"], g["infos"]):
            opt.add_constraint(int(a), int(b), z[0], z[1], z[2], info)
        if robust is not None:
            opt.set_robust(closures, robust)
        opt.cost()  # (the handle, the uploads, the code object)
        ms = []
        for _ in range(args.reps):
            opt.set_poses(g["poses"])
            t = time.perf_counter()
            rep = opt.compute(100, 1.0e-4, True, 1.0e-9, 50)
            ms.append((time.perf_counter() - t) * 1e3)
        _, w = opt.edge_terms()
        row = dict(case=name, nodes=len(g["poses"]), constraints=len(g["edges"]), closures=EXTRA, wrong=0 if g is base else len(wrong),
                   band=rep.band, lm_steps=rep.lm_steps, accepted=rep.accepted, cg_iterations=rep.cg_iterations, status=rep.status,
                   cost_initial=rep.chi2_initial, cost_final=rep.chi2_final, pose_error=rr.pose_error(opt.nodes_xyt, g["truth"]),
                   least_closure_weight=float(w[closures].min()), ms=float(np.median(ms)), ms_all=[round(v, 3) for v in ms])
        row["ms_per_step"] = row["ms"] / max(rep.lm_steps, 1)
        row["ms_per_cg"] = row["ms"] / max(rep.cg_iterations, 1)
        row["ratio_to_plain"] = row["ms"] / rows[0]["ms"] if rows else 1.0
        print("%-16s band %2d: %3d LM steps, %5d CG iterations, F %.6g -> %.6g, error against truth %.3g, least closure weight %.3g, "
              "%.1f ms (%.2f a step, %.3f an iteration), %.3f of plain"
              % (name, rep.band, rep.lm_steps, rep.cg_iterations, rep.chi2_initial, rep.chi2_final, row["pose_error"],
                 row["least_closure_weight"], row["ms"], row["ms_per_step"], row["ms_per_cg"], row["ratio_to_plain"]), flush=True)
        rows.append(row)
        opt.close()
    with open(args.out, "w") as f:
        json.dump(dict(call="compute(100, 1e-4, True, 1e-9, 50)", graph="ring(2000, noise=0.02, seed=2, extra=100)", kernel="cauchy(5) on the closures",
                       reps=args.reps, rows=rows), f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
