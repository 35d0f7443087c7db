"""Timing of the pose-graph optimiser's held set (PoseGraphOptimizer.hold, ym_graph_hold; DESIGN.md section 9, "Held
nodes"): Levenberg-Marquardt steps, conjugate-gradient iterations and ms of one `compute(100, 1e-4, True, 1e-9, 50)` (the
reference's call), the median of --reps calls on a handle that already holds the graph, each from the same poses, as
scripts/posegraph_time.py measures.

  spliced 43 / spliced 95   tests/posegraph_hold_ref.spliced: a grid(43, 43) (1849 nodes, about the README's map) or
                            grid(95, 95) prior whose edges carry information 1e12, a 2000-node robot chain with the ring's
                            links and 20 links into the grid; with the prior held, with nothing held at the automatic band,
                            with nothing held at band 0.  --yardstick also times the test-side scipy solve of the reduced
                            system on the held case (context: one CPU thread).
  ring 2000 + K held        tests/posegraph_ref.ring(2000) with K = 0, 2000, 20 000 extra nodes appended: a held chain,
                            linked to the ring by one edge.  The time should not grow with K beyond linearising K edges.

--only takes a comma-separated list of case-name prefixes (the unheld spliced cases run for minutes: they hit the iteration
cap); rows of cases that did not run are kept from the file that is there.  Writes profiles/posegraph_hold_time.json.
Development aid; bench.py is the judged benchmark.

    python scripts/posegraph_hold_time.py [--reps 2] [--yardstick] [--only "spliced 43 held,ring"] [--out FILE]
"""
import argparse
import json
import os
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
import numpy as np  # noqa: E402


def ring_with_held_chain(extra):
    """ring(2000) and `extra` more nodes on a line, chained with exact means, the first linked to node 0; returns (graph, held)"""
    from tests import posegraph_ref as ref
    g = ref.ring(2000, noise=0.02, seed=2)
    if not extra:
        return g, []
    n = len(g["poses"])
    line = np.stack([20.0 + 0.1 * np.arange(extra), np.zeros(extra), np.zeros(extra)], axis=1)
    pairs = [(0, n)] + [(n + k, n + k + 1) for k in range(extra - 1)]
    poses = np.concatenate([g["poses"], line])
    means = np.array([ref.relative(poses[a], poses[b]) for a, b in pairs])
    infos = np.tile(100.0 * np.eye(3), (len(pairs), 1, 1))
    g = dict(poses=poses, edges=np.concatenate([g["edges"], np.array(pairs, dtype=np.int32)]).astype(np.int32),
             means=np.concatenate([g["means"], means]), infos=np.concatenate([g["infos"], infos]))
    return g, list(range(n, n + extra))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=2)
    ap.add_argument("--yardstick", action="store_true")
    ap.add_argument("--only", default="")
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "posegraph_hold_time.json"))
    args = ap.parse_args()
    from tests import posegraph_hold_ref as href
    from yag_slam_amd.posegraph import PoseGraphOptimizer

    def spliced(side):
        g = href.spliced(side, side, 2000, seed=side, links=20)
        return g, list(g["prior"])
    cases = []
    for side in (43, 95):
        cases += [("spliced %d held" % side, lambda s=side: spliced(s), True, -1),
                  ("spliced %d free band auto" % side, lambda s=side: spliced(s), False, -1),
                  ("spliced %d free band 0" % side, lambda s=side: spliced(s), False, 0)]
    cases += [("ring 2000 + %d held" % k, lambda k=k: ring_with_held_chain(k), True, -1) for k in (0, 2000, 20000)]
    only = [v.strip() for v in args.only.split(",") if v.strip()]
    rows = {}
    if os.path.exists(args.out):
        with open(args.out) as f:
            rows = {r["case"]: r for r in json.load(f)["rows"]}
    for name, make, hold, band in cases:
        if only and not any(name.startswith(v) for v in only):
            continue
        g, held = make()
        opt = PoseGraphOptimizer()
        for i, p in enumerate(g["poses"]):
            opt.add_node(p[0], p[1], p[2], i)
        for (a, b), z, info in zip(g["edges"], g["means"], g["infos"]):
            opt.add_constraint(int(a), int(b), z[0], z[1], z[2], info)
        if hold:
            opt.hold(held)
        opt.band = band
        opt.chi2()  # (the handle, the uploads, the code object)
        print("%s: %d nodes, %d held, %d constraints ..." % (name, len(g["poses"]), len(opt.held), len(g["edges"])), flush=True)
        ms = []
        for _ in range(args.reps):
            opt.set_poses(g["poses"])
            t = time.perf_counter()
            rep = opt.compute(100, 1.0e-4, True, 1.0e-9, 50)
            ms.append((time.perf_counter() - t) * 1e3)
        row = dict(case=name, nodes=len(g["poses"]), held=int(len(opt.held)), constraints=len(g["edges"]), band=rep.band,
                   lm_steps=rep.lm_steps, accepted=rep.accepted, cg_iterations=rep.cg_iterations, status=rep.status,
                   chi2_initial=rep.chi2_initial, chi2_final=rep.chi2_final, reps=args.reps, ms=float(np.median(ms)),
                   ms_all=[round(v, 3) for v in ms])
        line = "%-26s band %2d: %3d LM steps, %6d CG iterations, chi2 %.6g -> %.6g, %.1f ms" % (
            name, rep.band, rep.lm_steps, rep.cg_iterations, rep.chi2_initial, rep.chi2_final, row["ms"])
        if args.yardstick and hold and name.startswith("spliced"):
            t = time.perf_counter()
            poses, want = href.optimize(g, held)
            row["yardstick_ms"] = (time.perf_counter() - t) * 1e3
            row["yardstick_lm_steps"] = want["lm_steps"]
            d = opt.nodes_xyt - poses
            d[:, 2] = d[:, 2] - 2 * np.pi * np.round(d[:, 2] / (2 * np.pi))
            row["yardstick_pose_difference"] = float(np.abs(d).max())
            line += "; scipy reduced solve %.1f ms, %d LM steps, poses differ by %.2g" % (row["yardstick_ms"], want["lm_steps"],
                                                                                         row["yardstick_pose_difference"])
        print(line, flush=True)
        rows[name] = row
        opt.close()
        with open(args.out, "w") as f:  # (after every case: a later case may run for minutes)
            json.dump(dict(call="compute(100, 1e-4, True, 1e-9, 50)", rows=[rows[c[0]] for c in cases if c[0] in rows]), f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
