#!/usr/bin/env python3
"""The reference's own `GraphSlam` driving this package's scan and pose classes (the scenario of
tests/test_reference_integration.py), recorded so that the test needs no copy of the reference.

Run where the reference is importable (tests/refstubs.py: its location and the stand-ins for what this image lacks):

    python tests/golden/make_golden_graphslam.py

Outputs (data files):
  tests/golden/graphslam_run.bin   the bytes `GraphSlam.binarize()` wrote at the end of the run
  tests/golden/graphslam_run.json  the calls that reached the two matchers, the scans that closed a loop, the optimiser's
                                   node and compute counts, the graph's edges and running scans, the numbers the run gave
                                   the scans, their corrected poses after the run and the class they were rebuilt as, and
                                   what the reference's own reader (`GraphSlam.unbinarize`) read back from the bytes
"""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
sys.dont_write_bytecode = True
sys.path.insert(0, REPO)

from tests import refstubs  # noqa: E402
from tests.test_reference_integration import N_SCANS, StandInMatcher, _scans  # noqa: E402


def main():
    if not refstubs.available():
        raise SystemExit("the reference is not importable here (tests/refstubs.py)")
    refstubs.install()
    from yag_slam.graph_slam import GraphSlam  # the reference
    truth, scans = _scans(N_SCANS)
    seq, loop = StandInMatcher(truth), StandInMatcher(truth, loop=True)
    slam = GraphSlam(seq, loop, scan_buffer_len=5, loop_search_dist=1.0, loop_search_min_chain_size=3)
    closed = []
    for s in scans:
        res, c = slam.process_scan(s)
        if c:
            closed.append(s.num)
    blob = slam.binarize()
    back = GraphSlam.unbinarize(blob)
    pose = lambda p: [float(p.x), float(p.y), float(p.euler[-1])]
    rec = {
        "n_scans": N_SCANS,
        "seq_calls": [[q, list(b), p, f] for q, b, p, f in seq.calls],
        "loop_calls": [[q, list(b), p, f] for q, b, p, f in loop.calls],
        "closed": closed,
        "opt_nodes": len(slam.opt.nodes),
        "opt_computes": slam.opt.computes,
        "edges": len(slam.graph.edges),
        "running_scans": [s.num for s in slam.running_scans],
        "nums": [s.num for s in scans],
        "corrected_poses": [pose(s.corrected_pose) for s in scans],
        "corrected_pose_classes": sorted({type(s.corrected_pose).__module__ + "." + type(s.corrected_pose).__name__ for s in scans}),
        "unbinarized": {"vertices": len(back.graph.vertices), "edges": len(back.graph.edges),
                        "ranges": [[float(r) for r in v.obj.ranges] for v in back.graph.vertices],
                        "corrected_poses": [pose(v.obj.corrected_pose) for v in back.graph.vertices]},
    }
    with open(os.path.join(HERE, "graphslam_run.bin"), "wb") as f:
        f.write(blob)
    with open(os.path.join(HERE, "graphslam_run.json"), "w") as f:
        json.dump(rec, f, separators=(",", ":"))
        f.write("\n")
    print("graphslam_run: %d scans, %d closures, %d bytes" % (N_SCANS, len(closed), len(blob)))


if __name__ == "__main__":
    main()
