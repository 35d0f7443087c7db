"""Timing of the segment graph of a prior map (yag_slam_amd/splicing.py segment_centroids + segment_edges, ym_segments_*):
ms per ingest of a label image, upload included, for the two cases of DESIGN.md section 4 (1024^2 with about 2000 segments
and 2048^2 with about 9000: a map segmented at the ROS node's density=5).  An ingest is what map_to_graph does before it
casts rays: one upload of the label image, the label range, the per-label sums, the pair table, the divisions and the
`count > 3` filter on the host.  Kernel time alone: run this under `rocprofv3 --kernel-trace --stats`.  --reference also
times the reference's determine_centroids and create_edges on the same label images where the reference is importable
(tests/refstubs.py; minutes on the larger case).  Development aid; bench.py is the judged benchmark.

    python scripts/segments_time.py [--reps 10] [--cases 1024:2000,2048:9000] [--reference]
"""
import argparse
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402


def label_image(n, k, seed=5, room=128):
    """n x n labels: a seeded nearest-seed partition into about k segments, cut by 2-pixel walls of zeros every `room` pixels
    (label 0 = no segment), relabelled 1 .. K without gaps"""
    from yag_slam_amd.synth import seeded_partition
    lab = seeded_partition(n, n, k, seed)
    for j in range(0, n, room):
        lab[j:j + 2, :] = 0
        lab[:, j:j + 2] = 0
    _, inv = np.unique(lab, return_inverse=True)
    return inv.reshape(n, n).astype(np.int32)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--cases", default="1024:2000,2048:9000")
    ap.add_argument("--reference", action="store_true")
    args = ap.parse_args()
    for case in args.cases.split(","):
        n, k = (int(v) for v in case.split(":"))
        lab = label_image(n, k)
        if args.reference:
            sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests", "golden"))
            import make_golden_segments as mg
            splicing = mg.reference_splicing()
            t = time.perf_counter()
            cent = splicing.determine_centroids(lab)
            t1 = time.perf_counter()
            edges = splicing.create_edges(lab)
            t2 = time.perf_counter()
            print("labels %d^2, %d segments: reference determine_centroids %.2f s, create_edges %.2f s (%d edges)"
                  % (n, len(cent), t1 - t, t2 - t1, len(edges)), flush=True)
            continue
        from yag_slam_amd.splicing import SegmentMap, segment_centroids, segment_edges
        cent, edges = segment_centroids(lab), segment_edges(lab)  # warm-up (code object load)
        t = time.perf_counter()
        for _ in range(args.reps):
            segment_centroids(lab)
            segment_edges(lab)
        dt = (time.perf_counter() - t) / args.reps
        # one handle for both, as map_to_graph does, and the parts of it
        parts = np.zeros(4)
        for _ in range(args.reps):
            t0 = time.perf_counter()
            with SegmentMap(lab) as sm:
                t1 = time.perf_counter()
                sm.stats(sm.label_range()[1] + 1)
                t2 = time.perf_counter()
                sm.pairs()
                t3 = time.perf_counter()
            parts += (t1 - t0, t2 - t1, t3 - t2, time.perf_counter() - t0)
        parts *= 1e3 / args.reps
        print("labels %d^2, %d segments, %d edges: segment_centroids + segment_edges %.2f ms; one handle %.2f ms "
              "(upload + range %.2f, stats %.2f, pairs %.2f)" % (n, len(cent), len(edges), dt * 1e3, parts[3], parts[0], parts[1], parts[2]),
              flush=True)


if __name__ == "__main__":
    main()
