"""Timing of the places search (MapLocator.locate_places, ym_locator_locate_places) on the settings of
scripts/locate_time.py: the 2048 x 2048 hall and its 512 x 512 crop, 360 headings, one 1439-beam scan.  Per map, in ONE
process and alternating: `locate(top_k=1)` as the yardstick, and `locate_places` for n_places in 1, 2, 4, 8 with
min_separation (1 m, 0.5 rad) -- wall time of the synchronous call (it ends in a device synchronise), nodes per round, what
the exclusion dropped.  Each case runs once untimed, then --reps rounds over all cases; medians and every sample are written.
These are records, not pass criteria.

--regression merges runs of scripts/locate_time.py on the parent commit and on this one (taken alternately in one session)
into the same file: the unchanged ym_locator_locate must not get slower.

    python scripts/locate_places_time.py [--reps 5] [--out profiles/locate_places_time.json]
    python scripts/locate_places_time.py --regression --parent a.json b.json c.json --change d.json e.json f.json
"""
import argparse
import json
import math
import os
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import numpy as np  # noqa: E402

import locate_time as T  # noqa: E402

PLACES = (1, 2, 4, 8)
SEPARATION = (1.0, 0.5)


def merge_regression(out, parent, change):
    doc = json.load(open(out)) if os.path.exists(out) else {}
    reg = {}
    for name, paths in (("parent", parent), ("change", change)):
        runs = [json.load(open(p)) for p in paths]
        reg[name] = dict(build_ids=sorted(set(r["build_id"] for r in runs)),
                         wall_ms={c["case"]: [run_case["wall_ms"] for r in runs for run_case in r["cases"] if run_case["case"] == c["case"]]
                                  for c in runs[0]["cases"]})
    verdict = {}
    for case, ms in reg["parent"]["wall_ms"].items():
        med = float(np.median(reg["change"]["wall_ms"][case]))
        verdict[case] = dict(parent_min=min(ms), parent_max=max(ms), change_median=med, not_slower=bool(med <= max(ms)),
                             within_parent_spread=bool(min(ms) <= med <= max(ms)))
    reg["verdict"] = verdict
    reg["note"] = ("scripts/locate_time.py (each run: the median of 3 timed locate(top_k=16) calls per case), three runs on the parent "
                   "commit and three on this one, alternating, in one session on one device")
    doc["locate_regression"] = reg
    json.dump(doc, open(out, "w"), indent=1)
    print(json.dumps(reg, indent=1))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "locate_places_time.json"))
    ap.add_argument("--regression", action="store_true")
    ap.add_argument("--parent", nargs="*", default=[])
    ap.add_argument("--change", nargs="*", default=[])
    args = ap.parse_args()
    if args.regression:
        return merge_regression(args.out, args.parent, args.change)
    from yag_slam_amd import _capi, synth
    from yag_slam_amd.models import LocalizedRangeScan
    from yag_slam_amd.scan_matching import ScanMatcher
    scene = T.big_scene(synth)
    image = T.world_image(scene)
    inc = 2 * math.pi / T.N_BEAMS
    ranges = scene.cast(T.TRUTH[0], T.TRUTH[1], T.TRUTH[2], n_beams=T.N_BEAMS, min_angle=-math.pi, inc=inc, max_range=150.0)
    ranges = ranges + np.random.default_rng(5).normal(0.0, 0.01, size=ranges.shape)
    scan = LocalizedRangeScan(ranges, -math.pi, -math.pi + (T.N_BEAMS - 1) * inc, inc, 0.05, 150.0, 150.0, 0.0, 0.0, 0.0)
    m = ScanMatcher(dict(resolution=T.RES, smear_deviation=T.RES), semantics="yagpy")
    rows = []
    for name, side in (("map2048", T.SIDE), ("crop512", 512)):
        if side == T.SIDE:
            im, origin = image, T.ORIGIN
        else:
            cx, cy = int((T.TRUTH[0] - T.ORIGIN[0]) / T.RES), int((T.TRUTH[1] - T.ORIGIN[1]) / T.RES)
            x0, y0 = min(max(cx - side // 2, 0), T.SIDE - side), min(max(cy - side // 2, 0), T.SIDE - side)
            im, origin = np.ascontiguousarray(image[y0:y0 + side, x0:x0 + side]), (T.ORIGIN[0] + x0 * T.RES, T.ORIGIN[1] + y0 * T.RES)
        cmap = m.correlation_grid_from_occupancy(im, occupied_value=0)
        with m.map_locator(cmap) as loc:
            def run(K):
                t = time.perf_counter()
                if K == 0:
                    cands = loc.locate([scan], origin[0], origin[1], n_angles=360, top_k=1)
                else:
                    cands = loc.locate_places([scan], origin[0], origin[1], n_places=K, min_separation=SEPARATION, n_angles=360)
                return (time.perf_counter() - t) * 1e3, cands, loc.last_stats
            ms = {K: [] for K in (0,) + PLACES}
            last = {}
            for rep in range(args.reps + 1):  # (round 0 is the warm-up of every case)
                for K in (0,) + PLACES:
                    dt, cands, st = run(K)
                    last[K] = (cands, st)
                    if rep:
                        ms[K].append(dt)
            base = float(np.median(ms[0]))
            st0 = last[0][1]
            row = dict(map=name, width=side, height=side, headings=360, levels=loc.levels, nq=st0["nq"], separation_m_rad=list(SEPARATION),
                       locate_top1=dict(wall_ms=base, wall_ms_all=[round(v, 3) for v in ms[0]],
                                        nodes_scored=sum(st0["nodes"]) + st0["probe_nodes"]), places=[])
            assert last[0][0][0].index == last[1][0][0].index and [c.index for c in last[8][0]][:4] == [c.index for c in last[4][0]]
            for K in PLACES:
                cands, st = last[K]
                med = float(np.median(ms[K]))
                row["places"].append(dict(n_places=K, found=len(cands), separation_cells=list(loc.last_separation), wall_ms=med,
                                          wall_ms_all=[round(v, 3) for v in ms[K]], over_locate_top1=round(med / base, 3),
                                          rounds=st["rounds"], round_nodes=st["round_nodes"], nodes=st["nodes"], probe_nodes=st["probe_nodes"],
                                          chunks=st["chunks"], excluded_leaves=st["excluded_leaves"], excluded_nodes=st["excluded_nodes"],
                                          scores=[c.score for c in cands], cells=[(c.k, c.cx, c.cy) for c in cands]))
                print("%-8s n_places %d: %d found, %.1f ms (%.2f x locate(top_k=1) at %.1f ms), round nodes %s, excluded %d leaves %d nodes"
                      % (name, K, len(cands), med, med / base, base, st["round_nodes"], st["excluded_leaves"], st["excluded_nodes"]), flush=True)
            rows.append(row)
        cmap.close()
    doc = json.load(open(args.out)) if os.path.exists(args.out) else {}
    doc.update(build_id=_capi.build_id(), device="AMD Instinct MI355X (gfx950), one GPU",
               scene="a 100 m x 100 m hall with 160 seeded boxes of 1 .. 4 m at 0.05 m",
               scan="1439 beams over 360 degrees at %r, sigma 0.01 m" % (T.TRUTH,), reps=args.reps, maps=rows)
    json.dump(doc, open(args.out, "w"), indent=1)


if __name__ == "__main__":
    main()
