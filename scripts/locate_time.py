"""Timing of the map locator (ScanMatcher.map_locator, ym_locator_locate): wall time of one synchronous
`locate`, nodes scored per level, probe nodes and chunks for
  - a 2048 x 2048 map (a 100 m x 100 m hall with 160 boxes at 0.05 m), 360 headings, one 1439-beam scan over 360 degrees
    taken inside it, at the default `levels`;
  - a 512 x 512 crop of that map around the scan, at levels=0 (every hypothesis scored) and at the default.
Each case runs once untimed (code objects, buffers), then --reps times; the median is reported.  The located pose is
compared with the true one.  Kernel time is the sum over the loc_* kernels of a `rocprofv3 --kernel-trace --stats` run of
this script with --case NAME --reps 1 (two calls: the figures are halved), whose kernel_stats.csv is merged in with --kernel-stats NAME=CSV (no device needed).
Writes profiles/locate_time.json.  Development aid; bench.py is the judged benchmark.

    python scripts/locate_time.py [--reps 3] [--case NAME] [--out profiles/locate_time.json]
    python scripts/locate_time.py --kernel-stats map2048=path/to/kernel_stats.csv [...]
"""
import argparse
import csv
import json
import math
import os
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
import numpy as np  # noqa: E402

RES = 0.05
SIDE = 2048
ORIGIN = (-1.2, -1.2)
TRUTH = (37.3, 61.7, 0.9)
N_BEAMS = 1439
CASES = (("map2048", SIDE, None), ("crop512_exhaustive", 512, 0), ("crop512", 512, None))


def world_image(scene):
    im = np.full((SIDE, SIDE), 255, dtype=np.uint8)
    for x0, y0, x1, y1 in scene.segs:
        t = np.linspace(0.0, 1.0, int(math.hypot(x1 - x0, y1 - y0) / (RES / 4)) + 2)
        cx = np.rint((x0 + t * (x1 - x0) - ORIGIN[0]) / RES).astype(int)
        cy = np.rint((y0 + t * (y1 - y0) - ORIGIN[1]) / RES).astype(int)
        im[cy, cx] = 0
    return im


def big_scene(synth):
    """a 100 m x 100 m hall: synth.Scene's walls, and 160 seeded boxes of 1 .. 4 m anywhere but on the sensor"""
    scene = synth.Scene(width=100.0, height=100.0, n_boxes=0)
    rng = np.random.default_rng(77)
    segs = [tuple(s) for s in scene.segs]
    while len(segs) < 4 + 4 * 160:
        w, h = rng.uniform(1.0, 4.0, size=2)
        x0, y0 = rng.uniform(1.0, 99.0 - w), rng.uniform(1.0, 99.0 - h)
        x1, y1 = x0 + w, y0 + h
        if x0 - 1.5 < TRUTH[0] < x1 + 1.5 and y0 - 1.5 < TRUTH[1] < y1 + 1.5:
            continue
        segs += [(x0, y0, x1, y0), (x1, y0, x1, y1), (x1, y1, x0, y1), (x0, y1, x0, y0)]
    scene.segs = np.array(segs, dtype=np.float64)
    return scene


def merge_kernel_stats(out, pairs):
    doc = json.load(open(out))
    for pair in pairs:
        name, path = pair.split("=", 1)
        rows = [r for r in csv.DictReader(open(path)) if "loc_" in r["Name"] or "map_points" in r["Name"]]
        # (the profiled run makes two calls: the untimed one and one repetition)
        per = {r["Name"].split("(")[0].replace("void ", "").replace("ym::", ""): dict(calls=int(r["Calls"]) // 2, ms=round(float(r["TotalDurationNs"]) / 2e6, 3))
               for r in rows}
        for row in doc["cases"]:
            if row["case"] == name:
                row["kernel_ms"] = round(sum(v["ms"] for v in per.values()), 3)
                row["kernels"] = per
    json.dump(doc, open(out, "w"), indent=1)
    print(json.dumps(doc["cases"], indent=1))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--case", default=None)
    ap.add_argument("--kernel-stats", action="append", default=[])
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "locate_time.json"))
    args = ap.parse_args()
    if args.kernel_stats:
        return merge_kernel_stats(args.out, args.kernel_stats)
    from yag_slam_amd import _capi, synth
    from yag_slam_amd.models import LocalizedRangeScan
    from yag_slam_amd.scan_matching import ScanMatcher
    scene = big_scene(synth)
    image = world_image(scene)
    inc = 2 * math.pi / N_BEAMS
    ranges = scene.cast(TRUTH[0], TRUTH[1], TRUTH[2], n_beams=N_BEAMS, min_angle=-math.pi, inc=inc, max_range=150.0)
    ranges = ranges + np.random.default_rng(5).normal(0.0, 0.01, size=ranges.shape)
    scan = LocalizedRangeScan(ranges, -math.pi, -math.pi + (N_BEAMS - 1) * inc, inc, 0.05, 150.0, 150.0, 0.0, 0.0, 0.0)
    m = ScanMatcher(dict(resolution=RES, smear_deviation=RES), semantics="yagpy")
    rows = []
    for name, side, levels in CASES:
        if args.case and args.case != name:
            continue
        if side == SIDE:
            im, origin = image, ORIGIN
        else:  # the crop around the scan
            cx, cy = int((TRUTH[0] - ORIGIN[0]) / RES), int((TRUTH[1] - ORIGIN[1]) / RES)
            x0, y0 = min(max(cx - side // 2, 0), SIDE - side), min(max(cy - side // 2, 0), SIDE - side)
            im, origin = np.ascontiguousarray(image[y0:y0 + side, x0:x0 + side]), (ORIGIN[0] + x0 * RES, ORIGIN[1] + y0 * RES)
        cmap = m.correlation_grid_from_occupancy(im, occupied_value=0)
        with m.map_locator(cmap, levels=levels) as loc:
            ms = []
            for rep in range(args.reps + 1):
                t = time.perf_counter()
                cands = loc.locate([scan], origin[0], origin[1], n_angles=360, top_k=16)
                if rep:
                    ms.append((time.perf_counter() - t) * 1e3)
            st, b = loc.last_stats, cands[0]
            err = (b.pose.x - TRUTH[0], b.pose.y - TRUTH[1], (b.pose.euler[-1] - TRUTH[2] + math.pi) % (2 * math.pi) - math.pi)
            row = dict(case=name, width=side, height=side, headings=360, levels=loc.levels, max_nodes=loc.max_nodes, device_bytes=loc.bytes,
                       nq=st["nq"], hypotheses=side * side * 360, chunks=st["chunks"], nodes=st["nodes"], survivors=st["survivors"],
                       probe_nodes=st["probe_nodes"], nodes_scored=sum(st["nodes"]) + st["probe_nodes"],
                       wall_ms=float(np.median(ms)) if ms else None, wall_ms_all=[round(v, 3) for v in ms],
                       best=dict(score=b.score, response=b.response, k=b.k, cx=b.cx, cy=b.cy), error_m_m_rad=[round(v, 4) for v in err])
            rows.append(row)
            print("%-19s %4d^2 x 360, L=%d, nq=%d: %d chunks, %d of %d hypotheses' worth of nodes (%.3f %%), %.1f ms wall, off the truth by %s"
                  % (name, side, loc.levels, st["nq"], st["chunks"], row["nodes_scored"], row["hypotheses"],
                     100.0 * row["nodes_scored"] / row["hypotheses"], row["wall_ms"] or float("nan"), row["error_m_m_rad"]), flush=True)
        cmap.close()
    if args.case:  # a profiled run of one case: nothing is written
        return
    doc = dict(build_id=_capi.build_id(), device="AMD Instinct MI355X (gfx950), one GPU", scene="a 100 m x 100 m hall with 160 seeded boxes of 1 .. 4 m at 0.05 m",
               scan="1439 beams over 360 degrees at %r, sigma 0.01 m" % (TRUTH,), reps=args.reps, cases=rows)
    json.dump(doc, open(args.out, "w"), indent=1)


if __name__ == "__main__":
    main()
