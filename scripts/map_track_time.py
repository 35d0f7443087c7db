"""Timing of localization mode (ScanMatcher.match_map_batch / track_in_map, ym_match_map_many / ym_map_track; DESIGN.md
section 13) against the per-scan entry it stands for, in the hall of scripts/locate_time.py: a 2048 x 2048 map at 0.05 m,
1081-beam scans.  Wall time of synchronous calls, each case once untimed, then --reps times; the median is reported.
  (a) a loop of N `match_scan_sets_with_map([scan])` calls (ym_match_map, yag_score_kernel): the yardstick;
  (b) one `match_map_batch` of the same N sets, N = 1, 16, 256, 1024;
  (c) `track_in_map` of one track of 2000 scans and of 16 tracks of 125, against the Python loop of (a) with its pose arithmetic.
The scans are taken at 125 poses along a path and reused (every set and every track step has its own resident scan; the
robot of a long track runs the path forth and back).  --case single makes one ym_match_map and one one-item
ym_match_map_many call on the same set: run under `rocprofv3 --kernel-trace --stats`, its kernel_stats.csv gives the per-launch
time of yag_score_kernel and yag_map_kernel, merged in with --kernel-stats CSV (no device needed).
Writes profiles/map_track_time.json.  Development aid; bench.py is the judged benchmark.

    python scripts/map_track_time.py [--reps 3] [--out profiles/map_track_time.json]
    python scripts/map_track_time.py --case single
    python scripts/map_track_time.py --kernel-stats path/to/kernel_stats.csv
"""
import argparse
import csv
import json
import os
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import numpy as np  # noqa: E402

import locate_time as LT  # noqa: E402  (the hall and its image)

N_PATH = 125
BATCHES = (1, 16, 256, 1024)


def path_poses():
    """125 poses 0.1 m apart on a gentle arc through free space around the locator's scan pose"""
    s = np.arange(N_PATH) * 0.1
    th = LT.TRUTH[2] + 0.004 * np.arange(N_PATH)
    x = LT.TRUTH[0] + np.cumsum(np.cos(th) * 0.1) - 0.1 * np.cos(th[0])
    y = LT.TRUTH[1] + np.cumsum(np.sin(th) * 0.1) - 0.1 * np.sin(th[0])
    return np.stack([x, y, th], axis=1), s


def merge_kernel_stats(out, path):
    doc = json.load(open(out))
    per = {}
    for r in csv.DictReader(open(path)):
        name = r["Name"].split("(")[0].replace("void ", "").replace("ym::", "")
        if name.startswith("yag_") or name.startswith("map_points"):
            per[name] = dict(calls=int(r["Calls"]), us_per_launch=round(float(r["TotalDurationNs"]) / 1e3 / int(r["Calls"]), 2))
    doc["single_item_kernels"] = per
    if "yag_map_kernel" in per and "yag_score_kernel" in per:
        doc["score_over_map_kernel"] = round(per["yag_score_kernel"]["us_per_launch"] / per["yag_map_kernel"]["us_per_launch"], 2)
    json.dump(doc, open(out, "w"), indent=1)
    print(json.dumps({k: doc[k] for k in ("single_item_kernels", "score_over_map_kernel") if k in doc}, indent=1))


def median_ms(fn, reps):
    ms = []
    for rep in range(reps + 1):
        t = time.perf_counter()
        fn()
        if rep:
            ms.append((time.perf_counter() - t) * 1e3)
    return float(np.median(ms)), [round(v, 3) for v in ms]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--case", default=None)
    ap.add_argument("--kernel-stats", default=None)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "map_track_time.json"))
    args = ap.parse_args()
    if args.kernel_stats:
        return merge_kernel_stats(args.out, args.kernel_stats)
    from yag_slam_amd import _capi, synth
    from yag_slam_amd.models import native_many
    from yag_slam_amd.scan_matching import ScanMatcher
    from yag_slam_amd.transform import Transform
    scene = LT.big_scene(synth)
    image = LT.world_image(scene)
    truth, _ = path_poses()
    n_distinct = 1 if args.case == "single" else N_PATH
    ranges = [scene.scan_ranges(truth[i], index=3000 + i) for i in range(n_distinct)]
    m = ScanMatcher(dict(resolution=LT.RES, smear_deviation=LT.RES), semantics="yagpy")
    cmap = m.correlation_grid_from_occupancy(image, occupied_value=0)
    ox, oy = LT.ORIGIN
    rng = np.random.default_rng(11)

    def prior_scan(i):  # the scan of path pose i % 125 at a prior a few centimetres and about 0.02 rad off
        p = truth[i % n_distinct] + np.concatenate([rng.normal(0, 0.03, 2), rng.normal(0, 0.02, 1)])
        return synth.resident_scan(ranges[i % n_distinct], p)

    if args.case == "single":  # a profiled run: one launch of each correlate on the same set, nothing is written
        s = [prior_scan(0)]
        a = m.match_scan_sets_with_map(cmap, ox, oy, s, True, True)
        b = m.match_map_batch(cmap, ox, oy, [s], True, True)[0]
        assert a.response == b.response
        print("single item: response", a.response)
        return
    rows = []
    for n in BATCHES:
        sets = [[prior_scan(i)] for i in range(n)]
        native_many([s[0] for s in sets], m.device)
        loop_ms, loop_all = median_ms(lambda: [m.match_scan_sets_with_map(cmap, ox, oy, s, True, True) for s in sets], args.reps)
        batch_ms, batch_all = median_ms(lambda: m.match_map_batch(cmap, ox, oy, sets, True, True), args.reps)
        one = m.match_scan_sets_with_map(cmap, ox, oy, sets[-1], True, True)
        got = m.match_map_batch(cmap, ox, oy, sets, True, True)[-1]
        assert one.response == got.response and one.covariance == got.covariance
        rows.append(dict(case="batch", n=n, loop_ms=loop_ms, loop_ms_all=loop_all, batch_ms=batch_ms, batch_ms_all=batch_all,
                         loop_over_batch=round(loop_ms / batch_ms, 2)))
        print("N = %4d: loop of match_scan_sets_with_map %.2f ms, match_map_batch %.2f ms (x %.2f)" % (n, loop_ms, batch_ms, loop_ms / batch_ms), flush=True)
        del sets

    def make_tracks(n_tracks, length):
        tracks = []
        for _ in range(n_tracks):
            tr = []
            for i in range(length):
                j = i % (2 * N_PATH - 2)
                j = j if j < N_PATH else 2 * N_PATH - 2 - j  # forth and back along the path
                s = synth.resident_scan(ranges[j], truth[j])
                o = truth[j] + np.array([0.02, -0.015, 0.015]) * i  # an odometry that drifts
                s.odom_pose = Transform(float(o[0]), float(o[1]), 0.0, float(o[2]))
                tr.append(s)
            native_many(tr, m.device)
            tracks.append(tr)
        return tracks

    def python_loop(tracks):
        for tr in tracks:
            tr[0].corrected_pose = Transform(tr[0].odom_pose.x, tr[0].odom_pose.y, 0.0, tr[0].odom_pose.euler[-1])
            for i in range(1, len(tr)):
                prior = tr[i - 1].corrected_pose + (tr[i].odom_pose - tr[i - 1].odom_pose)
                tr[i].corrected_pose = prior
                r = m.match_scan_sets_with_map(cmap, ox, oy, [tr[i]], True, True)
                cc = r.meta["corrected_centre"]
                tr[i].corrected_pose = Transform(cc[0], cc[1], 0.0, prior.euler[-1] + cc[2])

    def tracked(tracks):
        for tr in tracks:
            tr[0].corrected_pose = Transform(tr[0].odom_pose.x, tr[0].odom_pose.y, 0.0, tr[0].odom_pose.euler[-1])
        return m.track_in_map(cmap, ox, oy, tracks, 1, True, True)

    for n_tracks, length in ((1, 2000), (16, 125)):
        tracks = make_tracks(n_tracks, length)
        loop_ms, loop_all = median_ms(lambda: python_loop(tracks), args.reps)
        want = [(p.x, p.y, p.euler[-1]) for p in (tr[-1].corrected_pose for tr in tracks)]
        track_ms, track_all = median_ms(lambda: tracked(tracks), args.reps)
        assert want == [(p.x, p.y, p.euler[-1]) for p in (tr[-1].corrected_pose for tr in tracks)]
        rows.append(dict(case="track", tracks=n_tracks, scans_per_track=length, loop_ms=loop_ms, loop_ms_all=loop_all, track_ms=track_ms,
                         track_ms_all=track_all, loop_over_track=round(loop_ms / track_ms, 2)))
        print("%2d track(s) of %4d: Python loop %.1f ms, track_in_map %.1f ms (x %.2f)" % (n_tracks, length, loop_ms, track_ms, loop_ms / track_ms), flush=True)
        del tracks
    c = m.debug_counters()
    doc = dict(build_id=_capi.build_id(), device="AMD Instinct MI355X (gfx950), one GPU", scene="the hall of scripts/locate_time.py: 2048 x 2048 cells at 0.05 m",
               scan="1081 beams over 270 degrees, sigma 0.01 m, 125 poses along a path", reps=args.reps, cases=rows,
               map_kernel_items=c["map_kernel_items"], map_fallback_items=c["map_fallback_items"])
    if os.path.exists(args.out):  # (the kernel figures of an earlier --kernel-stats merge stay until they are merged again)
        old = json.load(open(args.out))
        for k in ("single_item_kernels", "score_over_map_kernel"):
            if k in old:
                doc[k] = old[k]
    json.dump(doc, open(args.out, "w"), indent=1)


if __name__ == "__main__":
    main()
