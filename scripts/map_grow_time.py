"""Timing of maps that take scans (CorrelationMap.add_scans / clear, MapBuilder; ym_map_add_scans) in the
hall of scripts/locate_time.py: 2048 x 2048 maps, 1081-beam scans taken at 125 poses along the path of scripts/map_track_time.py.
Wall time of synchronous calls, each case once untimed, then --reps times; the median is reported.
  (a) `add_scans` of 1 and of 64 scans at both tap sizes that matter -- 5 x 5 (resolution 0.05, smear 0.05: the hall's own map)
      and 29 x 29 (0.01 / 0.07: a 20 m x 20 m map around the path) -- into a cleared map (the clear is not timed) and again into
      the map that already holds them (no cell rises: the plain loads alone);
  (b) `MapBuilder.rebuild()` of 2000 scans (the 125 of the path, each 16 times), at both tap sizes;
  (c) a `MapBuilder.process_scan` step along the path, from an empty map, keyframes every 0.2 m;
yardsticks, in the same run:
  (d) `correlation_grid_from_occupancy` of the hall's 2048 x 2048 image, its upload included;
  (e) a `MapLocalizer.process_scan` step along the same path on that map.
Writes profiles/map_grow_time.json.  Development aid; bench.py is the judged benchmark.

    python scripts/map_grow_time.py [--reps 5] [--out profiles/map_grow_time.json]
"""
import argparse
import json
import os
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import numpy as np  # noqa: E402

import locate_time as LT  # noqa: E402  (the hall and its image)
import map_track_time as MT  # noqa: E402  (the path)

SIDE = 2048
TAPS = (("5x5", 0.05, 0.05), ("29x29", 0.01, 0.07))


def median_ms(fn, reps, before=None):
    ms = []
    for rep in range(reps + 1):
        if before:
            before()
        t = time.perf_counter()
        fn()
        if rep:
            ms.append((time.perf_counter() - t) * 1e3)
    return round(float(np.median(ms)), 4), [round(v, 4) for v in ms]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "map_grow_time.json"))
    args = ap.parse_args()
    from yag_slam_amd import _capi, synth
    from yag_slam_amd.mapping import MapBuilder, MapLocalizer
    from yag_slam_amd.models import native_many
    from yag_slam_amd.scan_matching import ScanMatcher
    from yag_slam_amd.transform import Transform
    scene = LT.big_scene(synth)
    truth, _ = MT.path_poses()
    ranges = [scene.scan_ranges(truth[i], index=3000 + i) for i in range(MT.N_PATH)]

    def scans_at_truth(n):
        out = [synth.resident_scan(ranges[i % MT.N_PATH], truth[i % MT.N_PATH]) for i in range(n)]
        native_many(out, 0)
        return out

    rows = []
    for name, res, smear in TAPS:
        m = ScanMatcher(dict(resolution=res, smear_deviation=smear), semantics="yagpy")
        # the hall's own origin at 0.05; at 0.01 the 20.48 m map is centred on the middle of the path
        ox, oy = LT.ORIGIN if res == LT.RES else (float(truth[62][0]) - 0.5 * SIDE * res, float(truth[62][1]) - 0.5 * SIDE * res)
        cm = m.empty_correlation_map(SIDE, SIDE)
        for n in (1, 64):
            scans = scans_at_truth(n)
            fresh_ms, fresh_all = median_ms(lambda: cm.add_scans(ox, oy, scans), args.reps, before=cm.clear)
            st = cm.add_scans(ox, oy, scans)
            again_ms, again_all = median_ms(lambda: cm.add_scans(ox, oy, scans), args.reps)
            rows.append(dict(case="add_scans", taps=name, resolution=res, smear_deviation=smear, scans=n, points=st.points, stamped=st.stamped,
                             dropped=st.dropped, into_cleared_map_ms=fresh_ms, into_cleared_map_ms_all=fresh_all,
                             into_same_map_ms=again_ms, into_same_map_ms_all=again_all))
            print("%-5s add_scans of %2d scans (%d readings, %d stamped): %.3f ms into a cleared map, %.3f ms again" % (
                name, n, st.points, st.stamped, fresh_ms, again_ms), flush=True)
        clear_ms, clear_all = median_ms(cm.clear, args.reps)
        b = MapBuilder(m, cm, ox, oy)
        b.added = scans_at_truth(2000)
        re_ms, re_all = median_ms(b.rebuild, args.reps)
        st = b.rebuild()
        rows.append(dict(case="rebuild", taps=name, resolution=res, scans=2000, points=st.points, stamped=st.stamped, dropped=st.dropped,
                         rebuild_ms=re_ms, rebuild_ms_all=re_all, clear_ms=clear_ms, clear_ms_all=clear_all))
        print("%-5s clear %.3f ms, rebuild of 2000 scans (%d readings, %d stamped) %.2f ms" % (name, clear_ms, st.points, st.stamped, re_ms), flush=True)
        del b
        cm.close()
        m.close()

    # ---- the steps: MapBuilder from an empty map, and the yardsticks on the hall's map built from its image
    m = ScanMatcher(dict(resolution=LT.RES, smear_deviation=LT.RES), semantics="yagpy")
    ox, oy = LT.ORIGIN
    image = LT.world_image(scene)
    occ_ms, occ_all = median_ms(lambda: m.correlation_grid_from_occupancy(image, occupied_value=0).close(), args.reps)
    rows.append(dict(case="correlation_grid_from_occupancy", side=SIDE, ms=occ_ms, ms_all=occ_all))
    print("correlation_grid_from_occupancy of the %d x %d image, upload included: %.2f ms" % (SIDE, SIDE, occ_ms), flush=True)

    def track():
        out = []
        for i in range(MT.N_PATH):
            s = synth.resident_scan(ranges[i], truth[0])
            o = truth[i] + np.array([0.002, -0.0015, 0.0015]) * i  # an odometry that drifts
            s.odom_pose = Transform(float(o[0]), float(o[1]), 0.0, float(o[2]))
            out.append(s)
        native_many(out, 0)
        return out

    def steps_ms(driver, scans):
        driver.start(scans[0])
        ms = []
        for s in scans[1:]:
            t = time.perf_counter()
            driver.process_scan(s)
            ms.append((time.perf_counter() - t) * 1e3)
        return ms

    prior = m.correlation_grid_from_occupancy(image, occupied_value=0)
    loc = MapLocalizer(m, prior, ox, oy)
    loc_ms = steps_ms(loc, track())
    grown = m.empty_correlation_map(SIDE, SIDE)
    b = MapBuilder(m, grown, ox, oy, min_distance=0.2, min_rotation=0.1)
    scans = track()
    b_ms = steps_ms(b, scans)
    added_steps = [r.meta["added"] for r in b.results]
    err = float(np.hypot(scans[-1].corrected_pose.x - truth[-1][0], scans[-1].corrected_pose.y - truth[-1][1]))
    rows.append(dict(case="steps", scans=MT.N_PATH, map_localizer_step_ms=round(float(np.median(loc_ms)), 4),
                     map_builder_step_ms=round(float(np.median(b_ms)), 4),
                     map_builder_step_with_add_ms=round(float(np.median([v for v, a in zip(b_ms, added_steps) if a])), 4),
                     map_builder_step_without_add_ms=round(float(np.median([v for v, a in zip(b_ms, added_steps) if not a])), 4),
                     added=len(b.added), lost_at_end=b.lost, localizer_lost_at_end=loc.lost, map_builder_final_error_m=round(err, 4)))
    print("step: MapLocalizer %.3f ms, MapBuilder %.3f ms (%d of %d scans added)" % (
        rows[-1]["map_localizer_step_ms"], rows[-1]["map_builder_step_ms"], len(b.added), MT.N_PATH), flush=True)
    doc = dict(build_id=_capi.build_id(), device="AMD Instinct MI355X (gfx950), one GPU",
               scene="the hall of scripts/locate_time.py; maps of %d x %d cells" % (SIDE, SIDE),
               scan="1081 beams over 270 degrees, sigma 0.01 m, 125 poses along the path of scripts/map_track_time.py",
               command="python scripts/map_grow_time.py --reps %d" % args.reps, reps=args.reps, cases=rows)
    json.dump(doc, open(args.out, "w"), indent=1)


if __name__ == "__main__":
    main()
