"""Timing of maps that forget (CorrelationMap.remove_scans / sync, the windowed MapBuilder; ym_map_update_scans; DESIGN.md section
16) in the setting of scripts/map_grow_time.py: the hall of scripts/locate_time.py, 2048 x 2048 maps, 1081-beam scans taken at 125
poses along the path of scripts/map_track_time.py, both tap sizes (5 x 5 at resolution 0.05, 29 x 29 at 0.01).  Wall time of
synchronous calls (every call ends in a wait for the device), each case once untimed, then --reps times; the median is reported.
Everything is measured in this one run:
  (a) `add_scans` of 1 and of 64 scans into a cleared map, counted beside uncounted, alternating: what the counts cost or save;
  (b) `remove_scans` of 1 and of 64 scans out of a map that holds them alone and out of one that holds 2000 (they are put back,
      untimed, before every repetition);
  (c) `sync` with 5, 50, 500 and 2000 of 2000 held scans moved by a few centimetres -- `sync()` over all held scans, which
      compares 2000 poses on the host, and `sync(moved)` for a caller who knows what moved --, beside `clear` plus `add_scans` of
      all 2000 on a map without counts, which is what `MapBuilder.rebuild()` did before and still does above REBUILD_SHARE
      (the 2000 scans of (b) and (c) stand a few centimetres off the path's 125 poses, each its own way);
  (d) a `MapBuilder.process_scan` step along the path with window=8, beside one without a window.
Writes profiles/map_forget_time.json.  Development aid; bench.py is the judged benchmark.

    python scripts/map_forget_time.py [--reps 5] [--out profiles/map_forget_time.json]
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
from map_grow_time import SIDE, TAPS, median_ms  # noqa: E402

WINDOW = 8
MOVED = (5, 50, 500, 2000)
HELD = 2000


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "map_forget_time.json"))
    args = ap.parse_args()
    from yag_slam_amd import _capi, synth
    from yag_slam_amd.mapping import MapBuilder
    from yag_slam_amd.models import native_many
    from yag_slam_amd.scan_matching import ScanMatcher
    from yag_slam_amd.transform import Transform
    scene = LT.big_scene(synth)
    truth, _ = MT.path_poses()
    ranges = [scene.scan_ranges(truth[i], index=3000 + i) for i in range(MT.N_PATH)]

    def scans_at_truth(n, jitter=None):
        """the path's scans, each pose used again every 125; jitter: a seed for poses a few centimetres off the path, so that the
        copies of a pose do not stamp the same cells"""
        off = np.zeros((n, 3)) if jitter is None else np.random.default_rng(jitter).normal(0.0, [0.03, 0.03, 0.01], (n, 3))
        out = [synth.resident_scan(ranges[i % MT.N_PATH], truth[i % MT.N_PATH] + off[i]) for i in range(n)]
        native_many(out, 0)
        return out

    rows = []
    for name, res, smear in TAPS:
        m = ScanMatcher(dict(resolution=res, smear_deviation=smear), semantics="yagpy")
        ox, oy = LT.ORIGIN if res == LT.RES else (float(truth[62][0]) - 0.5 * SIDE * res, float(truth[62][1]) - 0.5 * SIDE * res)
        counted = m.empty_correlation_map(SIDE, SIDE, counted=True, ox=ox, oy=oy)
        plain = m.empty_correlation_map(SIDE, SIDE)
        # ---- (a) add_scans, counted beside uncounted
        for n in (1, 64):
            scans = scans_at_truth(n)
            c_ms, c_all = median_ms(lambda: counted.add_scans(ox, oy, scans), args.reps, before=counted.clear)
            p_ms, p_all = median_ms(lambda: plain.add_scans(ox, oy, scans), args.reps, before=plain.clear)
            c2_ms, c2_all = median_ms(lambda: counted.add_scans(ox, oy, scans), args.reps, before=counted.clear)  # (again: the spread)
            st = plain.add_scans(ox, oy, scans)
            assert np.array_equal(counted.to_numpy(), plain.to_numpy())
            rows.append(dict(case="add_scans", taps=name, resolution=res, scans=n, points=st.points, stamped=st.stamped,
                             counted_ms=c_ms, counted_ms_all=c_all, uncounted_ms=p_ms, uncounted_ms_all=p_all,
                             counted_again_ms=c2_ms, counted_again_ms_all=c2_all))
            print("%-5s add_scans of %2d scans into a cleared map: counted %.3f ms (again %.3f), uncounted %.3f ms" % (
                name, n, c_ms, c2_ms, p_ms), flush=True)
        # ---- (b) remove_scans out of a map that holds the scans alone, and out of one that holds 2000
        held = scans_at_truth(HELD, jitter=1)
        for background in (0, HELD):
            counted.clear()
            if background:
                counted.add_scans(ox, oy, held)
            for n in (1, 64):
                scans = scans_at_truth(n, jitter=2)

                def put_back():
                    if scans[0] not in counted:
                        counted.add_scans(ox, oy, scans)

                stats = []
                r_ms, r_all = median_ms(lambda: stats.append(counted.remove_scans(scans)), args.reps, before=put_back)
                st = stats[-1]
                rows.append(dict(case="remove_scans", taps=name, resolution=res, scans=n, map_holds_other_scans=background,
                                 removed=st.removed, released=st.released, box=[st.x0, st.y0, st.x1, st.y1], ms=r_ms, ms_all=r_all))
                print("%-5s remove_scans of %2d scans out of a map holding %4d others: %.3f ms (%d readings, %d cells released)" % (
                    name, n, background, r_ms, st.removed, st.released), flush=True)
        # ---- (c) sync of k moved scans beside clear + add_scans of all, the rebuild of a map without counts
        counted.clear()
        counted.add_scans(ox, oy, held)

        def full():
            plain.clear()
            plain.add_scans(ox, oy, held)

        full_ms, full_all = median_ms(full, args.reps)
        rng = np.random.default_rng(7)
        for k in MOVED:
            picks = [held[i] for i in sorted(rng.permutation(HELD)[:k])]
            home = [s.corrected_pose for s in picks]
            flip = [0]

            def move():  # a few centimetres and a few milliradians off the pose of the add, another way every time
                flip[0] += 1
                for s, p in zip(picks, home):
                    d = 0.01 * (1 + flip[0] % 3)
                    s.corrected_pose = Transform(p.x + d, p.y - 0.6 * d, 0.0, p.euler[-1] + 0.1 * d)

            stats = []
            all_ms, all_all = median_ms(lambda: stats.append(counted.sync()), args.reps, before=move)
            st = stats[-1]
            some_ms, some_all = median_ms(lambda: counted.sync(picks), args.reps, before=move)
            t = time.perf_counter()
            for _ in range(20):
                counted.moved_scans()
            host_ms = (time.perf_counter() - t) * 1e3 / 20
            again_ms, again_all = median_ms(full, args.reps)
            rows.append(dict(case="sync", taps=name, resolution=res, held=HELD, moved=k, removed=st.removed, added=st.added,
                             released=st.released, gained=st.gained, box=[st.x0, st.y0, st.x1, st.y1],
                             sync_all_held_ms=all_ms, sync_all_held_ms_all=all_all, sync_moved_list_ms=some_ms, sync_moved_list_ms_all=some_all,
                             host_pose_compare_of_2000_ms=round(host_ms, 4), clear_plus_add_all_ms=again_ms, clear_plus_add_all_ms_all=again_all))
            print("%-5s sync of %4d of %d moved: %.3f ms over all held (%.3f ms of it comparing poses), %.3f ms given the list; "
                  "clear + add of all %d: %.3f ms" % (name, k, HELD, all_ms, host_ms, some_ms, HELD, again_ms), flush=True)
        rows.append(dict(case="clear_plus_add_all", taps=name, resolution=res, scans=HELD, ms=full_ms, ms_all=full_all))
        # the two routes end in the same map
        full()
        assert np.array_equal(counted.to_numpy(), plain.to_numpy())
        counted.close()
        plain.close()
        m.close()

    # ---- (d) the steps: MapBuilder along the path from an empty map, with and without a window
    m = ScanMatcher(dict(resolution=LT.RES, smear_deviation=LT.RES), semantics="yagpy")
    ox, oy = LT.ORIGIN

    def track():
        out = []
        for i in range(MT.N_PATH):
            s = synth.resident_scan(ranges[i], truth[0])
            o = truth[i] + np.array([0.002, -0.0015, 0.0015]) * i  # an odometry that drifts
            s.odom_pose = Transform(float(o[0]), float(o[1]), 0.0, float(o[2]))
            out.append(s)
        native_many(out, 0)
        return out

    def steps(window):
        cm = m.empty_correlation_map(SIDE, SIDE, counted=True, ox=ox, oy=oy) if window else m.empty_correlation_map(SIDE, SIDE)
        b = MapBuilder(m, cm, ox, oy, min_distance=0.2, min_rotation=0.1, window=window)
        scans = track()
        b.start(scans[0])
        ms = []
        for s in scans[1:]:
            t = time.perf_counter()
            b.process_scan(s)
            ms.append((time.perf_counter() - t) * 1e3)
        added = [r.meta["added"] for r in b.results]
        err = float(np.hypot(scans[-1].corrected_pose.x - truth[-1][0], scans[-1].corrected_pose.y - truth[-1][1]))
        out = dict(step_ms=round(float(np.median(ms)), 4),
                   step_with_add_ms=round(float(np.median([v for v, a in zip(ms, added) if a])), 4),
                   step_without_add_ms=round(float(np.median([v for v, a in zip(ms, added) if not a])), 4),
                   keyframes=len(b.added) + len(b.dropped), in_map_at_end=len(b.added), lost_at_end=b.lost, final_error_m=round(err, 4))
        cm.close()
        return out

    steps(None)  # (untimed: first launches)
    plain_steps, window_steps, plain_again = steps(None), steps(WINDOW), steps(None)
    rows.append(dict(case="steps", scans=MT.N_PATH, window=WINDOW, unwindowed=plain_steps, windowed=window_steps, unwindowed_again=plain_again))
    print("MapBuilder step with an add: %.3f ms unwindowed (again %.3f), %.3f ms with window=%d" % (
        plain_steps["step_with_add_ms"], plain_again["step_with_add_ms"], window_steps["step_with_add_ms"], WINDOW), flush=True)
    doc = dict(build_id=_capi.build_id(), device="AMD Instinct MI355X (gfx950), one GPU",
               scene="the hall of scripts/locate_time.py; maps of %d x %d cells" % (SIDE, SIDE),
               scan="1081 beams over 270 degrees, sigma 0.01 m, 125 poses along the path of scripts/map_track_time.py",
               command="python scripts/map_forget_time.py --reps %d" % args.reps, reps=args.reps, cases=rows)
    json.dump(doc, open(args.out, "w"), indent=1)


if __name__ == "__main__":
    main()
