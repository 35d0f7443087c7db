"""Timing of the live occupancy grid (yag_slam_amd/occupancy.py LiveOccupancyGrid; ym_occmap_*) against the
full rendering it replaces in a publish.

Workload: the synthetic room, `--scans` (2000) scans of 1081 beams along the seeded loop, resolution 0.05 m, threshold 12 m.
Wall time of synchronous calls, median of `--reps` (3), for every `--held` count H (2000 and 500: the live figures must not grow
with what is held):
  (a) occupancy.ros_map(the first H scans): the full path, every ray traced again -- the yardstick, measured in the same run
  (b) a live grid holding H - 5 scans: add() of the next 5, then ros_map()         -- a publish of the node (every five scans)
  (c) sync() after every pose was nudged (the rebuild route), and after 5 % were (the update route)
  (d) (b) with each form of the trace kernel: 0 a wave per ray, 1 a thread per ray
  (e) the add alone; ros_map() alone; grid() alone (threshold and copy, no filter)  -- what remains of a publish
  (f) add() of all H scans at once with slack_cells 0 and 64: the trace of a large call depends on the memory's pitch
The live grid is anchored at the full rendering's offset, so (a) and (b) must give the same map: the script checks it.
Writes profiles/occupancy_live_time.json.  Development aid; bench.py is the judged benchmark.

    python scripts/occupancy_live_time.py [--scans 2000] [--held 2000,500] [--reps 3] [--out profiles/occupancy_live_time.json]
"""
import argparse
import json
import os
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
import numpy as np  # noqa: E402

RES, RT, STEP = 0.05, 12.0, 5


def loop_scans(n):
    from yag_slam_amd import synth
    from yag_slam_amd.models import native_many
    scene = synth.Scene()
    truth, _ = synth.loop_trajectory(n)
    scans = [synth.resident_scan(scene.scan_ranges(p, index=700 + i), p) for i, p in enumerate(truth)]
    native_many(scans)
    return scans


def timed(fn, reps, before=None):
    """median wall time (ms) of fn(), `before()` run untimed ahead of every repetition -> (median, all)"""
    ms = []
    for _ in range(reps):
        if before is not None:
            before()
        t = time.perf_counter()
        fn()
        ms.append((time.perf_counter() - t) * 1e3)
    return float(np.median(ms)), [round(v, 3) for v in ms]


def measure(scans, held, reps):
    from yag_slam_amd import occupancy
    from yag_slam_amd.models import set_corrected_poses
    scans = scans[:held]
    old, new = scans[:held - STEP], scans[held - STEP:]
    row = dict(held=held, added_per_publish=STEP)
    full = occupancy.ros_map(scans, RES, RT)  # warm-up
    row["width"], row["height"] = full.width, full.height
    row["a_full_ros_map_ms"], row["a_all"] = timed(lambda: occupancy.ros_map(scans, RES, RT), reps)
    for form in (0, 1):
        live = occupancy.LiveOccupancyGrid(RES, RT, anchor=(full.origin.x, full.origin.y))
        live._set_trace_form(form)
        live.add(old)
        live.add(new)
        got = live.ros_map()
        identical = bool(np.array_equal(got.data, full.data) and got.stats == full.stats and (got.origin.x, got.origin.y) == (full.origin.x, full.origin.y))
        if not identical:
            raise RuntimeError("the live grid's map differs from the full rendering's (form %d, %d held)" % (form, held))
        key = "wave_per_ray" if form == 0 else "thread_per_ray"

        def publish():
            live.add(new)
            live.ros_map()

        row["bd_publish_%s_ms" % key], row["bd_publish_%s_all" % key] = timed(publish, reps, before=lambda: live.remove(new))
        row["e_add_%s_ms" % key], row["e_add_%s_all" % key] = timed(lambda: live.add(new), reps, before=lambda: live.remove(new))
        if form == 0:
            row["identical_to_full"] = identical
            row["e_ros_map_alone_ms"], _ = timed(live.ros_map, reps)
            row["e_grid_alone_ms"], row["e_grid_alone_all"] = timed(live.grid, reps)
            row["e_remove_ms"], _ = timed(lambda: live.remove(new), reps, before=lambda: new[0] in live or live.add(new))
            if new[0] not in live:
                live.add(new)
            info = live.info
            row["alloc"] = [info["alloc_width"], info["alloc_height"]]
            row["reallocations"] = info["reallocations"]
            # (c) the optimiser's moves
            base = np.array([(s.corrected_pose.x, s.corrected_pose.y, s.corrected_pose.euler[-1]) for s in scans])
            flip = [1.0]

            def nudge(count):
                def go():
                    flip[0] = -flip[0]
                    set_corrected_poses(scans[:count], base[:count] + flip[0] * np.array([0.01, -0.01, 0.002]))
                return go

            routes = []
            row["c_sync_all_nudged_ms"], row["c_all_nudged_all"] = timed(lambda: routes.append(live.sync(scans)), reps, before=nudge(held))
            assert set(routes) == {"rebuild"}, routes
            del routes[:]
            few = max(1, held // 20)
            row["c_sync_5pct_nudged_ms"], _ = timed(lambda: routes.append(live.sync(scans)), reps, before=nudge(few))
            assert set(routes) == {"update"}, routes
            row["c_5pct_scans"] = few
            set_corrected_poses(scans, base)
        live.close()
    # (f) the whole set traced in one call, by the slack: the memory's pitch is the window's width plus twice the slack
    row["f_add_all_by_slack"] = {}
    for slack in (0, 64):
        live = occupancy.LiveOccupancyGrid(RES, RT, anchor=(full.origin.x, full.origin.y), slack_cells=slack)
        live.add(scans)
        ms, every = timed(lambda: live.add(scans), reps, before=lambda: live.remove(scans))
        row["f_add_all_by_slack"][str(slack)] = dict(ms=ms, all=every, pitch=live.info["alloc_width"])
        live.close()
    row["b_live_publish_ms"] = row["bd_publish_wave_per_ray_ms"]
    row["speedup_b_over_a"] = round(row["a_full_ros_map_ms"] / row["b_live_publish_ms"], 2)
    print("%4d held (%d x %d): full ros_map %.2f ms; live publish (add %d + ros_map) %.2f ms wave-per-ray, %.2f ms thread-per-ray; "
          "add alone %.3f / %.3f ms; ros_map alone %.2f ms, grid alone %.2f ms; sync all nudged %.2f ms, 5 %% nudged %.2f ms; "
          "add of all at once %s" % (
              held, row["width"], row["height"], row["a_full_ros_map_ms"], STEP, row["bd_publish_wave_per_ray_ms"],
              row["bd_publish_thread_per_ray_ms"], row["e_add_wave_per_ray_ms"], row["e_add_thread_per_ray_ms"], row["e_ros_map_alone_ms"],
              row["e_grid_alone_ms"], row["c_sync_all_nudged_ms"], row["c_sync_5pct_nudged_ms"],
              ", ".join("%.2f ms at pitch %d" % (v["ms"], v["pitch"]) for v in row["f_add_all_by_slack"].values())), flush=True)
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scans", type=int, default=2000)
    ap.add_argument("--held", default="2000,500")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "occupancy_live_time.json"))
    args = ap.parse_args()
    from yag_slam_amd import _capi
    if _capi.lib().ym_device_count() < 1:
        raise SystemExit("occupancy_live_time.py needs a HIP device")
    scans = loop_scans(args.scans)
    rows = [measure(scans, int(h), args.reps) for h in args.held.split(",")]
    note = ("wall time of synchronous calls, median of reps, one device; (a) is the parent's path measured in the same run; "
            "the live grid is anchored at (a)'s offset and its map is checked to be (a)'s")
    with open(args.out, "w") as f:
        json.dump(dict(workload="synth loop, %d scans x 1081 beams, %.2f m, %.0f m" % (args.scans, RES, RT), reps=args.reps,
                       build_id=_capi.build_id(), note=note, rows=rows), f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
