"""Timing of maps that notice change (CorrelationMap.seen_through, ym_map_seen_through, MapBuilder(forget_seen_through=...);
DESIGN.md section 19) in the setting of scripts/map_forget_time.py: the hall of scripts/locate_time.py, a 2048 x 2048 counted map
at 0.05 m with 5 x 5 taps, 1081-beam scans at poses a few centimetres off the 125 poses of the path of scripts/map_track_time.py.
Wall time of synchronous calls, each case once untimed, then --reps times; the median is reported.
  seen_through  one viewer against 50 and against 2000 held scans, with and without flags
  the step      a `MapBuilder.process_scan` that adds a keyframe to a map of 50 keyframes with the option on, and the same step
                with the option off in the same run -- the yardstick; beside them the step's parts on the same scans: the
                `seen_through` call alone and one `update_scans` that swaps as many scans as the step blanked (at least one).  The
                map is cleared and filled again, untimed, before every repetition.
Writes profiles/map_seen_through_time.json.  Development aid; bench.py is the judged benchmark.

    python scripts/map_seen_through_time.py [--reps 5] [--out profiles/map_seen_through_time.json]
"""
import argparse
import json
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import numpy as np  # noqa: E402

import locate_time as LT  # noqa: E402  (the hall and its image)
import map_track_time as MT  # noqa: E402  (the path)
from map_grow_time import SIDE, median_ms  # noqa: E402

HELD = (50, 2000)
MIN_READINGS = 8


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "map_seen_through_time.json"))
    args = ap.parse_args()
    from yag_slam_amd import _capi, synth
    from yag_slam_amd.mapping import MapBuilder
    from yag_slam_amd.models import native_many
    from yag_slam_amd.scan_matching import ScanMatcher
    from yag_slam_amd.transform import Transform
    scene = LT.big_scene(synth)
    truth, _ = MT.path_poses()
    ranges = [scene.scan_ranges(truth[i], index=3000 + i) for i in range(MT.N_PATH)]
    res = LT.RES
    ox, oy = LT.ORIGIN
    m = ScanMatcher(dict(resolution=res, smear_deviation=0.05), semantics="yagpy")

    def scans_off_the_path(n, seed, first=0):
        off = np.random.default_rng(seed).normal(0.0, [0.03, 0.03, 0.01], (n, 3))
        out = []
        for i in range(n):
            k = (first + i) % MT.N_PATH
            s = synth.resident_scan(ranges[k], truth[k] + off[i])
            s.odom_pose = Transform(s.corrected_pose.x, s.corrected_pose.y, 0.0, s.corrected_pose.euler[-1])
            out.append(s)
        native_many(out, 0)
        return out

    rows = []
    # ---- seen_through alone
    for n in HELD:
        held = scans_off_the_path(n, 1)
        viewer = scans_off_the_path(1, 2, first=60)[0]
        cm = m.empty_correlation_map(SIDE, SIDE, counted=True, ox=ox, oy=oy)
        cm.add_scans(ox, oy, held)
        row = dict(case="seen_through", held=n, viewers=1)
        for flags in (False, True):
            out = []
            ms, ms_all = median_ms(lambda: out.append(cm.seen_through([viewer], flags=flags)), args.reps)
            key = "with_flags" if flags else "counts_only"
            row[key + "_ms"], row[key + "_ms_all"] = ms, ms_all
            row["inside"], row["seen"] = int(out[-1].inside.sum()), int(out[-1].seen.sum())
        rows.append(row)
        print("seen_through of 1 viewer against %4d held: %.3f ms, with flags %.3f ms (%d of %d readings seen through)" % (
            n, row["counts_only_ms"], row["with_flags_ms"], row["seen"], row["inside"]), flush=True)
        cm.close()
    # ---- the builder's step
    n = HELD[0]
    cm = m.empty_correlation_map(SIDE, SIDE, counted=True, ox=ox, oy=oy)
    state = {}

    def fresh_builder(forget):
        def before():
            cm.clear()
            held = scans_off_the_path(n, 1)
            cm.add_scans(ox, oy, held)
            b = MapBuilder(m, cm, ox, oy, forget_seen_through=forget)
            b.added, b.last, b.last_added = list(held), held[-1], held[-1]
            key = scans_off_the_path(1, 3, first=n)[0]
            key.odom_pose = Transform(float(truth[n][0]), float(truth[n][1]), 0.0, float(truth[n][2]))
            state.update(b=b, key=key)
        return before

    def step():
        state["result"] = state["b"].process_scan(state["key"])

    step_rows = {}
    for name, forget in (("option_off", None), ("option_on", MIN_READINGS)):
        ms, ms_all = median_ms(step, args.reps, before=fresh_builder(forget))
        assert state["result"].meta["added"]
        step_rows[name] = dict(ms=ms, ms_all=ms_all, blanked=len(state["b"].blanked))
    # the parts, on the map as the last step with the option on found it (the keyframe added, nothing blanked yet)
    fresh_builder(None)()
    b, key = state["b"], state["key"]
    b.process_scan(key)
    others = b.added[:-1]
    out = []
    seen_ms, seen_all = median_ms(lambda: out.append(cm.seen_through([key], scans=others, flags=True)), args.reps)
    st = out[-1]
    picked = [i for i in range(len(others)) if st.seen[i] >= MIN_READINGS] or [int(np.argmax(st.seen))]
    olds = [others[i] for i in picked]
    copy_ms, _ = median_ms(lambda: native_many([o.blanked(st.flags[i]) for o, i in zip(olds, picked)], 0), args.reps)
    swap = {}

    def swap_before():
        if "news" in swap:
            cm.update_scans(swap["news"], olds)
        swap["news"] = [o.blanked(st.flags[i]) for o, i in zip(olds, picked)]
        native_many(swap["news"], 0)

    upd_ms, upd_all = median_ms(lambda: cm.update_scans(olds, swap["news"]), args.reps, before=swap_before)
    off, on = step_rows["option_off"]["ms"], step_rows["option_on"]["ms"]
    rows.append(dict(case="process_scan_adds_a_keyframe", held=n, min_readings=MIN_READINGS, option_off=step_rows["option_off"],
                     option_on=step_rows["option_on"], ratio_on_to_off=round(on / off, 3),
                     parts=dict(seen_through_with_flags_ms=seen_ms, seen_through_with_flags_ms_all=seen_all,
                                blanked_copies_and_their_twins_ms=copy_ms, update_scans_ms=upd_ms, update_scans_ms_all=upd_all,
                                scans_swapped=len(olds), readings_seen=int(st.seen.sum())),
                     ratio_on_to_off_plus_one_update_scans=round(on / (off + upd_ms), 3)))
    print("process_scan adding a keyframe to %d: %.3f ms without the option, %.3f ms with it (x %.2f; %d scans blanked); parts: "
          "seen_through %.3f ms, copies %.3f ms, update_scans of %d scans %.3f ms" % (
              n, off, on, on / off, step_rows["option_on"]["blanked"], seen_ms, copy_ms, len(olds), upd_ms), flush=True)
    cm.close()
    m.close()
    doc = dict(build_id=_capi.build_id(), device="AMD Instinct MI355X (gfx950), one GPU",
               scene="the hall of scripts/locate_time.py; a counted map of %d x %d cells at %g m, 5 x 5 taps" % (SIDE, SIDE, res),
               scan="1081 beams over 270 degrees, sigma 0.01 m, poses a few centimetres off the 125 of scripts/map_track_time.py",
               command="python scripts/map_seen_through_time.py --reps %d" % args.reps, reps=args.reps, clearance=2, protect=1, cases=rows)
    json.dump(doc, open(args.out, "w"), indent=1)


if __name__ == "__main__":
    main()
