"""Timing of maps whose window moves (CorrelationMap.reframe, ym_map_reframe) in the setting of
scripts/map_forget_time.py: the hall of scripts/locate_time.py, 2048 x 2048 maps, 1081-beam scans at poses a few centimetres off
the 125 poses of the path of scripts/map_track_time.py, both tap sizes (5 x 5 at resolution 0.05, 29 x 29 at 0.01).  Wall time of
synchronous calls, each case once untimed, then --reps times; the median is reported.  Every case has its yardstick in the same run:
  counted maps    `reframe` beside `empty_correlation_map(..., window=)` plus `add_scans` of all held scans, which is what a caller
                  without it would do (and gives the same map: asserted);
  uncounted maps  `reframe` beside `to_numpy()`, the shifted or padded copy on the host and `upload_correlation_grid`.
Cases: a scroll by 64 columns with 50 and with 2000 scans held, and a grow from 1024 x 1024 to 2048 x 2048 (2000 held); the map is
moved back, untimed, before every repetition.  The reframe's statistics are kept: `restamped` and `recomputed` say what it had to do
beyond the copy, and the restamp reads every held scan whatever the shift.
Writes profiles/map_reframe_time.json.  Development aid; bench.py is the judged benchmark.

    python scripts/map_reframe_time.py [--reps 5] [--out profiles/map_reframe_time.json]
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
from map_grow_time import SIDE, TAPS, median_ms  # noqa: E402

SCROLL = 64
SMALL = SIDE // 2
HELD = (50, 2000)


def shifted(a, dx, dy, width, height):
    """new[j, i] = a[j + dy, i + dx] where that exists, zero elsewhere (np.pad when the window only grows)"""
    h, w = a.shape
    out = np.zeros((height, width), dtype=a.dtype)
    x0, x1, y0, y1 = max(0, -dx), min(width, w - dx), max(0, -dy), min(height, h - dy)
    out[y0:y1, x0:x1] = a[y0 + dy:y1 + dy, x0 + dx:x1 + dx]
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "map_reframe_time.json"))
    args = ap.parse_args()
    from yag_slam_amd import _capi, synth
    from yag_slam_amd.models import native_many
    from yag_slam_amd.scan_matching import ScanMatcher
    scene = LT.big_scene(synth)
    truth, _ = MT.path_poses()
    ranges = [scene.scan_ranges(truth[i], index=3000 + i) for i in range(MT.N_PATH)]

    def scans_off_the_path(n, seed):
        off = np.random.default_rng(seed).normal(0.0, [0.03, 0.03, 0.01], (n, 3))
        out = [synth.resident_scan(ranges[i % MT.N_PATH], truth[i % MT.N_PATH] + off[i]) for i in range(n)]
        native_many(out, 0)
        return out

    rows = []
    for name, res, smear in TAPS:
        m = ScanMatcher(dict(resolution=res, smear_deviation=smear), semantics="yagpy")
        ax, ay = LT.ORIGIN if res == LT.RES else (float(truth[62][0]) - 0.5 * SIDE * res, float(truth[62][1]) - 0.5 * SIDE * res)

        def yardstick_counted(window, held):
            def run():
                fresh = m.empty_correlation_map(window[2], window[3], counted=True, ox=ax, oy=ay, window=window[:2])
                fresh.add_scans(fresh.origin[0], fresh.origin[1], held)
                run.last = fresh
            return run

        def counted_case(case, start, move, held):
            """`move` = (dx, dy, width, height) from the window `start`, timed; back again untimed"""
            cm = m.empty_correlation_map(start[2], start[3], counted=True, ox=ax, oy=ay, window=start[:2])
            cm.add_scans(cm.origin[0], cm.origin[1], held)
            new = (start[0] + move[0], start[1] + move[1], move[2], move[3])
            stats = []

            def home():
                if cm.window != start:
                    cm.reframe(-move[0], -move[1], start[2], start[3])

            r_ms, r_all = median_ms(lambda: stats.append(cm.reframe(*move)), args.reps, before=home)
            yard = yardstick_counted(new, held)

            def drop():
                if getattr(yard, "last", None) is not None:
                    yard.last.close()
                    yard.last = None

            y_ms, y_all = median_ms(yard, args.reps, before=drop)
            assert np.array_equal(cm.to_numpy(), yard.last.to_numpy()) and np.array_equal(cm.stamps(), yard.last.stamps())
            drop()
            st = stats[-1]
            rows.append(dict(case=case, map="counted", taps=name, resolution=res, held=len(held), window=list(start), move=list(move),
                             kept=st.kept, restamped=st.restamped, dropped=st.dropped, recomputed=st.recomputed,
                             reframe_ms=r_ms, reframe_ms_all=r_all, create_plus_add_all_ms=y_ms, create_plus_add_all_ms_all=y_all))
            print("%-5s counted %-6s with %4d held: reframe %.3f ms (restamped %d, recomputed %d); create + add of all %.3f ms" % (
                name, case, len(held), r_ms, st.restamped, st.recomputed, y_ms), flush=True)
            cm.close()

        def uncounted_case(case, start, move, held):
            cm = m.empty_correlation_map(start[2], start[3])
            cm.add_scans(ax + start[0] * res, ay + start[1] * res, held)
            first = cm.to_numpy()

            def home():
                if cm.shape != first.shape or cm.window[:2] != (0, 0):
                    cm.reframe(-move[0], -move[1], start[2], start[3])

            r_ms, r_all = median_ms(lambda: cm.reframe(*move), args.reps, before=home)
            home()  # (a map without counts loses what left the window: the yardstick starts from what the map holds now)
            base = cm.to_numpy()
            cm.reframe(*move)
            got = cm.to_numpy()
            src = m.upload_correlation_grid(base)
            keep = []

            def round_trip():
                keep.append(m.upload_correlation_grid(shifted(src.to_numpy(), *move)))

            def drop():
                while keep:
                    keep.pop().close()

            y_ms, y_all = median_ms(round_trip, args.reps, before=drop)
            assert np.array_equal(got, keep[-1].to_numpy())
            drop()
            rows.append(dict(case=case, map="uncounted", taps=name, resolution=res, window=list(start), move=list(move),
                             reframe_ms=r_ms, reframe_ms_all=r_all, read_pad_upload_ms=y_ms, read_pad_upload_ms_all=y_all))
            print("%-5s uncounted %-6s: reframe %.3f ms; to_numpy + copy + upload %.3f ms" % (name, case, r_ms, y_ms), flush=True)
            src.close()
            cm.close()

        def parts(held):
            """where a scroll's time goes: memory (a map created, and created and destroyed), a scroll of a counted map that holds
            nothing (copy, flags, recompute, no restamp), and the pass over the held scans alone (`add_scans` into a cleared map)"""
            made = []

            def drop():
                while made:
                    made.pop().close()

            create_ms, _ = median_ms(lambda: made.append(m.empty_correlation_map(SIDE, SIDE, counted=True, ox=ax, oy=ay)), args.reps, before=drop)
            drop()
            both_ms, _ = median_ms(lambda: m.empty_correlation_map(SIDE, SIDE, counted=True, ox=ax, oy=ay).close(), args.reps)
            cm = m.empty_correlation_map(SIDE, SIDE, counted=True, ox=ax, oy=ay)
            empty_ms, _ = median_ms(lambda: cm.reframe(SCROLL, 0), args.reps, before=lambda: cm.window[0] and cm.reframe(-SCROLL, 0))
            row = dict(case="parts", taps=name, resolution=res, create_counted_ms=create_ms, create_and_destroy_counted_ms=both_ms,
                       scroll_of_an_empty_counted_map_ms=empty_ms)
            for n in HELD:
                add_ms, _ = median_ms(lambda: cm.add_scans(cm.origin[0], cm.origin[1], held[:n]), args.reps, before=cm.clear)
                row["add_scans_of_%d_into_a_cleared_map_ms" % n] = add_ms
            cm.close()
            rows.append(row)
            print("%-5s parts: create %.3f ms, create + destroy %.3f ms, scroll of an empty counted map %.3f ms, add of %s: %s ms" % (
                name, create_ms, both_ms, empty_ms, HELD, [row["add_scans_of_%d_into_a_cleared_map_ms" % n] for n in HELD]), flush=True)

        full, small = (0, 0, SIDE, SIDE), (SMALL // 2, SMALL // 2, SMALL, SMALL)
        grow = (-(SMALL // 2), -(SMALL // 2), SIDE, SIDE)
        for n in HELD:
            counted_case("scroll", full, (SCROLL, 0, SIDE, SIDE), scans_off_the_path(n, 1))
        held = scans_off_the_path(HELD[-1], 1)
        counted_case("grow", small, grow, held)
        uncounted_case("scroll", full, (SCROLL, 0, SIDE, SIDE), held)
        uncounted_case("grow", small, grow, held)
        parts(held)
        m.close()
    doc = dict(build_id=_capi.build_id(), device="AMD Instinct MI355X (gfx950), one GPU",
               scene="the hall of scripts/locate_time.py; maps of %d x %d cells" % (SIDE, SIDE),
               scan="1081 beams over 270 degrees, sigma 0.01 m, poses a few centimetres off the 125 of scripts/map_track_time.py",
               command="python scripts/map_reframe_time.py --reps %d" % args.reps, reps=args.reps, cases=rows)
    json.dump(doc, open(args.out, "w"), indent=1)


if __name__ == "__main__":
    main()
