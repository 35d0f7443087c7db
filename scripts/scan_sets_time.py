"""Timing of `match_scan_sets` on the device (ScanMatcher.match_scan_sets / match_scan_sets_batch, ym_match_sets /
ym_match_sets_many): the reference's default configuration (1 cm cells, 20 m threshold: a 4051 x 4051 grid per
item), 1081-beam scans of the synthetic room, chains of 10 base scans, sets of 1, 2 and 4 query scans, N = 1, 16, 256 and 4096
items.  Wall time of synchronous calls, each case once untimed, then --reps times; the median is reported.  Beside every batch
figure, from the same run:
  (a) a Python loop of N single `match_scan_sets` calls (N = 4096: the loop is run once, not --reps times);
  (b) `match_pairs` on the same matcher with one-scan queries on the same chains: what a set costs over a scan.
The 256-item call of every set size is also run with ym_profile_enable: the device time of its grids (clearing + sets_grid_kernel),
of its integer sums (yag_map_kernel, both passes) and of the whole call.
Writes profiles/scan_sets_time.json.  Development aid; bench.py is the judged benchmark.

    python scripts/scan_sets_time.py [--reps 5] [--items 1,16,256,4096] [--out profiles/scan_sets_time.json]
"""
import argparse
import json
import os
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
import numpy as np  # noqa: E402

CHAIN = 10
SET_SIZES = (1, 2, 4)
N_DISTINCT = 64  # distinct chains and sets; larger calls reuse them (every item still has its own grid and its own sums)


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
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--items", default="1,16,256,4096")
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "scan_sets_time.json"))
    args = ap.parse_args()
    from yag_slam_amd import _capi, synth
    from yag_slam_amd.models import native_many
    from yag_slam_amd.scan_matching import ScanMatcher
    scene = synth.Scene()
    base_poses, q_truth, q_prior = synth.single_match_poses()
    exact = [scene.cast(*p) for p in base_poses[:CHAIN]]
    chains, sets4 = [], []
    for c in range(N_DISTINCT):
        rng = np.random.default_rng(9000 + c)
        chains.append([synth.resident_scan(e + rng.normal(0.0, synth.SIGMA_RANGE, size=e.shape), p) for e, p in zip(exact, base_poses)])
        qs = []
        for i in range(max(SET_SIZES)):
            truth = (q_truth[0] + 0.1 * i, q_truth[1] + 0.01 * i, q_truth[2])
            prior = (q_prior[0] + 0.1 * i + rng.normal(0, 0.01), q_prior[1] + rng.normal(0, 0.01), q_prior[2])
            qs.append(synth.resident_scan(scene.scan_ranges(truth, index=600 + 8 * c + i), prior))
        sets4.append(qs)
    m = ScanMatcher(None, semantics="yagpy")
    native_many([s for ch in chains for s in ch] + [s for qs in sets4 for s in qs], m.device)
    rows, profiled = [], []

    def write():  # (after every case: a run cut short keeps what it measured)
        c = m.debug_counters()
        doc = dict(build_id=_capi.build_id(), config="default (resolution 0.01, range_threshold 20, search_size 0.5)",
                   grid_side=int(0.5 / 0.01 + 1 + 2 * 20 / 0.01), beams=synth.N_BEAMS, chain=CHAIN, reps=args.reps, rows=rows,
                   profiled_256=profiled, sets_kernel_items=c["sets_kernel_items"], sets_fallback_items=c["sets_fallback_items"])
        json.dump(doc, open(args.out, "w"), indent=1)
    for n in [int(v) for v in args.items.split(",")]:
        for k in SET_SIZES:
            sets = [sets4[i % N_DISTINCT][:k] for i in range(n)]
            chs = [chains[i % N_DISTINCT] for i in range(n)]
            batch_ms, batch_all = median_ms(lambda: m.match_scan_sets_batch(sets, chs, True, True), args.reps)
            loop_reps = args.reps if n <= 256 else 1
            loop_ms, loop_all = median_ms(lambda: [m.match_scan_sets(s, c, True, True) for s, c in zip(sets, chs)], loop_reps)
            pairs_ms, pairs_all = median_ms(lambda: m.match_pairs([s[0] for s in sets], chs, True, True), args.reps)
            one = m.match_scan_sets(sets[-1], chs[-1], True, True)
            got = m.match_scan_sets_batch(sets, chs, True, True)[-1]
            assert one.response == got.response and one.covariance == got.covariance
            rows.append(dict(set_size=k, n=n, batch_ms=batch_ms, batch_ms_all=batch_all, loop_ms=loop_ms, loop_ms_all=loop_all,
                             loop_reps=loop_reps, pairs_ms=pairs_ms, pairs_ms_all=pairs_all,
                             loop_over_batch=round(loop_ms / batch_ms, 2), batch_over_pairs=round(batch_ms / pairs_ms, 2)))
            print("set of %d, N = %4d: batch %.2f ms, loop of singles %.2f ms (x %.2f), match_pairs of one-scan queries %.2f ms (x %.2f)"
                  % (k, n, batch_ms, loop_ms, loop_ms / batch_ms, pairs_ms, batch_ms / pairs_ms), flush=True)
            write()
            if n == 256:
                m.profile(True)
                for w in range(3):
                    m.profile_read(w, reset=True)
                m.match_scan_sets_batch(sets, chs, True, True)
                p = {name: dict(zip(("ms", "intervals"), m.profile_read(w, reset=True))) for w, name in ((1, "grids"), (0, "sums"), (2, "call"))}
                m.profile(False)
                profiled.append(dict(set_size=k, n=n, device_ms={a: round(b["ms"], 3) for a, b in p.items()},
                                     intervals={a: int(b["intervals"]) for a, b in p.items()}))
                print("   device time of the 256-item call: grids %.2f ms, sums %.2f ms, whole call %.2f ms"
                      % (p["grids"]["ms"], p["sums"]["ms"], p["call"]["ms"]), flush=True)
    write()
    print("wrote", args.out)


if __name__ == "__main__":
    main()
