"""Timing of the map segmenter (yag_slam_amd/splicing.py SegmentMap.from_map, ym_segments_from_map): ms per segmentation of a
2048^2 and a 1024^2 floor plan (rooms of tests/segmenter_ref.py's `floorplan`, 512 pixels a side, tiled), with the upload
(the whole call) and without it (the call less the time an upload of the same image takes alone, `RayMap` create +
destroy), K, step and the Lloyd passes run, and the kernels' times from one `rocprofv3 --kernel-trace --stats` run per
size (a child process of this script; --no-profile leaves it out).  There is no yardstick: the reference's segment_map
needs scikit-image and OpenCV, which the machines of this project do not have.  For scale, centroids + edges of a 2048^2
label image take 3.6 ms (scripts/segments_time.py).  Writes profiles/segmenter_time.json.  Development aid; bench.py is
the judged benchmark.

    python scripts/segmenter_time.py [--reps 10] [--sizes 2048,1024] [--no-profile] [--out profiles/segmenter_time.json]
"""
import argparse
import csv
import glob
import json
import os
import subprocess
import sys
import tempfile
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
import numpy as np  # noqa: E402


def plan(n, seed=1, room=512):
    """n x n: floor plans of room x room pixels side by side"""
    from tests.segmenter_ref import floorplan
    k = (n + room - 1) // room
    rows = [np.concatenate([floorplan(room, room, seed + i * k + j) for j in range(k)], axis=1) for i in range(k)]
    return np.ascontiguousarray(np.concatenate(rows, axis=0)[:n, :n])


def kernel_times(n, reps):
    """one rocprofv3 run of a child that segments the n x n plan `reps` times -> {kernel: (calls, us per segmentation)}"""
    with tempfile.TemporaryDirectory() as d:
        cmd = ["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", d, "-o", "seg", "--",
               sys.executable, os.path.abspath(__file__), "--child", str(n), "--reps", str(reps)]
        p = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
        if p.returncode != 0:
            raise RuntimeError("rocprofv3 failed: " + p.stderr[-2000:])
        files = glob.glob(os.path.join(d, "**", "*kernel_stats.csv"), recursive=True)
        if not files:
            raise RuntimeError("rocprofv3 wrote no kernel_stats.csv")
        out = {}
        with open(files[0]) as f:
            for row in csv.DictReader(f):
                out[row["Name"]] = dict(calls=int(row["Calls"]), us_per_segmentation=round(int(row["TotalDurationNs"]) / 1e3 / reps, 2))
        return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--sizes", default="2048,1024")
    ap.add_argument("--no-profile", action="store_true")
    ap.add_argument("--child", type=int, default=0)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "segmenter_time.json"))
    args = ap.parse_args()
    from yag_slam_amd.splicing import RayMap, SegmentMap
    if args.child:
        im = plan(args.child)
        for _ in range(args.reps):
            SegmentMap.from_map(im).close()
        return
    rows = []
    for n in (int(v) for v in args.sizes.split(",")):
        im = plan(n)
        with SegmentMap.from_map(im) as sm:  # warm-up (code object load)
            info = sm.info
        RayMap(im).close()
        ms, up = [], []
        for _ in range(args.reps):
            t = time.perf_counter()
            sm = SegmentMap.from_map(im)
            ms.append((time.perf_counter() - t) * 1e3)
            sm.close()
            t = time.perf_counter()
            RayMap(im).close()
            up.append((time.perf_counter() - t) * 1e3)
        row = dict(size=n, segments=info["segments"], n_segments=info["n_segments"], step=info["step"], seeds=info["seeds"],
                   iterations_run=info["iterations_run"], unlabelled_share=info["unlabelled"] / info["n_free"],
                   ms_with_upload=float(np.median(ms)), ms_upload_alone=float(np.median(up)),
                   ms_without_upload=float(np.median(ms) - np.median(up)), ms_all=[round(v, 3) for v in ms])
        if not args.no_profile:
            row["kernels"] = kernel_times(n, args.reps)
            row["kernel_ms_per_segmentation"] = round(sum(k["us_per_segmentation"] for name, k in row["kernels"].items()
                                                          if "seg" in name) / 1e3, 3)
        print("plan %d^2: K %d (n %d, step %d, %d Lloyd passes): %.2f ms with the upload, %.2f ms without%s" % (
            n, row["segments"], row["n_segments"], row["step"], row["iterations_run"], row["ms_with_upload"], row["ms_without_upload"],
            "" if args.no_profile else ", kernels %.2f ms" % row["kernel_ms_per_segmentation"]), flush=True)
        rows.append(row)
    note = ("no yardstick: the reference's segment_map needs scikit-image and OpenCV, absent from this project's machines; for scale, "
            "centroids + edges of a 2048^2 label image take 3.6 ms (scripts/segments_time.py)")
    with open(args.out, "w") as f:
        json.dump(dict(call="SegmentMap.from_map(plan)", reps=args.reps, yardstick=None, note=note, rows=rows), f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
