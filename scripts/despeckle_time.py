"""Timing of the component area filter (yag_slam_amd/occupancy.py despeckle / create_clean_occupancy_grid; ym_image_despeckle,
ym_occupancy_create_clean).

Images: an occupancy-like 2048^2 and 4096^2 byte image, seeded: the floor plans of tests/segmenter_ref.py's `floorplan` (512
cells a side, tiled; their walls, value 0, are the foreground) plus a sprinkle of blobs of 1 to 4 cells on the cells that
are not walls.  The densities used are recorded.  Reported per image: the median of `reps` synchronous `despeckle` calls,
with the upload (the whole call) and without it (the call less the time an upload of the same image takes alone, `RayMap`
create + destroy); the kernels' times from one `rocprofv3 --kernel-trace --stats` run per size (a child process of this
script; --no-profile leaves it out); and, FOR SCALE ONLY, scipy.ndimage.label + np.bincount of the same image on the host:
there is no yardstick, the node's cv2.connectedComponentsWithStats cannot be installed on this project's machines.
Rendering: create_clean_occupancy_grid against create_occupancy_grid on the same 40 and 400 scans of the synthetic scene,
alternating in one process.  Writes profiles/despeckle_time.json.  Development aid; bench.py is the judged benchmark.

    python scripts/despeckle_time.py [--reps 10] [--sizes 2048,4096] [--no-profile] [--out profiles/despeckle_time.json]
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

BLOB_DENSITY = 0.002  # blobs per cell
BLOBS = ([(0, 0)], [(0, 0), (0, 1)], [(0, 0), (1, 1), (2, 0)], [(0, 0), (0, 1), (1, 0), (1, 1)])  # 1 .. 4 cells each


def image(n, seed=1, room=512):
    """n x n: floor plans of room x room cells side by side, and the sprinkle; -> (image, densities)"""
    from tests.segmenter_ref import floorplan
    k = (n + room - 1) // room
    rows = [np.concatenate([floorplan(room, room, seed + i * k + j) for j in range(k)], axis=1) for i in range(k)]
    im = np.ascontiguousarray(np.concatenate(rows, axis=0)[:n, :n])
    walls = float((im == 0).mean())
    r = np.random.RandomState(seed)
    count = int(BLOB_DENSITY * n * n)
    ys, xs, kinds = r.randint(0, n - 2, count), r.randint(0, n - 2, count), r.randint(0, len(BLOBS), count)
    for kind, blob in enumerate(BLOBS):
        sel = kinds == kind
        for dy, dx in blob:
            im[ys[sel] + dy, xs[sel] + dx] = 0
    return im, dict(wall_density=walls, blobs=count, blobs_per_cell=BLOB_DENSITY, foreground_density=float((im == 0).mean()))


def kernel_times(n, reps):
    """one rocprofv3 run of a child that filters the n x n image `reps` times -> {kernel: (calls, us per call of despeckle)}"""
    with tempfile.TemporaryDirectory() as d:
        cmd = ["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", d, "-o", "dsp", "--",
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
                out[row["Name"]] = dict(calls=int(row["Calls"]), us_per_call=round(int(row["TotalDurationNs"]) / 1e3 / reps, 2))
        return out


def loop_scans(n):
    from yag_slam_amd import synth
    scene = synth.Scene()
    truth, _ = synth.loop_trajectory(n * 12)
    scans = [synth.resident_scan(scene.scan_ranges(p, index=700 + i), p) for i, p in enumerate(truth[::12])]
    for s in scans:
        s.native()
    return scans


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--sizes", default="2048,4096")
    ap.add_argument("--no-profile", action="store_true")
    ap.add_argument("--child", type=int, default=0)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "despeckle_time.json"))
    args = ap.parse_args()
    from yag_slam_amd.occupancy import create_clean_occupancy_grid, create_occupancy_grid, despeckle
    from yag_slam_amd.splicing import RayMap
    if args.child:
        im, _ = image(args.child)
        for _ in range(args.reps):
            despeckle(im)
        return
    rows = []
    for n in (int(v) for v in args.sizes.split(",")):
        im, dens = image(n)
        out, st = despeckle(im, stats=True)  # warm-up (code object load)
        RayMap(im).close()
        ms, up = [], []
        for _ in range(args.reps):
            t = time.perf_counter()
            despeckle(im)
            ms.append((time.perf_counter() - t) * 1e3)
            t = time.perf_counter()
            RayMap(im).close()
            up.append((time.perf_counter() - t) * 1e3)
        from scipy import ndimage
        host = []
        for _ in range(3):
            t = time.perf_counter()
            labels, k = ndimage.label(im == 0, structure=np.ones((3, 3)))
            areas = np.bincount(labels.ravel())
            host.append((time.perf_counter() - t) * 1e3)
        assert k == st["components"] and int((areas[1:] < 5).sum()) == st["removed_components"]
        row = dict(size=n, **dens, stats=st, ms_with_upload=float(np.median(ms)), ms_upload_alone=float(np.median(up)),
                   ms_without_upload=float(np.median(ms) - np.median(up)), ms_all=[round(v, 3) for v in ms],
                   for_scale_only_host_scipy_label_bincount_ms=float(np.median(host)))
        if not args.no_profile:
            row["kernels"] = kernel_times(n, args.reps)
            row["kernel_ms_per_call"] = round(sum(k["us_per_call"] for name, k in row["kernels"].items() if "dsp_" in name) / 1e3, 3)
        print("image %d^2 (foreground %.3f, %d components, %d removed): %.2f ms with the upload, %.2f ms without%s; host scipy, for scale: %.0f ms" % (
            n, dens["foreground_density"], st["components"], st["removed_components"], row["ms_with_upload"], row["ms_without_upload"],
            "" if args.no_profile else ", kernels %.3f ms" % row["kernel_ms_per_call"], row["for_scale_only_host_scipy_label_bincount_ms"]),
            flush=True)
        rows.append(row)
    render = []
    for n in (40, 400):
        scans = loop_scans(n)
        g = create_clean_occupancy_grid(scans, 0.05, 12.0)
        create_occupancy_grid(scans, 0.05, 12.0)
        plain, clean = [], []
        for _ in range(args.reps):
            t = time.perf_counter()
            create_occupancy_grid(scans, 0.05, 12.0)
            plain.append((time.perf_counter() - t) * 1e3)
            t = time.perf_counter()
            create_clean_occupancy_grid(scans, 0.05, 12.0)
            clean.append((time.perf_counter() - t) * 1e3)
        r = dict(scans=n, resolution=0.05, range_threshold=12.0, width=g.width, height=g.height, stats=g.stats,
                 ms_create_occupancy_grid=float(np.median(plain)), ms_create_clean_occupancy_grid=float(np.median(clean)),
                 ms_plain_all=[round(v, 3) for v in plain], ms_clean_all=[round(v, 3) for v in clean])
        print("render %d scans (%d x %d): %.3f ms plain, %.3f ms clean" % (n, g.width, g.height, r["ms_create_occupancy_grid"],
                                                                           r["ms_create_clean_occupancy_grid"]), flush=True)
        render.append(r)
    note = ("no yardstick: the node's cv2.connectedComponentsWithStats cannot be installed on this project's machines; the host "
            "scipy.ndimage.label + np.bincount figure is for scale only")
    with open(args.out, "w") as f:
        json.dump(dict(call="despeckle(image)", reps=args.reps, yardstick=None, note=note, rows=rows, render=render), f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
