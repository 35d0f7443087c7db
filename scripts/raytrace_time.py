"""Timing of the virtual-scan ray casting (yag_slam_amd/splicing.py, ym_raymap_trace): ms per trace and pixel steps per
second on synthetic floor plans, for the two cases of DESIGN.md (a 2048^2 map with 1024 viewpoints and an 8192^2 map with
4096 viewpoints, 1439 rays each: map_to_graph's sweep).  A trace is one synchronous call: upload of the viewpoints and the
direction table, the kernel, download of the end points and lengths (16 bytes per ray).  Kernel time alone: run this
under `rocprofv3 --kernel-trace --stats`.  Development aid; bench.py is the judged benchmark.

    python scripts/raytrace_time.py [--reps 10] [--cases 2048:1024,8192:4096]
"""
import argparse
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402


def floor_plan(n, seed=5, room=128, door=24):
    """n x n pixels: rooms of `room` pixels walled by 2-pixel walls (0) with doors, unknown (205) outside a margin,
    seeded clutter (0) and a speckle of the threshold values"""
    rng = np.random.default_rng(seed)
    im = np.full((n, n), 254, dtype=np.uint8)
    for k in range(0, n, room):
        im[k:k + 2, :] = 0
        im[:, k:k + 2] = 0
    for k in range(0, n, room):
        for j in range(room // 2, n, room):
            im[k:k + 2, j - door // 2:j + door // 2] = 254
            im[j - door // 2:j + door // 2, k:k + 2] = 254
    m = n // 16
    im[:m, :] = 205
    im[:, :m] = 205
    for _ in range(n // 4):
        x, y = rng.integers(0, n - 8, 2)
        im[y:y + rng.integers(2, 8), x:x + rng.integers(2, 8)] = 0
    speck = rng.random((n, n)) < 0.0005
    im[speck] = rng.choice(np.array([179, 180, 181, 209, 210, 211], dtype=np.uint8), size=int(speck.sum()))
    return im


def viewpoints(im, k, seed=6):
    rng = np.random.default_rng(seed)
    free = np.argwhere(im == 254)
    pick = free[rng.choice(free.shape[0], k, replace=False)]
    return np.stack([pick[:, 1] + rng.uniform(-0.4, 0.4, k), pick[:, 0] + rng.uniform(-0.4, 0.4, k)], axis=1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--cases", default="2048:1024,8192:4096")
    args = ap.parse_args()
    from yag_slam_amd.splicing import REFERENCE_ANGLES, RayMap, direction_table
    cs = direction_table(REFERENCE_ANGLES[::-1])
    for case in args.cases.split(","):
        n, k = (int(v) for v in case.split(":"))
        im = floor_plan(n)
        vp = viewpoints(im, k)
        with RayMap(im) as rm:
            ends, lengths = rm.trace_dirs(vp, cs)  # warm-up (code object load, buffer growth)
            assert rm.capped == 0, rm.capped
            # pixel steps: one per unit of length, a jump adds 1000 pixels in one step
            steps = float(np.where(lengths >= 1000, np.rint(lengths - 1000), np.rint(lengths)).sum())
            t = time.perf_counter()
            for _ in range(args.reps):
                rm.trace_dirs(vp, cs)
            dt = (time.perf_counter() - t) / args.reps
        print("map %d^2, %d viewpoints x %d rays: %.2f ms per trace, %.3g pixel steps (%.1f per ray), %.3g steps/s"
              % (n, k, cs.shape[0], dt * 1e3, steps, steps / lengths.size, steps / dt), flush=True)


if __name__ == "__main__":
    main()
