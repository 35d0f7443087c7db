#!/usr/bin/env python3
"""Golden vectors for `match_scan_sets` -- several query scans matched as one point set against a chain of base scans --
produced by IMPORTING the reference.

Run where the reference checkout that make_golden.py imports is present:

    python tests/golden/make_golden_scan_sets.py

Calls the reference's own `Scan2DMatcherPy.match_scan_sets` (yag_slam/scan_matching.py:56-122) on synthetic inputs,
and its `validate_points`, `find_best_pose` and `score_world_points_on_grid` (helpers.py) for the intermediate quantities.  Same
throw-away stand-ins for numba / karto_scanmatcher / tiny_tf / cv2 as make_golden.py, the planar `+` and `-` of make_golden_map.py.

The inputs are constructed on purpose and the properties the tests rely on are ASSERTED here; an input that misses one is re-seeded
(the next noise index).  Every decision the fixtures turn on -- a base reading's cell, every (hypothesis, point) rounding of both
passes, both comparisons of the valid-point filter -- lies at least 1e-9 from its boundary.

Output: tests/golden/scan_sets_*.npz (inputs + the reference's outputs; data only).
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, HERE)
sys.dont_write_bytecode = True

import make_golden_map as MGM  # noqa: E402  (installs the stand-ins and the planar + and -, imports the reference)

MG = MGM.MG
H = MG.H
SM = MGM.SM
from yag_slam_amd import synth  # noqa: E402  (own scene generator: inputs only)
from tests import scansets_ref as REF  # noqa: E402  (own restatement: used for the distances to the decision boundaries only)

MARGIN = 1e-9


def set_sums(cgrid, pts, cx, cy, ct, ox, oy, xy_s, xy_r, a_s, a_r, res):
    """integer sums of one find_best_pose lattice from the reference's score_world_points_on_grid (helpers.py:149-153) on the
    lattice helpers.py:177-179 builds (make_golden.py's sums_volume for a point set)"""
    xvals = np.arange(-xy_s + cx, xy_s + cx, xy_r)
    yvals = np.arange(-xy_s + cy, xy_s + cy, xy_r)
    tvals = np.arange(-a_s + ct, a_s + ct, a_r)
    out = np.zeros((len(tvals), len(yvals), len(xvals)), dtype=np.int64)
    for k in range(len(tvals)):
        xx, yy = H._rotate_points(pts[0], pts[1], tvals[k])
        for i in range(len(xvals)):
            for j in range(len(yvals)):
                out[k, j, i] = int(H.score_world_points_on_grid(cgrid, xvals[i] + xx, yvals[j] + yy, ox, oy, res))
    return out


def _kept(scan, vx, vy):
    px, py = scan.points()
    if len(px) == 0:
        return np.zeros((0, 2))
    kx, ky = H.validate_points(px, py, vx, vy)
    return np.array([kx, ky]).T.reshape(-1, 2)


def run_case(name, scene, cfg, n_beams, base_poses, q_truth, q_priors, penalty, do_fine, dirty=False, base_threshold=12.0,
             blank_queries=(), want=None):
    """want(info) -> None or a string saying which constructed property the input misses"""
    sensor = dict(min_angle=synth.MIN_ANGLE, angle_increment=synth.ANGLE_INCREMENT * (1081 - 1) / (n_beams - 1),
                  min_range=synth.MIN_RANGE, range_threshold=12.0)
    bsensor = dict(sensor, range_threshold=float(base_threshold))
    kw = dict(n_beams=n_beams, min_angle=sensor["min_angle"], inc=sensor["angle_increment"])
    for seed in range(64):
        base_ranges = [scene.scan_ranges(p, index=10 + 100 * seed + i, dirty=dirty, **kw) for i, p in enumerate(base_poses)]
        q_ranges = [scene.scan_ranges(t, index=600 + 100 * seed + i, dirty=dirty, **kw) for i, t in enumerate(q_truth)]
        for i in blank_queries:  # a query scan without a valid reading: NaN and over-range only
            q_ranges[i] = np.where(np.arange(n_beams) % 2 == 0, np.nan, 31.0)
        base = [MG.RefScan(r, bsensor, p) for r, p in zip(base_ranges, base_poses)]
        queries = [MG.RefScan(r, sensor, p) for r, p in zip(q_ranges, q_priors)]
        m = SM.Scan2DMatcherPy(cfg)
        r = m.match_scan_sets(queries, base, penalty, do_fine)
        grid = r.meta["grid"]
        G = grid.shape[0]
        res = m.resolution
        xs, ys = zip(*[(q.corrected_pose.x, q.corrected_pose.y) for q in queries])
        cx, cy = sum(xs) / float(len(xs)), sum(ys) / float(len(ys))
        ox, oy = cx - 0.5 * (G - 1) * res, cy - 0.5 * (G - 1) * res
        xl = np.hstack([q.points()[0] for q in queries])
        yl = np.hstack([q.points()[1] for q in queries])
        xl, yl = H._transform_points(xl, yl, -cx, -cy, 0)
        coarse = H.find_best_pose(grid, (xl, yl), cx, cy, 0, ox, oy, m.search_size * 0.5, res * 2, m.angle_size * 0.5, m.angle_res,
                                  res, penalty)
        fin = coarse
        if do_fine:
            fin = H.find_best_pose(grid, (xl, yl), coarse[1], coarse[2], coarse[3], ox, oy, res * 2, res, 0.0349 * 0.5, 0.00349, res,
                                   penalty)
        assert float(r.response) == float(fin[0])
        last, first = queries[-1].corrected_pose, queries[0].corrected_pose
        kept_last = [_kept(b, last.x, last.y) for b in base]
        kept_first = [_kept(b, first.x, first.y) for b in base]
        kept_mean = [_kept(b, cx, cy) for b in base]
        # the distances to the decision boundaries, from the package's own restatement of the call on the same inputs
        full = dict(search_size=m.search_size, coarse_search_angle_offset=m.angle_size, coarse_angle_resolution=m.angle_res,
                    resolution=res, smear_deviation=m.smear_deviation, range_threshold=m.range_threshold)
        ref = REF.match_scan_sets(full, [(rr, p, sensor) for rr, p in zip(q_ranges, q_priors)],
                                  [(rr, p, bsensor) for rr, p in zip(base_ranges, base_poses)], penalty, do_fine)
        info = dict(G=G, ox=ox, oy=oy, res=res, half=r.meta["kernel"].shape[0] // 2, base=base, kept_last=kept_last,
                    kept_first=kept_first, kept_mean=kept_mean)
        miss = None
        if not (ref["tie"] >= MARGIN and ref["near_d"] >= MARGIN and ref["near_s"] >= MARGIN):
            miss = "a decision within %g of its boundary (tie %.3g, d^2 %.3g, ss %.3g)" % (MARGIN, ref["tie"], ref["near_d"], ref["near_s"])
        elif want:
            miss = want(info)
        if miss:
            print("%-26s seed %d: %s -- re-seeding" % (name, seed, miss))
            continue
        break
    else:
        raise SystemExit("%s: no seed gives the constructed properties" % name)
    coarse_sums = set_sums(grid, (xl, yl), cx, cy, 0, ox, oy, m.search_size * 0.5, res * 2, m.angle_size * 0.5, m.angle_res, res)
    out = dict(
        sensor_min_angle=sensor["min_angle"], sensor_angle_increment=sensor["angle_increment"], sensor_min_range=sensor["min_range"],
        q_thresholds=np.full(len(queries), sensor["range_threshold"]), base_thresholds=np.full(len(base), bsensor["range_threshold"]),
        cfg_keys=np.array(sorted(full.keys())), cfg_vals=np.array([float(full[k]) for k in sorted(full.keys())]),
        base_ranges=np.array(base_ranges), base_poses=np.array(base_poses, dtype=np.float64),
        q_ranges=np.array(q_ranges), q_poses=np.array(q_priors, dtype=np.float64),
        penalty=int(penalty), do_fine=int(do_fine), grid_size=G, centre=np.array([cx, cy]),
        valid_counts=np.array([len(k) for k in kept_last], dtype=np.int32),
        valid_counts_first=np.array([len(k) for k in kept_first], dtype=np.int32),
        valid_counts_mean=np.array([len(k) for k in kept_mean], dtype=np.int32))
    nzy, nzx = np.nonzero(grid)
    out.update(grid_nz_y=nzy.astype(np.int32), grid_nz_x=nzx.astype(np.int32), grid_nz_val=grid[nzy, nzx],
               pts_local_x=xl, pts_local_y=yl, coarse=np.array(coarse, dtype=np.float64), final=np.array(fin, dtype=np.float64),
               coarse_sums=coarse_sums.astype(np.int32), response=float(r.response),
               covariance=np.array(r.covariance, dtype=np.float64),
               poses=np.array([[p.x, p.y, p.euler[-1]] for p in r.best_pose], dtype=np.float64),
               margin_tie=ref["tie"], margin_d2=ref["near_d"], margin_ss=ref["near_s"])
    if do_fine:
        out["fine_sums"] = set_sums(grid, (xl, yl), coarse[1], coarse[2], coarse[3], ox, oy, res * 2, res, 0.0349 * 0.5, 0.00349,
                                    res).astype(np.int32)
    path = os.path.join(HERE, name + ".npz")
    np.savez_compressed(path, **out)
    print("%-26s G=%d nz=%d pts=%d kept %s (first %s, mean %s) coarse %s resp %.9f -> %.9f margins %.2g %.2g %.2g, %d bytes" % (
        name, G, len(nzx), len(xl), out["valid_counts"].tolist(), out["valid_counts_first"].tolist(),
        out["valid_counts_mean"].tolist(), coarse_sums.shape, coarse[0], fin[0], ref["tie"], ref["near_d"], ref["near_s"],
        os.path.getsize(path)))


def _differs(a, b):
    return any(x.shape != y.shape or not np.array_equal(x, y) for x, y in zip(a, b))


def want_view_points_differ(info):
    if not _differs(info["kept_last"], info["kept_first"]):
        return "the kept readings under the last and the first query's view-point are equal"
    if not _differs(info["kept_last"], info["kept_mean"]):
        return "the kept readings under the last query's view-point and under the mean are equal"
    return None


def want_readings_and_taps_outside(info):
    G, half, res = info["G"], info["half"], info["res"]
    outside = edge = 0
    for k in info["kept_last"]:
        if len(k) == 0:
            continue
        gx = np.round((k[:, 0] - info["ox"]) / res)
        gy = np.round((k[:, 1] - info["oy"]) / res)
        inside = (gx >= 0) & (gx < G) & (gy >= 0) & (gy < G)
        outside += int((~inside).sum())
        edge += int((inside & ((gx < half) | (gx >= G - half) | (gy < half) | (gy >= G - half))).sum())
    if not outside:
        return "no kept reading falls outside the grid"
    if not edge:
        return "no kept stamp has a tap outside the grid"
    return None


def main():
    room = synth.Scene()
    cfg05 = dict(resolution=0.05, smear_deviation=0.05, range_threshold=12.0)
    base3 = [(2.0 + 0.1 * i, 3.0, 0.0) for i in range(3)]
    # (a) two queries, penalty, fine pass
    run_case("scan_sets_two", room, cfg05, 181, base3, [(2.37, 3.04, 0.05), (2.47, 3.05, 0.06)],
             [(2.30, 3.00, 0.0), (2.40, 3.0, 0.0)], True, True)
    # (b) a set of one, no penalty, coarse only
    run_case("scan_sets_one_coarse", room, cfg05, 271, base3[:2], [(2.33, 2.96, -0.04)], [(2.30, 3.00, 0.0)], False, False)
    # (c) three dirty queries around a thin obstacle: the first two below it, the last above -- the view-point of the filter is the last
    thin = synth.Scene()
    thin.segs = np.vstack([thin.segs, [[3.4, 2.5, 4.6, 2.5]]])
    run_case("scan_sets_dirty_three", thin, dict(resolution=0.05, smear_deviation=0.1, range_threshold=12.0), 271,
             [(3.6, 3.3, -1.2), (4.0, 3.4, -1.6), (4.4, 3.3, -2.0)],
             [(3.9, 2.2, 1.5), (4.0, 2.3, 1.55), (4.1, 2.8, 1.6)], [(3.87, 2.17, 1.48), (3.97, 2.27, 1.52), (4.07, 2.77, 1.57)],
             True, True, dirty=True, want=want_view_points_differ)
    # (d) a long hall and a base scan whose sensor sees 20 m: readings beyond the 12 m grid, stamps on its rim
    hall = synth.Scene(width=28.0, height=6.0)
    run_case("scan_sets_far_base", hall, cfg05, 361, [(9.0, 3.0, 0.0), (3.2, 3.0, 0.1)], [(3.07, 3.04, 0.05), (3.17, 3.05, 0.06)],
             [(3.0, 3.0, 0.0), (3.1, 3.0, 0.0)], True, True, base_threshold=20.0, want=want_readings_and_taps_outside)
    # (e) 2 cm cells, another search size and smear; the middle query has no valid reading
    run_case("scan_sets_r02_blank", room, dict(resolution=0.02, smear_deviation=0.04, range_threshold=12.0, search_size=0.36), 181,
             base3[:2], [(2.35, 3.03, 0.04), (2.40, 3.0, 0.0), (2.45, 3.04, 0.05)],
             [(2.30, 3.00, 0.0), (2.36, 3.01, 0.0), (2.40, 3.0, 0.0)], True, True, blank_queries=(1,))


if __name__ == "__main__":
    main()
