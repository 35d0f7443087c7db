"""A numpy restatement of `ym_map_seen_through`: which readings a counted map holds do newer scans look
straight through?  Beside tests/mapreframe_ref.py, whose window and cell rule it shares.

A counted map has a window (wx0, wy0, w, h) in cells of the lattice of an anchor (ox, oy) and a cell size res.

  cells       the cell of a world point is (round((x - ox) / res) - wx0, round((y - oy) / res) - wy0): fp64 division, round half to
              even; a quotient that is not finite or does not fit an int32 yields no cell.  A reading is valid when
              not (r > range_threshold or isnan(r)).  A viewer's sensor cell is the cell of its pose's position; a viewer without one
              walks no ray.
  rays        every valid viewer reading with a cell gives a ray from the sensor cell to the reading's cell (`walk`): swap the axes
              if the ray is steep, walk from the lower major coordinate; after k of dM major steps the minor coordinate has moved
              floor((2 k dm + dM) / (2 dM)) cells.  A cell's distance to the end is dM - k, or k where the walk started at the
              reading's cell.  A cell is swept when it lies in the window and its distance to the end is greater than `clearance`.
              A ray of 32768 major steps or more sweeps nothing (no admitted matcher's sensor gives one).
  protection  a cell within Chebyshev distance `protect` of the end cell of any valid viewer reading is not swept, whichever ray
              passed through it.
  counts      per held scan, at the pose it was added at: `inside` = its valid readings whose cell lies in the window, `seen` =
              those of them whose cell is swept; a flag per beam, 1 exactly for the readings counted in `seen`.

A scan here is anything with `ranges`, `min_angle`, `angle_increment` and `range_threshold`; poses are (x, y, heading)."""
import numpy as np

HALF_GUARD = 1e-6  # fixtures keep every quotient at least this far from a half-integer (tests/mapgrow_ref.py's guard)
MAX_STEPS = 32768  # a ray with this many major steps or more sweeps nothing


def pose_of(scan):
    p = scan.corrected_pose
    return (float(p.x), float(p.y), float(p.euler[-1]))


def beam_points(scan, pose):
    """(valid, x, y) per beam: _get_point_readings' rule and project_points' expressions; x, y are NaN on invalid beams"""
    r = np.asarray(scan.ranges, dtype=np.float64)
    with np.errstate(invalid="ignore"):
        valid = ~((r > scan.range_threshold) | np.isnan(r))
    ang = pose[2] + scan.min_angle + np.arange(len(r)) * scan.angle_increment
    with np.errstate(invalid="ignore", over="ignore"):
        x, y = pose[0] + r * np.cos(ang), pose[1] + r * np.sin(ang)
    return valid, np.where(valid, x, np.nan), np.where(valid, y, np.nan)


def quotients(v, o, res):
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        return (np.asarray(v, dtype=np.float64) - o) / res


def coord(v, o, res, w0):
    """(has a cell, the window coordinate as a Python int or None) of one world coordinate"""
    q = np.round(quotients(v, o, res))
    if not np.isfinite(q) or abs(q) >= 2.0 ** 31:
        return None
    return int(q) - w0


def cell(x, y, window, anchor, res):
    cx, cy = coord(x, anchor[0], res, window[0]), coord(y, anchor[1], res, window[1])
    return None if cx is None or cy is None else (cx, cy)


def beam_cells(scan, pose, window, anchor, res):
    """per beam: the window cell (cx, cy) -- it may lie outside the window -- or None (invalid, or no cell)"""
    valid, x, y = beam_points(scan, pose)
    return [cell(x[i], y[i], window, anchor, res) if valid[i] else None for i in range(len(valid))]


def distance_to_half(scans_and_poses, anchor, res, sensors=True):
    """the smallest distance of any reading's quotient -- and, with `sensors`, of any pose's -- to a half-integer"""
    best = np.inf
    for scan, pose in scans_and_poses:
        valid, x, y = beam_points(scan, pose)
        q = [quotients(x[valid], anchor[0], res), quotients(y[valid], anchor[1], res)]
        if sensors:
            q.append(quotients(np.array([pose[0]]), anchor[0], res))
            q.append(quotients(np.array([pose[1]]), anchor[1], res))
        q = np.concatenate(q)
        q = q[np.isfinite(q)]
        if q.size:
            best = min(best, float(np.min(np.abs(q - np.floor(q) - 0.5))))
    return best


def walk(sx, sy, ex, ey):
    """the cells of the ray from sensor cell (sx, sy) to end cell (ex, ey) and their distances to the end: (xs, ys, dist), Python
    ints in int64 arrays, in the order of the walk"""
    steep = abs(ey - sy) > abs(ex - sx)
    a, b = ((sy, sx), (ey, ex)) if steep else ((sx, sy), (ex, ey))  # (major, minor)
    from_end = a[0] > b[0]
    if from_end:
        a, b = b, a
    d_major, d_minor = b[0] - a[0], abs(b[1] - a[1])
    k = np.arange(d_major + 1, dtype=np.int64)
    m = (2 * k * d_minor + d_major) // (2 * d_major) if d_major else np.zeros(1, dtype=np.int64)
    major, minor = a[0] + k, a[1] + (m if b[1] > a[1] else -m)
    dist = k if from_end else d_major - k
    return ((minor, major) if steep else (major, minor)) + (dist,)


def swept_mask(window, anchor, res, viewers, clearance, protect):
    """(mask uint8 [h][w]: the swept cells after protection, rays: the viewer readings that gave a ray).  viewers: (scan, pose)"""
    _, _, w, h = window
    mask = np.zeros((h, w), dtype=np.uint8)
    ends, rays = [], 0
    for scan, pose in viewers:
        cells = [c for c in beam_cells(scan, pose, window, anchor, res) if c is not None]
        ends.extend(cells)
        sensor = cell(pose[0], pose[1], window, anchor, res)
        if sensor is None:
            continue
        for ex, ey in cells:
            rays += 1
            if max(abs(ex - sensor[0]), abs(ey - sensor[1])) >= MAX_STEPS:
                continue
            xs, ys, dist = walk(sensor[0], sensor[1], ex, ey)
            hit = (dist > clearance) & (xs >= 0) & (xs < w) & (ys >= 0) & (ys < h)
            mask[ys[hit], xs[hit]] = 1
    for ex, ey in ends:
        x0, x1, y0, y1 = max(ex - protect, 0), min(ex + protect + 1, w), max(ey - protect, 0), min(ey + protect + 1, h)
        if x0 < x1 and y0 < y1:
            mask[y0:y1, x0:x1] = 0
    return mask, rays


def seen_through(window, anchor, res, held, viewers, clearance, protect):
    """held, viewers: lists of (scan, pose) -- the held scans at the poses they were added at, the viewers at their current ones.
    Returns (inside, seen, flags, mask, rays): int arrays per held scan, a list of boolean arrays per beam, the swept mask."""
    _, _, w, h = window
    mask, rays = swept_mask(window, anchor, res, viewers, clearance, protect)
    inside, seen, flags = [], [], []
    for scan, pose in held:
        cells = beam_cells(scan, pose, window, anchor, res)
        f = np.zeros(len(cells), dtype=bool)
        n_in = 0
        for i, c in enumerate(cells):
            if c is not None and 0 <= c[0] < w and 0 <= c[1] < h:
                n_in += 1
                f[i] = bool(mask[c[1], c[0]])
        inside.append(n_in)
        seen.append(int(f.sum()))
        flags.append(f)
    return np.array(inside, dtype=np.int64), np.array(seen, dtype=np.int64), flags, mask, rays


def blanked_ranges(ranges, flags):
    """`LocalizedRangeScan.blanked`'s readings: NaN where flagged"""
    r = np.array(ranges, dtype=np.float64).copy()
    r[np.asarray(flags, dtype=bool)] = np.nan
    return r
