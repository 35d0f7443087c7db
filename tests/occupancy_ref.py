"""Occupancy-grid rendering restated in numpy and Python integers (fp64), from the statement of the algorithm in the header of
yag_slam_amd/csrc/ym_k_occupancy.hpp and SURVEY.md 8f-4 -- not from the kernel's or the oracle's code, which are twins of one
another.  It is written the other way round wherever the statement allows it: readings are classified for all beams of a
scan at once, and a ray's cells come from the closed form of the line walk instead of a running error term.

The statement.  render(scans, resolution, range_threshold), scale = 1 / resolution:
  * beam i of a scan at pose (x, y, heading) points along heading + min_angle + i * angle_increment; its reading r ends at
    (x + r cos, y + r sin).
  * bounding box: every sensor position, and the end of every reading with min_range <= r <= range_threshold.  The offset is
    the box's minimum corner; width = Round((xmax - xmin) * scale), height likewise.  Round is half away from zero.
  * a reading with r <= min_range, r >= max_range or NaN is ignored.  Any other is traced from the sensor; one with
    r >= range_threshold only as far as range_threshold along the beam.  Its end point is VALID when
    r < range_threshold - 1e-6.
  * a world point's cell is Round((p - offset) * scale), per coordinate.  The ray's cells are those of Bresenham's line
    between the two cells, both ends included (the walk below); cells outside the grid are skipped, nothing else stops the
    walk.  Every cell of the line gets one pass.  A valid end point inside the grid gets one more pass, and one hit.
  * image: 200 (unknown) unless passes > 2; then 0 (occupied) when hits / passes > 0.1, else 255 (free).

The walk (Grid::TraceLine).  With the steeper axis as the major one, the line runs from the end with the smaller major
coordinate (A) to the other (B), one cell per major step.  After k steps the minor coordinate has moved m(k) cells towards B's,
where m(k) is the integer with -dM <= 2 (k dm - m(k) dM) < dM (dM, dm >= 0 the major and minor extents): the running error
2 * error >= dM moves the minor coordinate AFTER the cell is visited, so m(k) = floor((2 k dm + dM) / (2 dM)), m = 0 for a
single cell.  Equal extents count as not steep (x is the major axis).
"""
import math

import numpy as np

TOLERANCE = 1e-6   # KT_TOLERANCE
MIN_PASS = 2       # MinPassThrough
OCC_RATIO = 0.1    # OccupancyThreshold
OCCUPIED, UNKNOWN, FREE = 0, 200, 255


def round_half_away(v):
    """Karto's math::Round, elementwise: floor(v + 0.5) for v >= 0, ceil(v - 0.5) below"""
    v = np.asarray(v, dtype=np.float64)
    return np.where(v >= 0.0, np.floor(v + 0.5), np.ceil(v - 0.5))


def _pose(scan):
    p = scan.corrected_pose
    return float(p.x), float(p.y), float(p.euler[-1])


def _ends(scan, reach=None):
    """world end points of every beam (libm's cos and sin, one call per beam); reach: readings beyond it end at it"""
    x, y, t = _pose(scan)
    r = np.asarray(scan.ranges, dtype=np.float64)
    ex, ey = np.empty(r.shape[0]), np.empty(r.shape[0])
    for i in range(r.shape[0]):
        a = t + scan.min_angle + i * scan.angle_increment
        ri = float(r[i])
        px, py = x + ri * math.cos(a), y + ri * math.sin(a)
        if reach is not None and ri >= reach:
            f = reach / ri
            px, py = x + f * (px - x), y + f * (py - y)
        ex[i], ey[i] = px, py
    return ex, ey


def _frame(scans, resolution, range_threshold):
    """the bounding box -> (off_x, off_y, width as a real number before rounding, height likewise)"""
    xs, ys = [], []
    for s in scans:
        x, y, _ = _pose(s)
        r = np.asarray(s.ranges, dtype=np.float64)
        with np.errstate(invalid="ignore"):
            boxed = (r >= s.min_range) & (r <= range_threshold)
        ex, ey = _ends(s)
        xs += [np.array([x]), ex[boxed]]
        ys += [np.array([y]), ey[boxed]]
    xs, ys = np.concatenate(xs), np.concatenate(ys)
    scale = 1.0 / resolution
    return float(xs.min()), float(ys.min()), float((xs.max() - xs.min()) * scale), float((ys.max() - ys.min()) * scale)


def _rays(scans, resolution, range_threshold, off_x, off_y):
    """per scan: (start cell coordinates (2,), end cell coordinates (k, 2), valid (k,)) of the traced beams, as real numbers
    before rounding"""
    scale = 1.0 / resolution
    out = []
    for s in scans:
        x, y, _ = _pose(s)
        r = np.asarray(s.ranges, dtype=np.float64)
        with np.errstate(invalid="ignore"):
            ignored = (r <= s.min_range) | (r >= s.max_range) | np.isnan(r)
            valid = r < range_threshold - TOLERANCE
        ex, ey = _ends(s, reach=range_threshold)
        traced = ~ignored
        ends = np.stack([(ex[traced] - off_x) * scale, (ey[traced] - off_y) * scale], axis=1)
        out.append((np.array([(x - off_x) * scale, (y - off_y) * scale]), ends, valid[traced]))
    return out


def line_cells(x0, y0, x1, y1):
    """the cells of the walk from cell (x0, y0) to cell (x1, y1) (Python ints) -> (xs, ys), int64 arrays"""
    steep = abs(y1 - y0) > abs(x1 - x0)
    a, b = ((y0, x0), (y1, x1)) if steep else ((x0, y0), (x1, y1))   # (major, minor)
    if a[0] > b[0]:
        a, b = b, a
    d_major, d_minor = b[0] - a[0], abs(b[1] - a[1])
    k = np.arange(d_major + 1, dtype=np.int64)
    m = (2 * k * d_minor + d_major) // (2 * d_major) if d_major else np.zeros(1, dtype=np.int64)
    major, minor = a[0] + k, a[1] + (m if b[1] > a[1] else -m)
    return (minor, major) if steep else (major, minor)


def render(scans, resolution, range_threshold):
    """-> (image uint8 [h][w] or None when the rounded width or height is <= 0, passes uint32 [h][w], hits uint32 [h][w],
    (off_x, off_y)); without an image the count arrays are empty"""
    off_x, off_y, w_real, h_real = _frame(scans, resolution, range_threshold)
    width, height = int(round_half_away(w_real)), int(round_half_away(h_real))
    if width <= 0 or height <= 0:
        return None, np.zeros((0, 0), np.uint32), np.zeros((0, 0), np.uint32), (off_x, off_y)
    passes, hits = np.zeros((height, width), dtype=np.int64), np.zeros((height, width), dtype=np.int64)
    for start, ends, valid in _rays(scans, resolution, range_threshold, off_x, off_y):
        sx, sy = (int(v) for v in round_half_away(start))
        cells = round_half_away(ends).astype(np.int64)
        for (cx, cy), ok in zip(cells.tolist(), valid.tolist()):
            xs, ys = line_cells(sx, sy, cx, cy)
            inside = (xs >= 0) & (xs < width) & (ys >= 0) & (ys < height)
            np.add.at(passes, (ys[inside], xs[inside]), 1)   # (a line visits a cell once, but keep it a sum)
            if ok and 0 <= cx < width and 0 <= cy < height:
                passes[cy, cx] += 1
                hits[cy, cx] += 1
    image = np.full((height, width), UNKNOWN, dtype=np.uint8)
    seen = passes > MIN_PASS
    with np.errstate(invalid="ignore", divide="ignore"):
        occupied = seen & (hits.astype(np.float64) / passes.astype(np.float64) > OCC_RATIO)
    image[seen] = FREE
    image[occupied] = OCCUPIED
    return image, passes.astype(np.uint32), hits.astype(np.uint32), (off_x, off_y)


def tie_margin(scans, resolution, range_threshold):
    """The smallest distance, in cells, of any quantity that render() rounds from a rounding tie (k + 0.5): both grid
    coordinates of every sensor position and of every traced end point, and the width and the height.  A rendering whose
    margin exceeds the error of another implementation's arithmetic in these quantities must come out cell for cell the same."""
    off_x, off_y, w_real, h_real = _frame(scans, resolution, range_threshold)
    vals = [np.array([w_real, h_real])]
    for start, ends, _ in _rays(scans, resolution, range_threshold, off_x, off_y):
        vals += [start, ends.ravel()]
    v = np.abs(np.concatenate(vals))
    return float(np.min(np.abs(v - np.floor(v) - 0.5)))
