"""A numpy restatement of the reference's `world_to_grid` + `add_scan_to_grid` (yag_slam/helpers.py:81-83, 105-131), the
yardstick of `ym_map_add_scans`: sequential, point by point, scan by scan.

    gx, gy = round((x - ox) / res), round((y - oy) / res)     fp64 division, round half to even, then int32
    inside the grid: cgrid[gy, gx] = 1.0, then smear_point: every tap kernel[sy, sx] replaces
    cgrid[gy + sy - half, gx + sx - half] where that cell exists and holds less

It is fed the world points of the package's own Python `LocalizedRangeScan.points()` and takes its taps from
`calculate_kernel` below (helpers.py:86-97 restated; numpy's exp and the C library's may differ in the last bit, hence the
1e-15 the device tests allow on values) or from whatever table the caller passes."""
import numpy as np

HALF_GUARD = 1e-6  # fixtures keep every (x - ox) / res at least this far from a half-integer


def calculate_kernel(res, smear_deviation):
    size = int(4 * np.round(smear_deviation / res) + 1)
    kernel = np.zeros((size, size))
    half = int(size / 2)
    for i_ in range(size):
        for j_ in range(size):
            i, j = i_ - half, j_ - half
            sqdist = (i * res) ** 2 + (j * res) ** 2
            kernel[i_, j_] = np.exp(-0.5 * sqdist / (smear_deviation ** 2))
    return kernel


def world_to_grid(x, y, ox, oy, res):
    """(gx, gy) as float arrays, like helpers.py:82-83"""
    return np.round((np.asarray(x, dtype=np.float64) - ox) / res), np.round((np.asarray(y, dtype=np.float64) - oy) / res)


def distance_to_half(x, y, ox, oy, res):
    """the smallest distance of any quotient (x - ox) / res, (y - oy) / res to a half-integer: a fixture asserts it is above
    HALF_GUARD, so that a last-bit difference in the trigonometry cannot move a point to another cell"""
    q = np.concatenate([(np.asarray(x, dtype=np.float64) - ox) / res, (np.asarray(y, dtype=np.float64) - oy) / res])
    if q.size == 0:
        return np.inf
    return float(np.min(np.abs(q - np.floor(q) - 0.5)))


def add_points(cgrid, kernel, x, y, ox, oy, res):
    """add_scan_to_grid on the world points (x, y), in place.  Returns (stamped, dropped, cells): the counts and the list of
    stamped (gx, gy), one entry per stamped point."""
    h, w = cgrid.shape
    size = kernel.shape[0]
    half = int(size / 2)
    gxf, gyf = world_to_grid(x, y, ox, oy, res)
    stamped, dropped, cells = 0, 0, []
    for fx, fy in zip(gxf, gyf):
        # a quotient that is not finite or does not fit an int32 is outside every map
        if not (np.isfinite(fx) and np.isfinite(fy)) or abs(fx) >= 2.0 ** 31 or abs(fy) >= 2.0 ** 31:
            dropped += 1
            continue
        gx, gy = int(fx), int(fy)
        if not (0 <= gx < w and 0 <= gy < h):
            dropped += 1
            continue
        cgrid[gy, gx] = 1.0
        for sx in range(size):
            for sy in range(size):
                xx, yy = gx + (sx - half), gy + (sy - half)
                if 0 <= xx < w and 0 <= yy < h:
                    cand = kernel[sy, sx]
                    if cand > cgrid[yy, xx]:
                        cgrid[yy, xx] = cand
        stamped += 1
        cells.append((gx, gy))
    return stamped, dropped, cells


def add_scans(cgrid, kernel, scans, ox, oy, res):
    """every scan's `points()` at its current pose, in order.  Returns (points, stamped, dropped, cells)."""
    points = stamped = dropped = 0
    cells = []
    for s in scans:
        x, y = s.points()
        a, b, c = add_points(cgrid, kernel, x, y, ox, oy, res)
        points += len(x)
        stamped += a
        dropped += b
        cells.extend(c)
    return points, stamped, dropped, cells


def build(shape, kernel, scans, ox, oy, res):
    """a fresh grid of `shape` with `scans` added: (cgrid, (points, stamped, dropped, cells))"""
    g = np.zeros(shape, dtype=np.float64)
    return g, add_scans(g, kernel, scans, ox, oy, res)


def stamped_image(shape, cells):
    """uint8 image, 0 where a point was stamped and 255 elsewhere: `correlation_grid_from_occupancy` of it is the same map"""
    im = np.full(shape, 255, dtype=np.uint8)
    for gx, gy in cells:
        im[gy, gx] = 0
    return im
