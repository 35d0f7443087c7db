"""The live occupancy grid's statement, restated from tests/occupancy_ref.py's pieces: the rendering of a
set of scans in a GIVEN frame instead of the frame of their own bounding box.

The frame: an anchor (ax, ay) that fixes the lattice -- a world coordinate's cell is Round((p - anchor) * scale) -- and a window of
width x height cells whose cell (0, 0) is lattice cell `origin` (integers, subtracted after the rounding).  Everything else is
occupancy_ref's statement: the same readings are traced, the same line cells, the same image rule; cells outside the window are
skipped.  With anchor = render()'s offset, origin (0, 0) and render()'s size this is render()."""
import numpy as np

from tests import occupancy_ref as ref


def frame_of(scans, resolution, range_threshold, anchor):
    """the window the live grid reports for `scans` in `anchor`'s lattice: (origin (x, y), width, height), ComputeDimensions
    restated in the anchor's frame"""
    off_x, off_y, w_real, h_real = ref._frame(scans, resolution, range_threshold)
    scale = 1.0 / resolution
    origin = (int(ref.round_half_away((off_x - anchor[0]) * scale)), int(ref.round_half_away((off_y - anchor[1]) * scale)))
    return origin, int(ref.round_half_away(w_real)), int(ref.round_half_away(h_real))


def render_in_frame(scans, resolution, range_threshold, anchor, origin, width, height):
    """-> (image uint8 [height][width], passes uint32, hits uint32)"""
    passes, hits = np.zeros((height, width), dtype=np.int64), np.zeros((height, width), dtype=np.int64)
    ox, oy = int(origin[0]), int(origin[1])
    for start, ends, valid in ref._rays(scans, resolution, range_threshold, anchor[0], anchor[1]):
        sx, sy = (int(v) for v in ref.round_half_away(start))
        cells = ref.round_half_away(ends).astype(np.int64)
        for (cx, cy), ok in zip(cells.tolist(), valid.tolist()):
            xs, ys = ref.line_cells(sx, sy, cx, cy)
            xs, ys = xs - ox, ys - oy
            inside = (xs >= 0) & (xs < width) & (ys >= 0) & (ys < height)
            np.add.at(passes, (ys[inside], xs[inside]), 1)
            if ok and 0 <= cx - ox < width and 0 <= cy - oy < height:
                passes[cy - oy, cx - ox] += 1
                hits[cy - oy, cx - ox] += 1
    image = np.full((height, width), ref.UNKNOWN, dtype=np.uint8)
    seen = passes > ref.MIN_PASS
    with np.errstate(invalid="ignore", divide="ignore"):
        occupied = seen & (hits.astype(np.float64) / passes.astype(np.float64) > ref.OCC_RATIO)
    image[seen] = ref.FREE
    image[occupied] = ref.OCCUPIED
    return image, passes.astype(np.uint32), hits.astype(np.uint32)


def tie_margin_in_frame(scans, resolution, range_threshold, anchor, box_scans=None):
    """The smallest distance, in cells, from a rounding tie of any quantity the live grid rounds for `scans` in `anchor`'s
    lattice: both coordinates of every sensor position and traced end point, and the origin and size of the window of
    `box_scans` (default: `scans`; the window is that of everything ever added, which may be more than what is held)."""
    off_x, off_y, w_real, h_real = ref._frame(scans if box_scans is None else box_scans, resolution, range_threshold)
    scale = 1.0 / resolution
    vals = [np.array([w_real, h_real, (off_x - anchor[0]) * scale, (off_y - anchor[1]) * scale])]
    for start, ends, _ in ref._rays(scans, resolution, range_threshold, anchor[0], anchor[1]):
        vals += [start, ends.ravel()]
    v = np.abs(np.concatenate(vals))
    return float(np.min(np.abs(v - np.floor(v) - 0.5)))
