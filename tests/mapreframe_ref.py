"""A numpy restatement of a correlation map whose window moves, beside tests/mapgrow_ref.py and
tests/mapforget_ref.py and built on them.

A window is (x0, y0, width, height) in cells of the lattice of an anchor (ax, ay) that never moves.  The cell of a reading is

    (round((x - ax) / res) - x0, round((y - ay) / res) - y0)     mapgrow_ref.world_to_grid's quotient and rounding, then the offset

so a reading keeps its lattice cell wherever the window lies.  A counted map is a function of its window and the scans it holds:
`counts` is `np.add.at` on the cells inside the window, the grid is `mapforget_ref.from_counts` of them.  `reframe_counted` restates
what ym_map_reframe does -- the kept counts shifted, the readings the old window dropped and the new one holds added -- and must
equal `build` in the new window; `shifted` is the whole reframe of a map that keeps no counts."""
import numpy as np

from tests import mapforget_ref as F
from tests import mapgrow_ref as R


def origin(anchor, window, res):
    """the world position of the window's cell (0, 0): from the anchor and the whole offset, as the library writes it"""
    return (anchor[0] + window[0] * res, anchor[1] + window[1] * res)


def moved(window, dx, dy, width=None, height=None):
    """the window after reframe(dx, dy, width, height)"""
    return (window[0] + dx, window[1] + dy, window[2] if width is None else width, window[3] if height is None else height)


def lattice_cells(scans, anchor, res):
    """the lattice cell (int, int) of every finite reading of every scan's `points()`, in order"""
    out = []
    for s in scans:
        x, y = s.points()
        gx, gy = R.world_to_grid(x, y, anchor[0], anchor[1], res)
        for fx, fy in zip(gx, gy):
            if np.isfinite(fx) and np.isfinite(fy) and abs(fx) < 2.0 ** 31 and abs(fy) < 2.0 ** 31:
                out.append((int(fx), int(fy)))
    return out


def inside(window, cell):
    x0, y0, w, h = window
    return x0 <= cell[0] < x0 + w and y0 <= cell[1] < y0 + h


def window_cells(scans, anchor, res, window):
    """(cells, dropped): the stamped (gx, gy) in cells of the window, one entry per reading inside it, and the readings outside"""
    lat = lattice_cells(scans, anchor, res)
    cells = [(cx - window[0], cy - window[1]) for cx, cy in lat if inside(window, (cx, cy))]
    return cells, len(lat) - len(cells)


def counts(scans, anchor, res, window):
    return F.counts_of((window[3], window[2]), window_cells(scans, anchor, res, window)[0])


def build(kernel, scans, anchor, res, window):
    """(grid, counts) of a fresh counted map with this anchor and window that holds `scans` at their current poses"""
    c = counts(scans, anchor, res, window)
    return F.from_counts(c, kernel), c


def shifted(a, dx, dy, width, height):
    """new[j, i] = a[j + dy, i + dx] where that exists, zero elsewhere: numpy slicing into zeros"""
    h, w = a.shape
    out = np.zeros((height, width), dtype=a.dtype)
    x0, x1, y0, y1 = max(0, -dx), min(width, w - dx), max(0, -dy), min(height, h - dy)
    if x1 > x0 and y1 > y0:
        out[y0:y1, x0:x1] = a[y0 + dy:y1 + dy, x0 + dx:x1 + dx]
    return out


def reframe_counted(old_counts, scans, anchor, res, window, dx, dy, width, height):
    """ym_map_reframe on the counts: (new counts, stats) with stats = dict(kept, restamped, dropped, mismatch).  The kept counts
    are the old ones shifted; a reading of a held scan inside the new window and outside the old one is stamped; one inside both is
    only counted, and those must sum to what the kept cells hold."""
    new = moved(window, dx, dy, width, height)
    out = shifted(old_counts, dx, dy, new[2], new[3])
    lat = lattice_cells(scans, anchor, res)
    restamped = overlap = dropped = 0
    for c in lat:
        if not inside(new, c):
            dropped += 1
        elif inside(window, c):
            overlap += 1
        else:
            out[c[1] - new[1], c[0] - new[0]] += 1
            restamped += 1
    ox0, ox1 = max(window[0], new[0]), min(window[0] + window[2], new[0] + new[2])
    oy0, oy1 = max(window[1], new[1]), min(window[1] + window[3], new[1] + new[3])
    kept = max(0, ox1 - ox0) * max(0, oy1 - oy0)
    copied = int(shifted(old_counts, dx, dy, new[2], new[3]).sum())
    return out, dict(kept=kept, restamped=restamped, dropped=dropped, mismatch=abs(copied - overlap))


def touches_difference(window, new, half):
    """bool [new height][new width]: the cells of the new window whose tap neighbourhood (+- half) meets the two windows in
    different cells -- the only cells whose value a copy cannot give"""
    out = np.zeros((new[3], new[2]), dtype=bool)
    for j in range(new[3]):
        for i in range(new[2]):
            cx, cy = new[0] + i, new[1] + j
            cut = []
            for x0, y0, w, h in (window, new):
                a0, a1, b0, b1 = max(cx - half, x0), min(cx + half + 1, x0 + w), max(cy - half, y0), min(cy + half + 1, y0 + h)
                cut.append(None if a1 <= a0 or b1 <= b0 else (a0, a1, b0, b1))
            out[j, i] = cut[0] != cut[1]
    return out
