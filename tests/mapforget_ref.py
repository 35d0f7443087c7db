"""A numpy restatement of what a counted correlation map holds, beside tests/mapgrow_ref.py and built on
it: the counts are `np.add.at` on the cells the restatement of `add_scan_to_grid` stamps, a removal is a decrement, and the map
is a function of the counts -- `from_counts`, every cell with a positive count stamped by the restatement's own loop."""
import numpy as np

from tests import mapgrow_ref as R


def cells_of(scans, shape, ox, oy, res):
    """the stamped (gx, gy) of every scan's `points()` at its current pose, one entry per stamped reading"""
    return R.build(shape, np.ones((1, 1)), scans, ox, oy, res)[1][3]


def counts_of(shape, cells):
    counts = np.zeros(shape, dtype=np.int64)
    if cells:
        c = np.asarray(cells, dtype=np.int64)
        np.add.at(counts, (c[:, 1], c[:, 0]), 1)
    return counts


def remove(counts, cells):
    """the decrement, in place; a count below zero is the caller's error and an assertion here"""
    if cells:
        c = np.asarray(cells, dtype=np.int64)
        np.add.at(counts, (c[:, 1], c[:, 0]), -1)
    assert counts.min() >= 0
    return counts


def from_counts(counts, kernel):
    """the map of the image counts > 0: add_scan_to_grid's stamp and smear (mapgrow_ref.add_points) on one point per such cell"""
    g = np.zeros(counts.shape, dtype=np.float64)
    ys, xs = np.nonzero(counts > 0)
    # a point at the centre of cell (gx, gy) of a grid with origin 0 and cell size 1 lands in that cell
    R.add_points(g, kernel, xs.astype(np.float64), ys.astype(np.float64), 0.0, 0.0, 1.0)
    return g
