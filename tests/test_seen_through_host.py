"""tests/seenthrough_ref.py, the restatement of `ym_map_seen_through`, on the CPU: its closed-form walk
against an independent running-error Bresenham loop, the distance-to-end bookkeeping under both swaps, protection over sweeping,
and the room-and-box scene at true poses -- the check that what tests/test_gpu_map_seen_through.py's MapBuilder scenario asks of
the device is reachable at all."""
import math

import numpy as np

from tests import seenthrough_ref as S
from yag_slam_amd import synth
from yag_slam_amd.models import LocalizedRangeScan


def _bresenham(x0, y0, x1, y1):
    """Grid::TraceLine with its running error, cell by cell: [(x, y)] in the order of the walk"""
    steep = abs(y1 - y0) > abs(x1 - x0)
    if steep:
        x0, y0, x1, y1 = y0, x0, y1, x1
    if x0 > x1:
        x0, x1, y0, y1 = x1, x0, y1, y0
    delta_x, delta_y = x1 - x0, abs(y1 - y0)
    error, y, ystep = 0, y0, (1 if y0 < y1 else -1)
    out = []
    for x in range(x0, x1 + 1):
        out.append((y, x) if steep else (x, y))
        error += delta_y
        if 2 * error >= delta_x:
            y += ystep
            error -= delta_x
    return out


def _assert_walk(sx, sy, ex, ey):
    xs, ys, dist = S.walk(sx, sy, ex, ey)
    cells = list(zip(xs.tolist(), ys.tolist()))
    assert cells == _bresenham(sx, sy, ex, ey), (sx, sy, ex, ey)
    # the distance to the end: 0 on the reading's cell, the number of major steps on the sensor's, one less with every step between
    d_major = max(abs(ex - sx), abs(ey - sy))
    assert len(cells) == d_major + 1
    by_cell = dict(zip(cells, dist.tolist()))
    assert by_cell[(ex, ey)] == 0 and by_cell[(sx, sy)] == d_major
    order = cells if cells[0] == (sx, sy) else cells[::-1]
    assert [by_cell[c] for c in order] == list(range(d_major, -1, -1))
    # and it is the number of major steps left, whichever axis is the major one
    major = 1 if abs(ey - sy) > abs(ex - sx) else 0
    assert all(by_cell[c] == abs((ex, ey)[major] - c[major]) for c in cells)


def test_the_closed_form_walk_is_bresenhams_on_every_ray_of_a_block_and_on_long_rays():
    for sx in range(9):
        for sy in range(9):
            for ex in range(9):
                for ey in range(9):
                    _assert_walk(sx - 4, sy - 4, ex - 4, ey - 4)  # all octants, dM = 0, axis rays, diagonals, negative cells
    rng = np.random.default_rng(5)
    for _ in range(300):
        sx, sy = (int(v) for v in rng.integers(-50, 50, 2))
        dx, dy = (int(v) for v in rng.integers(-300, 301, 2))
        _assert_walk(sx, sy, sx + dx, sy + dy)


def test_the_distance_to_the_end_under_both_swaps():
    # (sensor, end, is the walk started at the end): shallow and steep, towards higher and towards lower coordinates
    for (sx, sy, ex, ey), from_end in (((2, 3, 12, 7), False), ((12, 7, 2, 3), True), ((3, 2, 7, 12), False), ((7, 12, 3, 2), True),
                                       ((2, 7, 12, 3), False), ((7, 2, 3, 12), False), ((3, 12, 7, 2), True)):
        xs, ys, dist = S.walk(sx, sy, ex, ey)
        assert ((xs[0], ys[0]) == (ex, ey)) == from_end
        assert dist.tolist() == (list(range(0, 11)) if from_end else list(range(10, -1, -1)))
        assert (xs[-1], ys[-1]) == ((sx, sy) if from_end else (ex, ey))


class _Beams(object):
    """a scan by its fields: what the restatement reads"""

    def __init__(self, ranges, min_angle, inc, threshold=12.0):
        self.ranges, self.min_angle, self.angle_increment, self.range_threshold = np.asarray(ranges, dtype=np.float64), min_angle, inc, threshold


def _aimed(sensor, ends, res, threshold=12.0):
    """a viewer at the centre of cell `sensor` whose beams end on the centres of the cells `ends` (anchor (0, 0), heading 0): the
    beams' angles are free, so this scan carries one angle per beam in `min_angle` (numpy broadcasts it)"""
    sx, sy = sensor[0] * res, sensor[1] * res
    d = np.array([(ex * res - sx, ey * res - sy) for ex, ey in ends], dtype=np.float64)
    return _Beams(np.hypot(d[:, 0], d[:, 1]), np.arctan2(d[:, 1], d[:, 0]), 0.0, threshold), (sx, sy, 0.0)


def test_clearance_and_protection():
    res, window, anchor = 0.05, (0, 0, 40, 30), (0.0, 0.0)
    # one ray along a row: everything but the last `clearance` + 1 cells is swept
    v = _aimed((5, 10), [(25, 10)], res)
    for clearance in (0, 2, 5, 19, 20, 21):
        mask, rays = S.swept_mask(window, anchor, res, [v], clearance, 0)
        want = np.zeros((30, 40), dtype=np.uint8)
        want[10, 5:max(5, 25 - clearance)] = 1
        assert rays == 1 and np.array_equal(mask, want), clearance
    # a second, shorter reading on the same row: its end's neighbourhood is not swept, whichever ray passed through it
    v = _aimed((5, 10), [(25, 10), (15, 10), (25, 11)], res)
    for protect in (0, 1, 3):
        mask, rays = S.swept_mask(window, anchor, res, [v], 2, protect)
        assert rays == 3 and not mask[10 - protect:10 + protect + 1, 15 - protect:15 + protect + 1].any()
        assert mask[10, 5:15 - protect].all() and mask[10, 15 + protect + 1:25 - max(2, protect) - 1].all()
        assert not mask[:, 25 - protect:].any()
    unprotected, _ = S.swept_mask(window, anchor, res, [_aimed((5, 10), [(25, 10), (25, 11)], res)], 2, 0)
    assert unprotected[10, 15] == 1
    # a held reading on a swept cell is seen, one on a protected or untouched cell is not; one outside the window is not inside
    held = _aimed((0, 0), [(10, 10), (15, 10), (30, 20), (45, 10)], res)
    inside, seen, flags, _, _ = S.seen_through(window, anchor, res, [held], [v], 2, 1)
    assert (inside.tolist(), seen.tolist(), flags[0].tolist()) == ([3], [1], [True, False, False, False])
    # no sensor cell: no ray is walked, but the ends still protect; an over-long ray sweeps nothing and still counts as a ray
    blind = (v[0], (float("nan"), 10 * res, 0.0))
    mask, rays = S.swept_mask(window, anchor, res, [blind], 0, 0)
    assert rays == 0 and not mask.any()
    far = _aimed((5, 10), [(5 - S.MAX_STEPS, 10), (6 - S.MAX_STEPS, 10)], res, threshold=1.0e9)
    mask, rays = S.swept_mask(window, anchor, res, [far], 0, 0)
    assert rays == 2 and np.array_equal(np.argwhere(mask), [[10, x] for x in range(0, 6)])


# ---- the room and the box: shared with tests/test_gpu_map_seen_through.py ------------------------------------------------------
ROOM_RES, ROOM_BEAMS, ROOM_MIN_ANGLE, ROOM_INC, ROOM_RANGE = 0.05, 361, -math.pi, 2.0 * math.pi / 360.0, 12.0
ROOM_ANCHOR, ROOM_WINDOW = (-1.513, -1.487), (0, 0, 260, 220)
BOX = (4.5, 5.5, 3.5, 4.5)  # x0, x1, y0, y1: 1 m at the centre of the 10 m x 8 m room


def room_scenes():
    """(the room with the box, the room without it)"""
    with_box, empty = synth.Scene(10, 8, n_boxes=0), synth.Scene(10, 8, n_boxes=0)
    x0, x1, y0, y1 = BOX
    with_box.segs = np.vstack([with_box.segs, [(x0, y0, x1, y0), (x1, y0, x1, y1), (x1, y1, x0, y1), (x0, y1, x0, y0)]])
    return with_box, empty


def room_cast(scene, pose):
    return scene.cast(pose[0], pose[1], pose[2], n_beams=ROOM_BEAMS, min_angle=ROOM_MIN_ANGLE, inc=ROOM_INC)


def room_scan(scene, truth, index, pose=None):
    """the 361-beam scan `scene` gives at `truth` (1 cm range noise, seed 1000 + index), placed at `pose` (None: at `truth`)"""
    r = scene.scan_ranges(truth, index=index, n_beams=ROOM_BEAMS, min_angle=ROOM_MIN_ANGLE, inc=ROOM_INC)
    p = truth if pose is None else pose
    return LocalizedRangeScan(r, ROOM_MIN_ANGLE, ROOM_MIN_ANGLE + (ROOM_BEAMS - 1) * ROOM_INC, ROOM_INC, synth.MIN_RANGE, synth.MAX_RANGE,
                              ROOM_RANGE, p[0], p[1], p[2])


def on_box(with_box, empty, truth):
    """bool per beam, from the two noise-free casts: the box is what the beam hits"""
    return room_cast(with_box, truth) < room_cast(empty, truth) - 1e-9


OLD_POSES = [(5.0 + 2.6 * math.cos(a), 4.0 + 2.2 * math.sin(a), a + 2.0) for a in (0.3 + k * math.pi / 3.0 for k in range(6))]
NEW_POSES = [(2.2, 3.1, 0.4), (7.9, 5.2, 2.5)]


def test_the_room_and_the_box_at_true_poses():
    """Six scans around the box, then the box is taken away: two new scans look through every reading the six had on the box and
    through none they had on a wall (clearance 2, protect 1 and 2); while the box stands, protect 2 leaves at most a few grazing
    readings (the counts are printed: they are what the defaults rest on, on this one scene)."""
    with_box, empty = room_scenes()
    olds = [room_scan(with_box, p, 500 + i) for i, p in enumerate(OLD_POSES)]
    box = [on_box(with_box, empty, p) for p in OLD_POSES]
    n_box, n_wall = sum(int(b.sum()) for b in box), sum(int((~b).sum()) for b in box)
    assert n_box >= 100 and n_wall >= 1900 and all(b.sum() >= 8 for b in box)
    held = [(s, S.pose_of(s)) for s in olds]
    for scene, gone in ((empty, True), (with_box, False)):
        news = [room_scan(scene, p, 600 + i) for i, p in enumerate(NEW_POSES)]
        viewers = [(s, S.pose_of(s)) for s in news]
        assert S.distance_to_half(held + viewers, ROOM_ANCHOR, ROOM_RES) > S.HALF_GUARD
        for protect in (1, 2):
            for n_viewers in (1, 2):
                inside, seen, flags, _, rays = S.seen_through(ROOM_WINDOW, ROOM_ANCHOR, ROOM_RES, held, viewers[:n_viewers], 2, protect)
                f_box = sum(int((f & b).sum()) for f, b in zip(flags, box))
                f_wall = sum(int((f & ~b).sum()) for f, b in zip(flags, box))
                print("box %s, protect %d, %d viewer(s): %d of %d box readings and %d of %d wall readings flagged"
                      % ("gone" if gone else "still there", protect, n_viewers, f_box, n_box, f_wall, n_wall))
                assert rays == n_viewers * ROOM_BEAMS and inside.tolist() == [ROOM_BEAMS] * 6 and seen.sum() == f_box + f_wall
                if gone and n_viewers == 2:
                    assert (f_box, f_wall) == (n_box, 0)
                if gone:
                    assert f_box >= 0.85 * n_box
                if not gone:
                    assert f_box <= 0.06 * n_box  # (grazing rays along the box's faces)
