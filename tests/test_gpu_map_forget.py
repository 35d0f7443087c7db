"""Maps that forget, on the device: `ym_map_create_counted`, `ym_map_update_scans`, the counts behind them,
`CorrelationMap.remove_scans` / `sync` / `update_scans` and the windowed `MapBuilder`.

The yardstick is tests/mapgrow_ref.py, the sequential restatement of the reference's add_scan_to_grid loop: after any sequence of
adds, removes and moves the map must be `mapgrow_ref.build` of the scans that remain, at the poses they were added at (the same
nonzero cells, 1e-15 on values because of `exp`: the tolerance and the reason of tests/test_gpu_map_grow.py), its counts
`np.add.at` on the restatement's cells, and on the device it must equal bit for bit a fresh counted map that received just those
scans, an uncounted map that received them, and `correlation_grid_from_occupancy` of the image `stamps > 0`.  `_check` asserts all
of it.  Every fixture asserts on the CPU that no quotient (x - ox) / res lies within 1e-6 of a rounding tie.

Every case runs with both configurations of tests/test_gpu_map_grow.py: 5 x 5 taps in a 70 x 45 map and 29 x 29 taps in a
130 x 67 map (where the box a removal recomputes spans several gather tiles both ways); the room walk keeps that file's own map."""
import ctypes as C
import math

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from tests import mapforget_ref as F  # noqa: E402
from tests import mapgrow_ref as R  # noqa: E402
from tests.test_gpu_map_grow import (CONFIGS, FAR, INC, MIN_ANGLE, N_BEAMS, WALK_MIN_RESPONSE, WALK_RES,  # noqa: E402
                                     _border_scan, _guard, _scan, _walk)

TILE_W, TILE_H = 64, 4  # map_forget_gather_kernel's tile (kMfTileW x kMfTileH), anchored at multiples of itself in map cells


def _tf(p):
    return (p.x, p.y, p.euler[-1])


def _clone(s, pose=None):
    return _scan(s.ranges, _tf(s.corrected_pose) if pose is None else pose)


class _Ctx(object):
    pass


@pytest.fixture(scope="module", params=CONFIGS, ids=[c[0] for c in CONFIGS])
def ctx(request):
    """a matcher and the three overlapping 91-beam scans of tests/test_gpu_map_grow.py's fixture (most readings inside the map,
    some beyond the nearer sides)"""
    from yag_slam_amd.scan_matching import ScanMatcher
    name, res, smear, taps, w, h = request.param
    c = _Ctx()
    c.name, c.res, c.taps, c.w, c.h = name, res, taps, w, h
    c.m = ScanMatcher(dict(resolution=res, smear_deviation=smear, range_threshold=12.0), semantics="yagpy")
    c.kernel = R.calculate_kernel(res, smear)
    assert c.kernel.shape == (taps, taps)
    c.ox, c.oy = -0.513 * res / 0.05, 0.237 * res / 0.05
    c.cx, c.cy = c.ox + 0.5 * w * res, c.oy + 0.5 * h * res
    rng = np.random.default_rng(11)
    c.ranges, c.poses = [], []
    for dx, dy, th in [(-6.3, 1.2, 0.3), (2.1, -3.4, 1.7), (7.7, 4.6, -2.2)]:
        r = rng.uniform(4.0, 0.7 * h, N_BEAMS) * res
        r[rng.permutation(N_BEAMS)[:5]] = [FAR, np.nan, FAR, np.inf, FAR]
        c.ranges.append(r)
        c.poses.append((c.cx + dx * res, c.cy + dy * res, th))
    yield c
    c.m.close()


def _abc(c):
    """fresh scan objects (a scan remembers nothing of the maps of other tests)"""
    scans = [_scan(r, p) for r, p in zip(c.ranges, c.poses)]
    _guard(scans, c.ox, c.oy, c.res)
    return scans


def _counted(c):
    return c.m.empty_correlation_map(c.w, c.h, counted=True, ox=c.ox, oy=c.oy)


def _assert_equals_restatement(got, want):
    assert got.shape == want.shape
    assert np.array_equal(got != 0, want != 0), np.argwhere((got != 0) != (want != 0))[:5]
    assert np.abs(got - want).max() <= 1e-15


def _check(c, cm, held):
    """`cm` against every form of the map of `held` (scans whose CURRENT pose is the one they are in the map at); returns the
    restated grid"""
    _guard(held, c.ox, c.oy, c.res)
    want, (_, _, _, cells) = R.build((c.h, c.w), c.kernel, held, c.ox, c.oy, c.res)
    got, stamps = cm.to_numpy(), cm.stamps()
    _assert_equals_restatement(got, want)
    assert stamps.dtype == np.uint32 and np.array_equal(stamps.astype(np.int64), F.counts_of((c.h, c.w), cells))
    twins = [_clone(s) for s in held]
    fresh = _counted(c)
    fresh.add_scans(c.ox, c.oy, twins)
    assert np.array_equal(got, fresh.to_numpy()) and np.array_equal(stamps, fresh.stamps())
    fresh.close()
    plain = c.m.empty_correlation_map(c.w, c.h)
    plain.add_scans(c.ox, c.oy, twins)
    assert np.array_equal(got, plain.to_numpy())
    plain.close()
    occ = c.m.correlation_grid_from_occupancy(np.where(stamps > 0, 0, 255).astype(np.uint8), occupied_value=0)
    assert np.array_equal(got, occ.to_numpy())
    occ.close()
    return want


def _coarse(c):
    return dict(grid_resolution=c.res)


def _key(r):
    return (r.response, r.covariance, r.meta["corrected_centre"], r.meta["coarse_response"], r.meta["n_query_points"],
            [(p.x, p.y, p.euler[-1]) for p in r.best_pose])


def _assert_matches_equal_the_restated_grid(c, cm, want):
    """what scoring reads followed the removal: `match_scan_sets_with_map`, `match_map_batch` and `track_in_map` on the resident map
    against the same calls on an upload of the restated grid"""
    twin = c.m.upload_correlation_grid(want)
    p0, p1, p2 = c.poses
    q = _scan(c.ranges[0], (p0[0] + 2.3 * c.res, p0[1] - 1.4 * c.res, p0[2] + 0.02))
    a = c.m.match_scan_sets_with_map(cm, c.ox, c.oy, [q], True, True, coarse=_coarse(c))
    b = c.m.match_scan_sets_with_map(twin, c.ox, c.oy, [q], True, True, coarse=_coarse(c))
    assert _key(a) == _key(b), (_key(a), _key(b))
    sets = [[q], [_scan(c.ranges[1], p1), _scan(c.ranges[2], p2)]]
    ra = c.m.match_map_batch(cm, c.ox, c.oy, sets, True, True, coarse=_coarse(c))
    rb = c.m.match_map_batch(twin, c.ox, c.oy, sets, True, True, coarse=_coarse(c))
    assert [_key(r) for r in ra] == [_key(r) for r in rb]
    out = []
    for mp in (cm, twin):
        track = [_scan(c.ranges[2], p2), _scan(c.ranges[2], p2, odom=(p2[0] + 1.7 * c.res, p2[1] + 0.9 * c.res, p2[2] - 0.015))]
        res, done = c.m.track_in_map(mp, c.ox, c.oy, track, 1, True, True, _coarse(c), 0.0)
        assert done == 2
        out.append((res[1].response, res[1].covariance, _tf(res[1].best_pose), res[1].meta["accepted"], _tf(track[1].corrected_pose)))
    assert out[0] == out[1]
    twin.close()
    return a.response


def _assert_blank(c, cm):
    assert not cm.to_numpy().any() and not cm.stamps().any() and len(cm) == 0
    q = _scan(c.ranges[0], c.poses[0])
    assert c.m.match_scan_sets_with_map(cm, c.ox, c.oy, [q], True, True, coarse=_coarse(c)).response == 0.0  # (the bytes too)


def _changed_inside(st, before, after):
    ys, xs = np.nonzero(before != after)
    if len(ys):
        assert st.x0 <= xs.min() and xs.max() < st.x1 and st.y0 <= ys.min() and ys.max() < st.y1, (st, xs.min(), xs.max(), ys.min(), ys.max())


# ---- 1: three scans in, the middle one out, then the rest ---------------------------------------------------------------------
def test_removing_one_of_three_leaves_the_map_of_the_other_two_and_removing_all_leaves_zeros(ctx):
    c = ctx
    a, b, s3 = _abc(c)
    cm = _counted(c)
    assert cm.counted and cm.origin == (c.ox, c.oy) and len(cm) == 0 and cm.revision == 0
    cm.add_scans(c.ox, c.oy, [a, b, s3])
    assert len(cm) == 3 and cm.revision == 1
    want = _check(c, cm, [a, b, s3])
    assert _assert_matches_equal_the_restated_grid(c, cm, want) > 0.0
    before = cm.to_numpy()
    n_b = len(F.cells_of([b], (c.h, c.w), c.ox, c.oy, c.res))
    st = cm.remove_scans([b])
    assert (st.removed, st.added, st.unmatched, st.gained) == (n_b, 0, 0, 0) and st.released > 0 and st.dropped == N_BEAMS - 5 - n_b
    assert b not in cm and a in cm and len(cm) == 2 and cm.revision == 2
    want = _check(c, cm, [a, s3])
    _changed_inside(st, before, cm.to_numpy())
    assert 0 <= st.x0 < st.x1 <= c.w and 0 <= st.y0 < st.y1 <= c.h
    _assert_matches_equal_the_restated_grid(c, cm, want)
    cm.remove_scans([s3, a])
    _assert_blank(c, cm)
    cm.add_scans(c.ox, c.oy, [a])  # the emptied map is a map like any other, and equal to a cleared one
    cm.clear()
    _assert_blank(c, cm)
    cm.close()


# ---- 2, 8: single readings placed by hand -------------------------------------------------------------------------------------
def _reading_at(c, gx, gy):
    """a scan whose one reading lands 0.2 cells off the centre of cell (gx, gy)"""
    r0 = 0.3 * c.res / 0.05
    s = _scan([r0] + [FAR] * 7, (c.ox + (gx + 0.2) * c.res - r0 * math.cos(MIN_ANGLE), c.oy + (gy - 0.2) * c.res - r0 * math.sin(MIN_ANGLE), 0.0))
    _guard([s], c.ox, c.oy, c.res)
    assert F.cells_of([s], (c.h, c.w), c.ox, c.oy, c.res) == [(gx, gy)]
    return s


def test_a_released_cell_within_reach_of_a_survivor_keeps_the_survivors_taps(ctx):
    c = ctx
    half = c.taps // 2
    gx, gy = 31, 22
    gone, stay = _reading_at(c, gx, gy), _reading_at(c, gx + half, gy)  # `half` cells apart: every cell between is in reach of both
    cm = _counted(c)
    cm.add_scans(c.ox, c.oy, [gone, stay])
    both = cm.to_numpy()
    st = cm.remove_scans([gone])
    assert (st.removed, st.released, st.unmatched) == (1, 1, 0)
    got = cm.to_numpy()
    k = c.kernel
    mid = gx + half // 2 + 1  # nearer to the survivor than to the released cell: its value was the survivor's tap and stays so
    assert both[gy, mid] == got[gy, mid] and abs(got[gy, mid] - k[half, half - (gx + half - mid)]) <= 1e-15 and got[gy, mid] > 0
    assert both[gy, gx] == 1.0 and abs(got[gy, gx] - k[half, 0]) <= 1e-15 and 0 < got[gy, gx] < 1.0  # the released cell: the survivor's outermost tap
    # above it: down from the released cell's nearest tap to a tap of the survivor's outermost column
    assert both[gy + 1, gx] > got[gy + 1, gx] > 0 and abs(got[gy + 1, gx] - k[half + 1, 0]) <= 1e-15
    assert both[gy, gx - 1] > 0 and got[gy, gx - 1] == 0.0 and got[gy, gx + half] == 1.0  # out of the survivor's reach: zero
    _check(c, cm, [stay])
    assert (st.x0, st.y0, st.x1, st.y1) == (gx - half, gy - half, gx + half + 1, gy + half + 1)
    cm.close()


def test_released_cells_on_the_edges_and_corners_of_a_gather_tile(ctx):
    """The gather's tiles are 64 x 4 cells (TILE_W x TILE_H) and start at multiples of that in map cells: (63, 3) is the last cell
    of tile (0, 0), (64, 4) the first of tile (1, 1) -- the two corners that meet --, (64, 23) lies on a tile's left edge in its
    last row, (40, 7) in a last row, (63, 20) on a right edge in a first row."""
    c = ctx
    assert (TILE_W, TILE_H) == (64, 4) and c.w > 66
    spots = [(63, 3), (64, 4), (64, 23), (40, 7), (63, 20)]
    for x, y in spots[:2]:
        assert (x % TILE_W, y % TILE_H) in ((TILE_W - 1, TILE_H - 1), (0, 0))
    gone = [_reading_at(c, x, y) for x, y in spots]
    stay = [_reading_at(c, 66, 6), _reading_at(c, 50, 21)]
    cm = _counted(c)
    cm.add_scans(c.ox, c.oy, gone + stay)
    _check(c, cm, gone + stay)
    for i in range(len(gone)):  # one at a time: each box is that cell's reach alone
        st = cm.remove_scans([gone[i]])
        assert (st.removed, st.released, st.unmatched) == (1, 1, 0)
        _check(c, cm, gone[i + 1:] + stay)
    cm.add_scans(c.ox, c.oy, gone)
    st = cm.remove_scans(gone)  # and all in one call
    assert (st.removed, st.released) == (len(gone), len(gone))
    _check(c, cm, stay)
    cm.close()


# ---- 3: a cell two scans share ------------------------------------------------------------------------------------------------
def test_the_same_readings_twice_halve_the_counts_and_change_no_cell_when_one_goes(ctx):
    c = ctx
    one, two = _scan(c.ranges[0], c.poses[0]), _scan(c.ranges[0], c.poses[0])
    cm = _counted(c)
    cm.add_scans(c.ox, c.oy, [one])
    single, single_counts = cm.to_numpy(), cm.stamps()
    st = cm.add_scans(c.ox, c.oy, [two])
    assert st.stamped == single_counts.sum() and np.array_equal(cm.to_numpy(), single) and np.array_equal(cm.stamps(), 2 * single_counts)
    st = cm.remove_scans([one])
    assert (st.removed, st.released, st.unmatched) == (int(single_counts.sum()), 0, 0) and (st.x0, st.y0, st.x1, st.y1) == (0, 0, 0, 0)
    assert np.array_equal(cm.to_numpy(), single) and np.array_equal(cm.stamps(), single_counts)
    _check(c, cm, [two])
    st = cm.remove_scans([two])
    assert st.released == np.count_nonzero(single_counts)
    _assert_blank(c, cm)
    cm.close()


# ---- 4: many readings of one scan in one cell ---------------------------------------------------------------------------------
def test_a_count_above_one_goes_to_zero_in_one_call(ctx):
    """a scan facing a wall six cells away: neighbouring beams end 0.3 cells apart, three to a cell"""
    c = ctx
    rel = MIN_ANGLE + np.arange(N_BEAMS) * INC
    r = np.where(np.abs(rel) < 1.2, 6.0 * c.res / np.cos(np.clip(rel, -1.2, 1.2)), FAR)
    s = _scan(r, (c.ox + 30.3 * c.res, c.oy + 20.2 * c.res, 0.0))
    other = _reading_at(c, 38, 21)
    cm = _counted(c)
    cm.add_scans(c.ox, c.oy, [s, other])
    _check(c, cm, [s, other])
    counts = cm.stamps()
    assert counts.max() >= 3 and counts.sum() == 45 + 1
    st = cm.remove_scans([s])
    assert (st.removed, st.unmatched) == (45, 0) and st.released == np.count_nonzero(counts) - 1 < 45
    _check(c, cm, [other])
    cm.remove_scans([other])
    _assert_blank(c, cm)
    cm.close()


# ---- 5: the pose of the add, not the current one ------------------------------------------------------------------------------
def test_a_scan_is_removed_at_the_pose_it_was_added_at(ctx):
    c = ctx
    a, b, _ = _abc(c)
    cm = _counted(c)
    cm.add_scans(c.ox, c.oy, [a, b])
    p = a.corrected_pose
    a.corrected_pose = type(p)(p.x + 7.3 * c.res, p.y - 4.1 * c.res, 0.0, p.euler[-1] + 0.4)
    assert cm.moved_scans() == [a]
    st = cm.remove_scans([a])
    assert st.unmatched == 0 and st.removed == len(F.cells_of([_scan(c.ranges[0], c.poses[0])], (c.h, c.w), c.ox, c.oy, c.res))
    want = _check(c, cm, [b])
    _assert_matches_equal_the_restated_grid(c, cm, want)
    cm.add_scans(c.ox, c.oy, [a])  # back in, where it is now
    _check(c, cm, [a, b])
    cm.close()


# ---- 6: sync ------------------------------------------------------------------------------------------------------------------
def test_sync_moves_what_moved_and_nothing_else(ctx):
    c = ctx
    a, b, s3 = _abc(c)
    rng = np.random.default_rng(5)
    d = _scan(rng.uniform(4.0, 0.4 * c.h, N_BEAMS) * c.res, (c.cx + 3.3 * c.res, c.cy - 2.6 * c.res, 0.9))
    e = _scan(rng.uniform(4.0, 0.4 * c.h, N_BEAMS) * c.res, (c.cx - 9.4 * c.res, c.cy + 1.7 * c.res, -0.6))
    cm = _counted(c)
    cm.add_scans(c.ox, c.oy, [a, b, s3, d, e])
    _check(c, cm, [a, b, s3, d, e])
    assert cm.sync().removed == 0 and cm.revision == 1  # nothing moved: nothing done
    tf = type(a.corrected_pose)
    a.corrected_pose = tf(c.poses[0][0] + 3.7 * c.res, c.poses[0][1] - 2.2 * c.res, 0.0, c.poses[0][2] + 0.11)
    pd, pe = d.corrected_pose, e.corrected_pose
    d.corrected_pose = tf(pd.x + 40.0 * c.w * c.res, pd.y, 0.0, pd.euler[-1])  # every reading of d leaves the map
    e_cells = F.cells_of([e], (c.h, c.w), c.ox, c.oy, c.res)
    e.corrected_pose = tf(pe.x + 1e-4 * c.res, pe.y - 1e-4 * c.res, 0.0, pe.euler[-1])  # less than a cell: the same cells again
    assert F.cells_of([e], (c.h, c.w), c.ox, c.oy, c.res) == e_cells and len(e_cells) > 20
    assert F.cells_of([d], (c.h, c.w), c.ox, c.oy, c.res) == []
    assert set(map(id, cm.moved_scans())) == {id(a), id(d), id(e)}
    before = cm.to_numpy()
    st = cm.sync()
    assert st.unmatched == 0 and st.dropped >= N_BEAMS and cm.revision == 2 and cm.moved_scans() == [] and len(cm) == 5
    want = _check(c, cm, [a, b, s3, d, e])
    _changed_inside(st, before, cm.to_numpy())
    _assert_matches_equal_the_restated_grid(c, cm, want)
    # a list names the scans to look at: b has moved too, but only s3 is asked about
    b.corrected_pose = tf(c.poses[1][0] - 2.9 * c.res, c.poses[1][1] + 1.3 * c.res, 0.0, c.poses[1][2])
    s3.corrected_pose = tf(c.poses[2][0] + 1.9 * c.res, c.poses[2][1] + 2.3 * c.res, 0.0, c.poses[2][2] - 0.07)
    cm.sync([s3])
    want = _check(c, cm, [a, _scan(c.ranges[1], c.poses[1]), s3, d, e])
    _assert_matches_equal_the_restated_grid(c, cm, want)
    cm.sync()
    _check(c, cm, [a, b, s3, d, e])
    cm.close()


# ---- 7: the borders -----------------------------------------------------------------------------------------------------------
def test_removing_a_scan_that_touches_every_border_a_corner_and_cells_beyond_every_side(ctx):
    c = ctx
    s = _border_scan(c)  # even beams on the four borders, beam 41 on the corner cell (w - 1, h - 1), odd beams beyond every side
    a = _abc(c)[0]
    cells = F.cells_of([s], (c.h, c.w), c.ox, c.oy, c.res)
    xs, ys = {x for x, _ in cells}, {y for _, y in cells}
    assert 0 in xs and c.w - 1 in xs and 0 in ys and c.h - 1 in ys and (c.w - 1, c.h - 1) in cells and len(cells) == 47
    cm = _counted(c)
    cm.add_scans(c.ox, c.oy, [a, s])
    _check(c, cm, [a, s])
    st = cm.remove_scans([s])
    assert (st.removed, st.dropped, st.unmatched) == (47, 44, 0)  # the readings beyond the map decrement nothing
    assert (st.x0, st.y0, st.x1, st.y1) == (0, 0, c.w, c.h)
    _check(c, cm, [a])  # (a recompute past a row's end would show in the next row)
    cm.add_scans(c.ox, c.oy, [s])
    cm.remove_scans([a])
    _check(c, cm, [s])
    cm.remove_scans([s])
    _assert_blank(c, cm)
    cm.close()


# ---- 9: more scans than a chunk -----------------------------------------------------------------------------------------------
def test_one_call_with_more_scans_than_a_chunk(ctx):
    """4097 scans of 8 beams (a launch takes 4096): all added in one call, every other one removed in one call.  The scans stand on
    a 17 x 15 lattice of poses and reach 5 to 9 cells, so they share a few hundred cells and the restated map is quick."""
    from yag_slam_amd import models
    c = ctx
    rng = np.random.default_rng(23)
    n = 4097
    scans = []
    for i in range(n):
        px, py = c.cx + ((i % 17) - 8.0 + 0.37) * 0.9 * c.res, c.cy + ((i // 17 % 15) - 7.0 + 0.29) * 0.9 * c.res
        scans.append(_scan(rng.uniform(5.0, 9.0, 8) * c.res, (px, py, 0.7 * (i % 9))))
    _guard(scans, c.ox, c.oy, c.res)
    models.native_many(scans, c.m.device)
    cells = [F.cells_of([s], (c.h, c.w), c.ox, c.oy, c.res) for s in scans]
    assert all(len(v) == 8 for v in cells)
    cm = _counted(c)
    st = cm.add_scans(c.ox, c.oy, scans)
    assert (st.points, st.stamped, st.dropped) == (8 * n, 8 * n, 0) and len(cm) == n
    counts = F.counts_of((c.h, c.w), [x for v in cells for x in v])
    assert np.array_equal(cm.stamps().astype(np.int64), counts) and np.count_nonzero(counts) < 1500
    _assert_equals_restatement(cm.to_numpy(), F.from_counts(counts, c.kernel))
    st = cm.remove_scans(scans[1::2])
    assert (st.removed, st.unmatched, st.dropped) == (8 * (n // 2), 0, 0) and len(cm) == n - n // 2
    rest = F.counts_of((c.h, c.w), [x for v in cells[0::2] for x in v])
    assert st.released == np.count_nonzero((counts > 0) & (rest == 0))
    got, stamps = cm.to_numpy(), cm.stamps()
    assert np.array_equal(stamps.astype(np.int64), rest)
    _assert_equals_restatement(got, F.from_counts(rest, c.kernel))
    twins = [_clone(s) for s in scans[0::2]]
    models.native_many(twins, c.m.device)
    fresh = _counted(c)
    fresh.add_scans(c.ox, c.oy, twins)
    assert np.array_equal(got, fresh.to_numpy()) and np.array_equal(stamps, fresh.stamps())
    fresh.close()
    plain = c.m.empty_correlation_map(c.w, c.h)
    plain.add_scans(c.ox, c.oy, scans[0::2])  # (an uncounted map holds no scans: the same objects will do)
    assert np.array_equal(got, plain.to_numpy())
    plain.close()
    occ = c.m.correlation_grid_from_occupancy(np.where(stamps > 0, 0, 255).astype(np.uint8), occupied_value=0)
    assert np.array_equal(got, occ.to_numpy())
    occ.close()
    cm.remove_scans(scans[0::2])
    _assert_blank(c, cm)
    cm.close()


# ---- 11: through ctypes -------------------------------------------------------------------------------------------------------
def test_the_library_counts_what_does_not_match_and_refuses_what_it_must(ctx):
    from yag_slam_amd import _capi
    c = ctx
    L = c.m._lib
    a, b, _ = _abc(c)
    cm = _counted(c)
    assert L.ym_map_counted(cm._h) == 1
    cm.add_scans(c.ox, c.oy, [a])
    counts = cm.stamps().astype(np.int64)
    # a out at a pose half a cell from where it went in: some readings meet cells of a, the others a count of zero
    wrong_pose = (c.poses[0][0] + 0.6 * c.res, c.poses[0][1] + 0.3 * c.res, c.poses[0][2])
    wrong = _scan(c.ranges[0], wrong_pose)
    _guard([wrong], c.ox, c.oy, c.res)
    wrong_counts = F.counts_of((c.h, c.w), F.cells_of([wrong], (c.h, c.w), c.ox, c.oy, c.res))
    want_unmatched = int(np.maximum(wrong_counts - counts, 0).sum())
    want_counts = np.maximum(counts - wrong_counts, 0)
    assert want_unmatched > 20 and int(wrong_counts.sum()) - want_unmatched > 20
    hs = (C.c_void_p * 1)(c.m._require_native(a))
    st = _capi.YmMapUpdateStats()
    assert L.ym_map_update_scans(c.m._m, cm._h, hs, (C.c_double * 3)(*wrong_pose), 1, None, 0, C.byref(st)) == 0
    assert st.unmatched == want_unmatched and st.removed == int(wrong_counts.sum()) - want_unmatched and st.added == 0
    stamps = cm.stamps()
    assert np.array_equal(stamps.astype(np.int64), want_counts) and stamps.max() < 2 ** 31  # no count went below zero
    assert st.released == np.count_nonzero((counts > 0) & (want_counts == 0))
    got = cm.to_numpy()
    occ = c.m.correlation_grid_from_occupancy(np.where(stamps > 0, 0, 255).astype(np.uint8), occupied_value=0)
    assert np.array_equal(got, occ.to_numpy())  # the map is still a function of its counts
    occ.close()
    _assert_equals_restatement(got, F.from_counts(want_counts, c.kernel))
    # a foreign origin is refused and nothing changes
    hb = (C.c_void_p * 1)(c.m._require_native(b))
    for ox, oy in ((c.ox + c.res, c.oy), (c.ox, float("nan"))):
        assert L.ym_map_add_scans(c.m._m, cm._h, ox, oy, hb, 1, None) == -1 and "origin" in _capi.last_error()
    assert np.array_equal(cm.stamps(), stamps) and np.array_equal(cm.to_numpy(), got)
    # a null scan in either list, before anything changes
    two = (C.c_void_p * 2)(c.m._require_native(b), None)
    assert L.ym_map_update_scans(c.m._m, cm._h, None, None, 0, two, 2, None) == -1 and "scan 1" in _capi.last_error()
    assert L.ym_map_update_scans(c.m._m, cm._h, two, (C.c_double * 6)(), 2, hb, 1, None) == -1 and "scan 1" in _capi.last_error()
    assert np.array_equal(cm.stamps(), stamps) and np.array_equal(cm.to_numpy(), got)
    # a map without counts cannot forget, and is left as it is: the float grid and what scoring reads
    plain = c.m.empty_correlation_map(c.w, c.h)
    assert L.ym_map_counted(plain._h) == 0 and not plain.counted and plain.origin is None
    plain.add_scans(c.ox, c.oy, [b])
    grid = plain.to_numpy()
    q = _scan(c.ranges[1], c.poses[1])
    key = _key(c.m.match_scan_sets_with_map(plain, c.ox, c.oy, [q], True, True, coarse=_coarse(c)))
    assert L.ym_map_update_scans(c.m._m, plain._h, hb, (C.c_double * 3)(*c.poses[1]), 1, None, 0, C.byref(st)) == -4
    assert "counts" in _capi.last_error()
    buf = (C.c_uint32 * (c.w * c.h))()
    assert L.ym_map_read_stamps(plain._h, buf, c.w * c.h) == -4
    assert L.ym_map_read_stamps(cm._h, buf, c.w * c.h - 1) == -1
    assert np.array_equal(plain.to_numpy(), grid)
    assert _key(c.m.match_scan_sets_with_map(plain, c.ox, c.oy, [q], True, True, coarse=_coarse(c))) == key
    with pytest.raises(ValueError, match="keeps no counts"):
        plain.remove_scans([b])
    # a matcher of the other semantics
    from yag_slam_amd.scan_matching import ScanMatcher
    karto = ScanMatcher(dict(resolution=0.05, smear_deviation=0.05, search_size=0.3), semantics="karto")
    assert not karto._lib.ym_map_create_counted(karto._m, c.w, c.h, c.ox, c.oy) and "YM_SEM_YAGPY" in _capi.last_error()
    assert karto._lib.ym_map_update_scans(karto._m, cm._h, None, None, 0, hb, 1, None) == -4 and "YM_SEM_YAGPY" in _capi.last_error()
    assert np.array_equal(cm.stamps(), stamps)
    karto.close()
    plain.close()
    cm.close()


# ---- 12: revision and the locator rule ----------------------------------------------------------------------------------------
def test_a_locator_made_before_a_removal_refuses_and_one_made_after_it_locates(ctx):
    c = ctx
    a, b, s3 = _abc(c)
    cm = _counted(c)
    cm.add_scans(c.ox, c.oy, [a, b, s3])
    q = _scan(c.ranges[0], c.poses[0])
    with c.m.map_locator(cm, levels=2) as old:
        assert len(old.locate([q], c.ox, c.oy, n_angles=8)) >= 1
        cm.sync()  # nothing moved: the map and its revision stay, and so does the locator
        assert cm.revision == 1 and len(old.locate([q], c.ox, c.oy, n_angles=8)) >= 1
        cm.remove_scans([b])
        assert cm.revision == 2
        with pytest.raises(ValueError, match="make a new locator"):
            old.locate([q], c.ox, c.oy, n_angles=8)
    with c.m.map_locator(cm, levels=2) as new:
        cands = new.locate([q], c.ox, c.oy, n_angles=8)
        assert len(cands) >= 1 and cands[0].response > 0
        assert np.array_equal(new.read_level(0), (100 * cm.to_numpy()).astype(np.uint8))
    cm.close()


# ---- 13: the windowed MapBuilder on the room walk -----------------------------------------------------------------------------
def test_windowed_map_builder_keeps_four_keyframes_and_the_map_of_exactly_those():
    """tests/test_gpu_map_grow.py's 31-scan walk through the room (its own map: 187 x 141 cells of 0.05 m, 5 x 5 taps), once with
    window=4 and once without.  No accuracy bound: nothing in the code yields one for a windowed map; the final errors and `lost`
    are printed."""
    from yag_slam_amd.mapping import MapBuilder
    from yag_slam_amd.scan_matching import ScanMatcher
    res, ox, oy, w, h = WALK_RES, -0.613, -0.437, 187, 141
    m = ScanMatcher(dict(resolution=res, smear_deviation=0.05, range_threshold=12.0), semantics="yagpy")
    kernel = R.calculate_kernel(res, 0.05)
    truth, scans = _walk()
    _, plain_scans = _walk()
    cm = m.empty_correlation_map(w, h, counted=True, ox=ox, oy=oy)
    plain_map = m.empty_correlation_map(w, h)
    kw = dict(min_response=WALK_MIN_RESPONSE, min_distance=0.2, min_rotation=0.1)
    b, u = MapBuilder(m, cm, ox, oy, window=4, **kw), MapBuilder(m, plain_map, ox, oy, **kw)
    same_until = None  # the first step at which the two builders' poses differ
    for i, (s, t) in enumerate(zip(scans, plain_scans)):
        b.process_scan(s)
        u.process_scan(t)
        if same_until is None and _tf(s.corrected_pose) != _tf(t.corrected_pose):
            same_until = i
        if same_until is None:
            keys = [scans.index(x) for x in b.dropped + b.added]
            assert keys == [plain_scans.index(x) for x in u.added], i
        assert len(b.added) <= 4 and len(cm) == len(b.added) and all(x in cm for x in b.added) and not any(x in cm for x in b.dropped)
        _guard(b.added, ox, oy, res)
        want, (_, _, _, cells) = R.build((h, w), kernel, b.added, ox, oy, res)
        _assert_equals_restatement(cm.to_numpy(), want)
        assert np.array_equal(cm.stamps().astype(np.int64), F.counts_of((h, w), cells))
    assert len(b.added) == 4 and len(b.dropped) >= 1 and b.dropped + b.added == sorted(b.dropped + b.added, key=scans.index)
    assert same_until is None or same_until > 4  # (the window is full after four keyframes: nothing can differ before)
    assert isinstance(b.lost, int) and b.lost >= 0 and len(b.results) == len(scans) - 1
    err = [math.hypot(x[-1].corrected_pose.x - truth[-1][0], x[-1].corrected_pose.y - truth[-1][1]) for x in (scans, plain_scans)]
    print("window=4: %d keyframes, %d dropped, lost %d, final error %.4f m; unwindowed: %d keyframes, lost %d, final error %.4f m; "
          "poses equal until step %s" % (len(b.added) + len(b.dropped), len(b.dropped), b.lost, err[0], len(u.added), u.lost, err[1], same_until))
    # rebuild after a perturbation equals clear-and-add, bit for bit, by either route: the moved scans moved (a share of 1 allows
    # every rebuild to), the map cleared and filled (a share of 0 allows none), and the builder's own choice
    tf = type(scans[0].corrected_pose)
    for moved, share in ((b.added[1:2], 1.0), (b.added, 1.0), (b.added[2:], 0.0), (b.added[:1], MapBuilder.REBUILD_SHARE)):
        b.REBUILD_SHARE = share
        for x in moved:
            p = x.corrected_pose
            x.corrected_pose = tf(p.x + 0.083, p.y - 0.061, 0.0, p.euler[-1] + 0.013)
        revision = cm.revision
        b.rebuild()
        assert cm.revision > revision and cm.moved_scans() == [] and len(cm) == 4
        fresh = m.empty_correlation_map(w, h)
        fresh.add_scans(ox, oy, b.added)
        assert np.array_equal(cm.to_numpy(), fresh.to_numpy())
        fresh.close()
        _guard(b.added, ox, oy, res)
        _assert_equals_restatement(cm.to_numpy(), R.build((h, w), kernel, b.added, ox, oy, res)[0])
    plain_map.close()
    cm.close()
    m.close()
