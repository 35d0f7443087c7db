"""Maps that notice change, on the device: `ym_map_seen_through`, `CorrelationMap.seen_through`,
`LocalizedRangeScan.blanked` and `MapBuilder(forget_seen_through=...)`.

The yardstick is tests/seenthrough_ref.py: counts, flags and the swept mask must equal the restatement exactly.  Both
configurations of tests/test_gpu_map_grow.py (70 x 45 cells of 0.05 m; 130 x 67 cells of 0.01 m, where a ray can be longer than 128
cells and a lane of the sweep takes three of them).  Every fixture asserts on the CPU that no reading's quotient and no sensor's
quotient lies within 1e-6 of a rounding tie, so a last-bit difference in the trigonometry cannot move a cell."""
import ctypes as C
import math

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from tests import mapgrow_ref as R  # noqa: E402
from tests import seenthrough_ref as S  # noqa: E402
from tests.test_gpu_map_grow import CONFIGS, FAR, MIN_ANGLE, N_BEAMS, _guard, _scan  # noqa: E402
from tests.test_seen_through_host import (BOX, OLD_POSES, ROOM_ANCHOR, ROOM_RES, ROOM_WINDOW, on_box, room_scan,  # noqa: E402
                                          room_scenes)

PAIRS = [(0, 0), (2, 1), (5, 3)]  # (clearance, protect)
HEADING = -MIN_ANGLE              # beam i of a scan with this heading points along i * INC: 0, 3, ... 270 degrees


def _tf(p):
    return (p.x, p.y, p.euler[-1])


def _clone(s):
    return _scan(s.ranges, _tf(s.corrected_pose))


def _guard_all(c, scans):
    """tests/test_gpu_map_grow.py's guard on the readings, and the same distance for the sensors' own quotients"""
    _guard(scans, c.ox, c.oy, c.res)
    assert S.distance_to_half([(s, S.pose_of(s)) for s in scans], (c.ox, c.oy), c.res) > S.HALF_GUARD, "a sensor lies on a tie"


def _pairs(scans):
    return [(s, S.pose_of(s)) for s in scans]


class _Ctx(object):
    pass


def fixture_on_the_cpu(config):
    """everything of the fixture that needs no device: the three held scans of tests/test_gpu_map_grow.py's fixture, a viewer
    near the centre and one near the left side, some of whose rays leave the window, and the restatement at (2, 1)"""
    name, res, smear, taps, w, h = config
    c = _Ctx()
    c.name, c.res, c.smear, c.taps, c.w, c.h = name, res, smear, taps, w, h
    c.ox, c.oy = -0.513 * res / 0.05, 0.237 * res / 0.05
    c.window, c.anchor = (0, 0, w, h), (c.ox, c.oy)
    c.cx, c.cy = c.ox + 0.5 * w * res, c.oy + 0.5 * h * res
    rng = np.random.default_rng(11)
    c.ranges, c.poses = [], []
    for dx, dy, th in [(-6.3, 1.2, 0.3), (2.1, -3.4, 1.7), (7.7, 4.6, -2.2)]:
        r = rng.uniform(4.0, 0.7 * h, N_BEAMS) * res
        r[rng.permutation(N_BEAMS)[:5]] = [FAR, np.nan, FAR, np.inf, FAR]
        c.ranges.append(r)
        c.poses.append((c.cx + dx * res, c.cy + dy * res, th))
    vrng = np.random.default_rng(23)
    c.view_ranges, c.view_poses = [], []
    for (px, py, th) in [(c.cx + 1.3 * res, c.cy - 0.7 * res, 0.9), (c.ox + 6.4 * res, c.cy + 3.3 * res, -0.5)]:
        r = vrng.uniform(6.0, 0.8 * h, N_BEAMS) * res
        r[vrng.permutation(N_BEAMS)[:3]] = [FAR, np.nan, np.inf]
        c.view_ranges.append(r)
        c.view_poses.append((px, py, th))
    held, viewers = held_scans(c), viewer_scans(c)
    _guard_all(c, held + viewers)
    ends = [e for v in viewers for e in S.beam_cells(v, S.pose_of(v), c.window, c.anchor, res) if e is not None]
    assert sum(1 for x, y in ends if not (0 <= x < w and 0 <= y < h)) >= 10, "too few viewer rays leave the window"
    inside, seen, flags, _, _ = S.seen_through(c.window, c.anchor, res, _pairs(held), _pairs(viewers), 2, 1)
    assert all(s >= 10 and i - s >= 10 for i, s in zip(inside, seen)), (inside, seen)
    return c


def held_scans(c):
    """fresh scan objects (a scan remembers nothing of the maps of other tests)"""
    return [_scan(r, p) for r, p in zip(c.ranges, c.poses)]


def viewer_scans(c):
    return [_scan(r, p) for r, p in zip(c.view_ranges, c.view_poses)]


@pytest.fixture(scope="module", params=CONFIGS, ids=[c[0] for c in CONFIGS])
def ctx(request):
    from yag_slam_amd.scan_matching import ScanMatcher
    c = fixture_on_the_cpu(request.param)
    c.m = ScanMatcher(dict(resolution=c.res, smear_deviation=c.smear, range_threshold=12.0), semantics="yagpy")
    yield c
    c.m.close()


def _counted(c, scans, window=None):
    cm = c.m.empty_correlation_map(c.w, c.h, counted=True, ox=c.ox, oy=c.oy, window=window)
    cm.add_scans(cm.origin[0], cm.origin[1], scans)
    return cm


def _assert_equals_restatement(c, cm, held, viewers, clearance, protect, window=None, scans=None):
    """counts, flags, mask and rays of the device against the restatement; `held`: (scan, the pose it was added at)"""
    window = c.window if window is None else window
    inside, seen, flags, mask, rays = S.seen_through(window, c.anchor, c.res, held, _pairs(viewers), clearance, protect)
    got = cm.seen_through(viewers, scans=scans, clearance=clearance, protect=protect, flags=True)
    assert [id(s) for s in got.scans] == [id(s) for s, _ in held]
    assert got.inside.tolist() == inside.tolist() and got.seen.tolist() == seen.tolist(), (got.inside, inside, got.seen, seen)
    assert len(got.flags) == len(flags)
    for g, f in zip(got.flags, flags):
        assert g.dtype == bool and np.array_equal(g, f), np.nonzero(g != f)[0][:5]
    plain = cm.seen_through(viewers, scans=scans, clearance=clearance, protect=protect)
    assert plain.flags is None and plain.inside.tolist() == inside.tolist() and plain.seen.tolist() == seen.tolist()
    got_mask, got_rays = cm.debug_swept_mask(viewers, clearance, protect)
    assert got_mask.shape == mask.shape and np.array_equal(got_mask, mask), np.argwhere(got_mask != mask)[:5]
    assert got_rays == rays
    return inside, seen, flags, mask


# ---- the mask, counts and flags of three held scans and two viewers -----------------------------------------------------------
@pytest.mark.parametrize("clearance,protect", PAIRS)
def test_mask_counts_and_flags_of_three_held_scans_equal_the_restatement(ctx, clearance, protect):
    c = ctx
    held, viewers = held_scans(c), viewer_scans(c)
    cm = _counted(c, held)
    _, seen, _, mask = _assert_equals_restatement(c, cm, _pairs(held), viewers, clearance, protect)
    assert mask.any() and seen.sum() > 0
    cm.close()


# ---- aimed rays ---------------------------------------------------------------------------------------------------------------
def _beams(c, sensor_cell, lengths, heading=HEADING):
    """a viewer standing 0.2 cells right of and 0.2 cells below the centre of `sensor_cell` whose beam i is lengths[i] cells long
    (the other beams see nothing)"""
    r = np.full(N_BEAMS, FAR)
    for i, cells in lengths.items():
        r[i] = cells * c.res
    return _scan(r, (c.ox + (sensor_cell[0] + 0.2) * c.res, c.oy + (sensor_cell[1] - 0.2) * c.res, heading))


def aimed_viewers(c):
    """The viewers of the aimed-ray case, with the CPU assertions that they are what they are meant to be."""
    w, h, s2 = c.w, c.h, math.sqrt(2.0)
    mx, my = w // 2 + 3, h // 2 - 2
    every = {i: 17.0 * (s2 if i % 30 == 15 else 1.0) for i in range(N_BEAMS)}  # the exact diagonals end on a diagonal cell
    out = dict(
        fan=_beams(c, (mx, my), every),                                   # 0 .. 270 degrees
        fan_back=_beams(c, (mx - 9, my + 4), every, HEADING + math.pi),   # 180 .. 450 degrees
        short=_beams(c, (12, 9), {0: 0.1, 7: 1.3, 30: 2.0, 52: 5.4}),     # dM = 0, 1, 2 and 5
        across=_beams(c, (0, h - 12), {0: w - 1.0}),                      # from the left border to the right one
        outside=_beams(c, (-7, my + 5), {0: 30.0, 3: 40.0, 87: 25.0, 60: 11.0}),  # a sensor outside the window looking in (and away)
        leaving=_beams(c, (mx + 2, 5), {0: 0.8 * w, 85: 30.0, 30: 2.0 * h}),      # a sensor inside, ends beyond three sides
        borders=_beams(c, (mx, my), {0: w - 1.0 - mx, 30: h - 1.0 - my, 60: float(mx), 90: float(my)}),  # ends ON each border
        overlong=_beams(c, (mx - 5, my + 7), {0: -40000.0, 30: 9.0}),     # a reading no sensor gives: 32768 steps or more
    )
    viewers = list(out.values())
    _guard_all(c, viewers)
    rel = []
    for v in (out["fan"], out["fan_back"]):
        sensor = S.cell(*S.pose_of(v)[:2], c.window, c.anchor, c.res)
        rel += [(e[0] - sensor[0], e[1] - sensor[1]) for e in S.beam_cells(v, S.pose_of(v), c.window, c.anchor, c.res) if e is not None]
    octants = {(dx > 0, dy > 0, abs(dy) > abs(dx)) for dx, dy in rel if dx and dy and abs(dx) != abs(dy)}
    assert len(octants) == 8
    for sign in (1, -1):
        assert (sign * 17, 0) in rel and (0, sign * 17) in rel                         # horizontal and vertical, both ways
        assert (sign * 17, sign * 17) in rel and (sign * 17, -sign * 17) in rel        # the exact diagonals
    cells = lambda v: [e for e in S.beam_cells(v, S.pose_of(v), c.window, c.anchor, c.res) if e is not None]  # noqa: E731
    sensor = lambda v: S.cell(*S.pose_of(v)[:2], c.window, c.anchor, c.res)  # noqa: E731
    d_major = lambda v: sorted(max(abs(e[0] - sensor(v)[0]), abs(e[1] - sensor(v)[1])) for e in cells(v))  # noqa: E731
    assert d_major(out["short"]) == [0, 1, 2, 5]
    assert sensor(out["across"]) == (0, h - 12) and cells(out["across"]) == [(w - 1, h - 12)] and (w <= 128 or d_major(out["across"])[0] > 128)
    assert sensor(out["outside"])[0] < 0 and sum(1 for x, y in cells(out["outside"]) if 0 <= x < w and 0 <= y < h) >= 2
    lx, ly = zip(*cells(out["leaving"]))
    assert 0 <= sensor(out["leaving"])[0] < w and max(lx) >= w and min(ly) < 0 and max(ly) >= h
    assert sorted(cells(out["borders"])) == sorted([(w - 1, my), (mx, h - 1), (0, my), (mx, 0)])
    assert d_major(out["overlong"]) == [9, 40000]
    return viewers


def test_aimed_rays_in_every_octant_over_the_borders_and_around_them(ctx):
    c = ctx
    held, viewers = held_scans(c), aimed_viewers(c)
    cm = _counted(c, held)
    for clearance, protect in PAIRS:
        _, _, _, mask = _assert_equals_restatement(c, cm, _pairs(held), viewers, clearance, protect)
        assert mask.any()
    # one viewer at a time too: another launch shape, and no other viewer's ends to hide a wrong cell
    for v in viewers:
        mask, rays = S.swept_mask(c.window, c.anchor, c.res, _pairs([v]), 2, 1)
        got_mask, got_rays = cm.debug_swept_mask([v], 2, 1)
        assert np.array_equal(got_mask, mask) and got_rays == rays
    cm.close()


# ---- the held pose, subsets, a held viewer, purity ----------------------------------------------------------------------------
def test_the_pose_a_scan_was_added_at_is_used_not_its_current_one(ctx):
    c = ctx
    held, viewers = held_scans(c), viewer_scans(c)
    cm = _counted(c, held)
    at = _pairs(held)
    before = cm.seen_through(viewers, flags=True)
    p = held[1].corrected_pose
    held[1].corrected_pose = type(p)(p.x + 7.3 * c.res, p.y - 4.1 * c.res, 0.0, p.euler[-1] + 0.4)  # (no sync)
    after = cm.seen_through(viewers, flags=True)
    assert before.inside.tolist() == after.inside.tolist() and before.seen.tolist() == after.seen.tolist()
    assert all(np.array_equal(a, b) for a, b in zip(before.flags, after.flags))
    _assert_equals_restatement(c, cm, at, viewers, 2, 1)
    # a viewer, though, is taken where it stands now
    moved = viewer_scans(c)
    q = moved[0].corrected_pose
    moved[0].corrected_pose = type(q)(q.x - 5.2 * c.res, q.y + 2.9 * c.res, 0.0, q.euler[-1] - 0.3)
    _guard_all(c, moved)
    _assert_equals_restatement(c, cm, at, moved, 2, 1)
    cm.close()


def test_a_subset_in_the_callers_order_a_held_viewer_and_a_scan_that_is_not_held(ctx):
    c = ctx
    held, viewers = held_scans(c), viewer_scans(c)
    cm = _counted(c, held)
    at = _pairs(held)
    _assert_equals_restatement(c, cm, [at[2], at[0]], viewers, 2, 1, scans=[held[2], held[0]])
    _assert_equals_restatement(c, cm, [], viewers, 2, 1, scans=[])
    # a held scan as a viewer, itself among the counted: no special case (its own end cells are protected, its rays sweep the rest)
    inside, seen, _, _ = _assert_equals_restatement(c, cm, at, [held[1]], 0, 0)
    assert seen[1] >= 0 and seen[0] + seen[2] > 0
    _assert_equals_restatement(c, cm, at, [held[1], viewers[0]], 2, 1)
    revision = cm.revision
    with pytest.raises(ValueError, match="not held"):
        cm.seen_through(viewers, scans=[held[0], viewers[0]])
    with pytest.raises(ValueError, match="twice"):
        cm.seen_through(viewers, scans=[held[0], held[0]])
    with pytest.raises(ValueError, match="clearance"):
        cm.seen_through(viewers, clearance=-1)
    with pytest.raises(ValueError, match="keeps no counts"):
        plain = c.m.empty_correlation_map(c.w, c.h)
        try:
            plain.seen_through(viewers)
        finally:
            plain.close()
    assert cm.revision == revision
    cm.close()


def test_the_call_changes_no_byte_of_the_map_its_counts_or_its_revision(ctx):
    c = ctx
    held, viewers = held_scans(c), viewer_scans(c) + aimed_viewers(c)
    cm = _counted(c, held)
    grid, stamps, revision = cm.to_numpy(), cm.stamps(), cm.revision
    for clearance, protect in PAIRS:
        cm.seen_through(viewers, clearance=clearance, protect=protect, flags=True)
        cm.debug_swept_mask(viewers, clearance, protect)
    assert np.array_equal(cm.to_numpy(), grid) and np.array_equal(cm.stamps(), stamps) and cm.revision == revision
    # what scoring reads is untouched too: the same match before and after
    twin = c.m.upload_correlation_grid(grid)
    q = _scan(c.ranges[0], (c.poses[0][0] + 2.3 * c.res, c.poses[0][1] - 1.4 * c.res, c.poses[0][2] + 0.02))
    a = c.m.match_scan_sets_with_map(cm, c.ox, c.oy, [q], True, True, coarse=dict(grid_resolution=c.res))
    b = c.m.match_scan_sets_with_map(twin, c.ox, c.oy, [q], True, True, coarse=dict(grid_resolution=c.res))
    assert (a.response, a.covariance, a.meta["corrected_centre"]) == (b.response, b.covariance, b.meta["corrected_centre"])
    # and the map still forgets exactly what it held
    cm.remove_scans(held)
    assert not cm.to_numpy().any() and not cm.stamps().any()
    twin.close()
    cm.close()


def test_after_a_reframe_counts_and_flags_equal_those_of_a_fresh_map_in_the_new_window(ctx):
    c = ctx
    held, viewers = held_scans(c), viewer_scans(c)
    cm = _counted(c, held)
    cm.reframe(13, -7)
    window = (13, -7, c.w, c.h)
    assert cm.window == window
    twins = [_clone(s) for s in held]
    fresh = _counted(c, twins, window=window[:2])
    assert fresh.window == window
    for clearance, protect in PAIRS[1:]:
        inside, seen, flags, _ = _assert_equals_restatement(c, cm, _pairs(held), viewers, clearance, protect, window=window)
        other = fresh.seen_through(viewers, clearance=clearance, protect=protect, flags=True)
        assert other.inside.tolist() == inside.tolist() and other.seen.tolist() == seen.tolist()
        assert all(np.array_equal(a, b) for a, b in zip(other.flags, flags))
        assert np.array_equal(fresh.debug_swept_mask(viewers, clearance, protect)[0], cm.debug_swept_mask(viewers, clearance, protect)[0])
    assert inside.sum() != S.seen_through(c.window, c.anchor, c.res, _pairs(held), _pairs(viewers), 5, 3)[0].sum()  # (the window matters)
    fresh.close()
    cm.close()


# ---- what the library refuses -------------------------------------------------------------------------------------------------
def test_refusals_through_the_raw_abi(ctx):
    from yag_slam_amd import _capi
    from yag_slam_amd.scan_matching import ScanMatcher
    c = ctx
    held, viewers = held_scans(c), viewer_scans(c)
    cm = _counted(c, held)
    lib = c.m._lib
    hs = (C.c_void_p * 3)(*[c.m._require_native(s) for s in held])
    vs = (C.c_void_p * 2)(*[c.m._require_native(s) for s in viewers])
    poses = np.array([S.pose_of(s) for s in held], dtype=np.float64)
    pp = poses.ctypes.data_as(C.POINTER(C.c_double))
    counts = np.full((3, 2), -5, dtype=np.int32)
    cp = counts.ctypes.data_as(C.POINTER(C.c_int32))

    def call(m=c.m, mp=cm, h=hs, n=3, v=vs, nv=2, clearance=2, protect=1, out=cp):
        return lib.ym_map_seen_through(m._m, mp._h, h, pp, n, v, nv, clearance, protect, out, None, None, None)

    assert call() == 0
    inside, seen, _, _, _ = S.seen_through(c.window, c.anchor, c.res, _pairs(held), _pairs(viewers), 2, 1)
    assert counts[:, 0].tolist() == inside.tolist() and counts[:, 1].tolist() == seen.tolist()
    plain = c.m.empty_correlation_map(c.w, c.h)
    assert call(mp=plain) == -4 and "counts" in _capi.last_error()
    plain.close()
    karto = ScanMatcher(dict(resolution=0.05, smear_deviation=0.05, search_size=0.3), semantics="karto")
    assert call(m=karto) == -4 and "YM_SEM_YAGPY" in _capi.last_error()
    karto.close()
    assert call(clearance=-1) == -1 and call(protect=-1) == -1 and call(n=-1) == -1 and call(nv=-1) == -1
    assert call(out=None) == -1 and call(h=None) == -1 and call(v=None) == -1
    null_held = (C.c_void_p * 3)(hs[0], None, hs[2])
    assert call(h=null_held) == -1 and "held scan 1" in _capi.last_error()
    null_viewer = (C.c_void_p * 2)(vs[0], None)
    assert call(v=null_viewer) == -1 and "viewer 1" in _capi.last_error()
    # a matcher whose range threshold reaches 32768 cells: the sweep's walk is 32-bit
    longm = ScanMatcher(dict(resolution=c.res, smear_deviation=c.smear, range_threshold=32766.5 * c.res), semantics="yagpy")
    assert call(m=longm) == -4 and "32768" in _capi.last_error()
    longm.close()
    # zero viewers: nothing is swept (the readings inside the window are still counted); zero held scans: nothing to count
    counts[:] = -5
    assert call(nv=0) == 0 and counts[:, 1].tolist() == [0, 0, 0] and counts[:, 0].tolist() == inside.tolist()
    mask = np.full((c.h, c.w), 9, dtype=np.uint8)
    st = _capi.YmMapSeenStats()
    assert lib.ym_map_seen_through(c.m._m, cm._h, None, None, 0, None, 0, 2, 1, None, None, mask.ctypes.data_as(C.POINTER(C.c_uint8)),
                                   C.byref(st)) == 0
    assert not mask.any() and (st.rays, st.inside, st.seen) == (0, 0, 0)
    assert lib.ym_map_seen_through(c.m._m, cm._h, hs, pp, 3, vs, 2, 2, 1, cp, None, None, C.byref(st)) == 0
    assert (st.inside, st.seen) == (int(inside.sum()), int(seen.sum())) and st.rays == 2 * (N_BEAMS - 3)
    cm.close()


# ---- blanked copies -----------------------------------------------------------------------------------------------------------
def test_a_blanked_copy_has_nan_where_flagged_the_same_poses_and_num_and_leaves_the_original_alone(ctx):
    from yag_slam_amd.transform import Transform
    c = ctx
    held, viewers = held_scans(c), viewer_scans(c)
    old = held[0]
    old.num = 41
    old.odom_pose = Transform(old.corrected_pose.x - 0.31, old.corrected_pose.y + 0.17, 0.0, old.corrected_pose.euler[-1] + 0.05)
    cm = _counted(c, held)
    st = cm.seen_through(viewers, flags=True)
    flags, ranges = st.flags[0], old.ranges.copy()
    assert flags.sum() == st.seen[0] >= 10
    new = old.blanked(flags)
    assert new is not old and new.ranges is not old.ranges and np.array_equal(old.ranges, ranges, equal_nan=True)
    assert np.array_equal(new.ranges, S.blanked_ranges(ranges, flags), equal_nan=True) and np.isnan(new.ranges[flags]).all()
    assert np.array_equal(new.ranges[~flags], ranges[~flags], equal_nan=True)
    assert new.num == 41 and _tf(new.corrected_pose) == _tf(old.corrected_pose) and _tf(new.odom_pose) == _tf(old.odom_pose)
    assert [getattr(new, k) for k in new._SENSOR_KEYS] == [getattr(old, k) for k in old._SENSOR_KEYS]
    with pytest.raises(ValueError, match="flags"):
        old.blanked(flags[:-1])
    # its own device twin: swapped in, the map is the map of the blanked readings, and nothing of it is seen through any more
    cm.update_scans([old], [new])
    assert new in cm and old not in cm and new._native is not None and new._native != old._native
    want = R.build((c.h, c.w), R.calculate_kernel(c.res, c.smear), [new, held[1], held[2]], c.ox, c.oy, c.res)[0]
    got = cm.to_numpy()
    assert np.array_equal(got != 0, want != 0) and np.abs(got - want).max() <= 1e-15
    again = cm.seen_through(viewers, scans=[new], flags=True)
    assert again.seen.tolist() == [0] and again.inside.tolist() == [int(st.inside[0] - st.seen[0])] and not again.flags[0].any()
    cm.close()


# ---- MapBuilder: a box that is taken away -------------------------------------------------------------------------------------
ROOM_W, ROOM_H = ROOM_WINDOW[2], ROOM_WINDOW[3]
SECOND_HALF = [(2.6 + 1.1 * k, 4.05 + 0.02 * k, 0.1 * math.sin(0.9 * k)) for k in range(5)]  # through where the box stood
MIN_READINGS = 8


def room_run():
    """(truth, scans, on the box): six scans around the box, then -- the box gone -- five along a line through where it stood.
    Every scan starts at the first pose and carries an odometry pose that drifts 1 cm, -0.5 cm and 0.004 rad per step in the
    previous scan's frame, like tests/test_gpu_map_grow.py's walk."""
    from yag_slam_amd.transform import Transform
    with_box, empty = room_scenes()
    truth = list(OLD_POSES) + list(SECOND_HALF)
    odom = [Transform(truth[0][0], truth[0][1], 0.0, truth[0][2])]
    for a, b in zip(truth, truth[1:]):
        d = Transform(b[0], b[1], 0.0, b[2]) - Transform(a[0], a[1], 0.0, a[2])
        odom.append(odom[-1] + Transform(d.x + 0.01, d.y - 0.005, 0.0, d.euler[-1] + 0.004))
    scans = []
    for i, t in enumerate(truth):
        s = room_scan(with_box if i < len(OLD_POSES) else empty, t, 700 + i, pose=truth[0])
        s.odom_pose = Transform(odom[i].x, odom[i].y, 0.0, odom[i].euler[-1])
        s.num = i
        scans.append(s)
    return truth, scans, [on_box(with_box, empty, t) for t in OLD_POSES]


def _room_builder(m, forget):
    from yag_slam_amd.mapping import MapBuilder
    cm = m.empty_correlation_map(ROOM_W, ROOM_H, counted=True, ox=ROOM_ANCHOR[0], oy=ROOM_ANCHOR[1])
    return MapBuilder(m, cm, ROOM_ANCHOR[0], ROOM_ANCHOR[1], min_response=0.3, forget_seen_through=forget), cm


def _check_room(m, cm, held):
    """tests/test_gpu_map_forget.py's `_check` rule for the room's map (its own `_check` clones scans of that file's sensor): the
    restated grid of `held` (the same nonzero cells, 1e-15 on values because of `exp`), the restated counts, and bit for bit a
    fresh counted map and an uncounted one that received copies of the scans, and the map of the image stamps > 0"""
    from tests import mapforget_ref as F
    ox, oy = ROOM_ANCHOR
    for s in held:
        x, y = s.points()
        assert R.distance_to_half(x, y, ox, oy, ROOM_RES) > R.HALF_GUARD, "a reading lies on a tie"
    want, (_, _, _, cells) = R.build((ROOM_H, ROOM_W), R.calculate_kernel(ROOM_RES, 0.05), held, ox, oy, ROOM_RES)
    got, stamps = cm.to_numpy(), cm.stamps()
    assert np.array_equal(got != 0, want != 0) and np.abs(got - want).max() <= 1e-15
    assert stamps.dtype == np.uint32 and np.array_equal(stamps.astype(np.int64), F.counts_of((ROOM_H, ROOM_W), cells))
    twins = [s.copy() for s in held]
    fresh = m.empty_correlation_map(ROOM_W, ROOM_H, counted=True, ox=ox, oy=oy)
    fresh.add_scans(ox, oy, twins)
    assert np.array_equal(got, fresh.to_numpy()) and np.array_equal(stamps, fresh.stamps())
    fresh.close()
    plain = m.empty_correlation_map(ROOM_W, ROOM_H)
    plain.add_scans(ox, oy, twins)
    assert np.array_equal(got, plain.to_numpy())
    plain.close()
    occ = m.correlation_grid_from_occupancy(np.where(stamps > 0, 0, 255).astype(np.uint8), occupied_value=0)
    assert np.array_equal(got, occ.to_numpy())
    occ.close()


def test_map_builder_forgets_the_readings_on_a_box_that_was_taken_away_and_keeps_the_walls():
    """Measured on an MI355X (the test prints the figures in every run): the first keyframe after the box is gone looks through 27
    to 32 readings of each of the six scans and all six are blanked, the four later ones flag nothing; 180 of the 180 box readings
    are gone (the cap: at least 90 %) and 0 of the 1986 others (the cap: at most 1 %), at a largest pose error of 0.029 m; the
    box's footprint keeps 85 stamped cells without the option and none with it.  The caps are the issue's: at true poses the host
    test shows 100 % and 0 %, the margin is for matched poses a fraction of a cell off."""
    from yag_slam_amd.mapping import MapBuilder
    from yag_slam_amd.scan_matching import ScanMatcher
    m = ScanMatcher(dict(resolution=ROOM_RES, smear_deviation=0.05, range_threshold=12.0), semantics="yagpy")
    with pytest.raises(ValueError, match="a window needs a map that can forget"):
        MapBuilder(m, m.empty_correlation_map(8, 8), 0.0, 0.0, forget_seen_through=MIN_READINGS)
    with pytest.raises(ValueError, match="forget_seen_through"):
        MapBuilder(m, m.empty_correlation_map(8, 8, counted=True, ox=0.0, oy=0.0), 0.0, 0.0, forget_seen_through=0)
    truth, scans, box = room_run()
    n_old = len(OLD_POSES)
    b, cm = _room_builder(m, MIN_READINGS)
    # 1: the device's decisions against the restatement, step by step at the poses the builder produced
    mirror = []  # the restated `added`: (scan, pose) of what the map should hold
    for i, s in enumerate(scans):
        b.forget_seen_through = MIN_READINGS if i >= n_old else None  # the first half only builds the map
        n_pairs = len(b.blanked)
        r = b.process_scan(s)
        assert r is None or (r.meta["accepted"] and r.meta["added"]), (i, r.response)
        pairs = b.blanked[n_pairs:]
        if i >= n_old:
            held = [(x, S.pose_of(x)) for x in mirror]
            assert S.distance_to_half(held + [(s, S.pose_of(s))], ROOM_ANCHOR, ROOM_RES) > S.HALF_GUARD, "a matched pose put a reading on a tie"
            inside, seen, flags, _, _ = S.seen_through(ROOM_WINDOW, ROOM_ANCHOR, ROOM_RES, held, [(s, S.pose_of(s))], 2, 1)
            want = [k for k in range(len(mirror)) if seen[k] >= MIN_READINGS]
            assert [id(old) for old, _ in pairs] == [id(mirror[k]) for k in want], (i, seen.tolist(), [o.num for o, _ in pairs])
            for k, (old, new) in zip(want, pairs):
                assert np.array_equal(new.ranges, S.blanked_ranges(old.ranges, flags[k]), equal_nan=True), (i, k)
                assert new.num == old.num and _tf(new.corrected_pose) == _tf(old.corrected_pose) and new in cm and old not in cm
                mirror[k] = new
            print("keyframe %d: seen %s of inside %s, %d scans blanked" % (i, seen.tolist(), inside.tolist(), len(pairs)))
        else:
            assert not pairs
        mirror.append(s)
        assert [id(x) for x in b.added] == [id(x) for x in mirror] and len(cm) == len(mirror) and not b.dropped
    assert len(b.blanked) >= 1
    # 2: the map is the restated map of the final `added`, by tests/test_gpu_map_forget.py's rule
    _check_room(m, cm, b.added)
    # 3, 4: of the readings the first-half scans had on the box at least 90 % are gone, of their other valid readings at most 1 %
    final = {x.num: x for x in b.added}
    box_all = box_nan = other_all = other_nan = 0
    for i in range(n_old):
        was, now = scans[i].ranges, final[i].ranges
        valid = ~((was > scans[i].range_threshold) | np.isnan(was))
        box_all += int((valid & box[i]).sum())
        box_nan += int((valid & box[i] & np.isnan(now)).sum())
        other_all += int((valid & ~box[i]).sum())
        other_nan += int((valid & ~box[i] & np.isnan(now)).sum())
    err = [math.hypot(s.corrected_pose.x - t[0], s.corrected_pose.y - t[1]) for s, t in zip(scans, truth)]
    print("box readings gone: %d of %d; other readings gone: %d of %d; largest pose error %.4f m" % (box_nan, box_all, other_nan, other_all, max(err)))
    assert box_all >= 100 and box_nan >= 0.9 * box_all, (box_nan, box_all)
    assert other_nan <= 0.01 * other_all, (other_nan, other_all)
    x0, x1 = (int(round((v - ROOM_ANCHOR[0]) / ROOM_RES)) for v in BOX[:2])
    y0, y1 = (int(round((v - ROOM_ANCHOR[1]) / ROOM_RES)) for v in BOX[2:])
    with_option = int((cm.stamps()[y0 - 1:y1 + 2, x0 - 1:x1 + 2] > 0).sum())
    # 5: the control run without the option: nothing is blanked and the box stays stamped in the map
    _, again, _ = room_run()
    u, plain = _room_builder(m, None)
    u.process_scans(again)
    assert not u.blanked and [id(x) for x in u.added] == [id(x) for x in again]
    assert all(np.array_equal(x.ranges, s.ranges, equal_nan=True) for x, s in zip(u.added, scans))  # none of them is NaN now
    without = int((plain.stamps()[y0 - 1:y1 + 2, x0 - 1:x1 + 2] > 0).sum())
    print("stamped cells in the box's footprint: %d with the option, %d without" % (with_option, without))
    assert without >= 40 and with_option < without
    plain.close()
    cm.close()
    m.close()
