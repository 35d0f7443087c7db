"""Maps whose window moves, on the device: `ym_map_reframe`, `ym_map_window`,
`ym_map_create_counted_window`, `CorrelationMap.reframe` and `MapBuilder(extent=...)`.

The yardstick is tests/mapreframe_ref.py: after every reframe a counted map must be the restatement of its held scans in the new
window (the same nonzero cells, 1e-15 on values because of `exp`, the counts exactly), and on the device it must equal bit for bit
a fresh `window=` map that received twins of the scans and `correlation_grid_from_occupancy` of the image `stamps > 0`.  `_check`
asserts all of it, and the call's statistics against the restatement's.  Both configurations of tests/test_gpu_map_grow.py, whose
maps are less than two gather tiles across; the three 91-beam scans of tests/test_gpu_map_forget.py, some of whose readings lie
beyond the nearer sides; every fixture asserts on the CPU that no quotient lies within 1e-6 of a tie of the anchor's lattice."""
import ctypes as C
import math

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from tests import mapgrow_ref as R  # noqa: E402
from tests import mapreframe_ref as W  # noqa: E402
from tests.test_gpu_map_forget import _abc, _assert_equals_restatement, _clone, _coarse, _key, _tf, ctx  # noqa: E402,F401
from tests.test_gpu_map_grow import WALK_MIN_RESPONSE, WALK_RES, _guard, _scan, _walk  # noqa: E402


def _anchor(c):
    return (c.ox, c.oy)


def _start(c):
    """a counted map in the fixture's window holding the three scans, and the scans"""
    scans = _abc(c)
    cm = c.m.empty_correlation_map(c.w, c.h, counted=True, ox=c.ox, oy=c.oy)
    cm.add_scans(c.ox, c.oy, scans)
    return cm, scans


def _check(c, cm, held, window):
    """`cm` against every form of the map of `held` in `window`; returns (restated grid, restated counts)"""
    _guard(held, c.ox, c.oy, c.res)
    assert cm.window == window and cm.shape == (window[3], window[2]) and cm.anchor == _anchor(c)
    assert cm.origin == W.origin(_anchor(c), window, c.res)
    x0, y0, w, h = (C.c_int32() for _ in range(4))
    assert c.m._lib.ym_map_window(cm._h, C.byref(x0), C.byref(y0), C.byref(w), C.byref(h)) == 0
    assert (x0.value, y0.value, w.value, h.value) == window
    want, counts = W.build(c.kernel, held, _anchor(c), c.res, window)
    got, stamps = cm.to_numpy(), cm.stamps()
    _assert_equals_restatement(got, want)
    assert stamps.dtype == np.uint32 and np.array_equal(stamps.astype(np.int64), counts)
    fresh = c.m.empty_correlation_map(window[2], window[3], counted=True, ox=c.ox, oy=c.oy, window=window[:2])
    assert fresh.origin == cm.origin and fresh.window == window
    fresh.add_scans(fresh.origin[0], fresh.origin[1], [_clone(s) for s in held])
    assert np.array_equal(got, fresh.to_numpy()) and np.array_equal(stamps, fresh.stamps())
    fresh.close()
    occ = c.m.correlation_grid_from_occupancy(np.where(stamps > 0, 0, 255).astype(np.uint8), occupied_value=0)
    assert np.array_equal(got, occ.to_numpy())
    occ.close()
    return want, counts


def _reframe(c, cm, held, dx, dy, width=None, height=None):
    """one reframe with its statistics checked against the restatement; returns (stats, restated grid of the new window)"""
    old, before, rev = cm.window, cm.stamps().astype(np.int64), cm.revision
    new = W.moved(old, dx, dy, width, height)
    _, want = W.reframe_counted(before, held, _anchor(c), c.res, old, dx, dy, width, height)
    st = cm.reframe(dx, dy, width, height)
    assert (st.kept, st.restamped, st.dropped, st.mismatch) == (want["kept"], want["restamped"], want["dropped"], 0), (st, want)
    assert (st.x0, st.y0, st.width, st.height) == new and cm.revision == rev + 1
    # recomputed: the cells within the taps' reach of the overlap whose neighbourhood meets the two windows differently
    half = c.taps // 2
    ox0, ox1 = max(old[0], new[0]) - new[0], min(old[0] + old[2], new[0] + new[2]) - new[0]
    oy0, oy1 = max(old[1], new[1]) - new[1], min(old[1] + old[3], new[1] + new[3]) - new[1]
    reach = np.zeros((new[3], new[2]), dtype=bool)
    if ox1 > ox0 and oy1 > oy0:
        reach[max(0, oy0 - half):oy1 + half, max(0, ox0 - half):ox1 + half] = True
    assert st.recomputed == np.count_nonzero(W.touches_difference(old, new, half) & reach)
    return st, _check(c, cm, held, new)[0]


# ---- scrolls, and away and back ------------------------------------------------------------------------------------------------
def test_scrolls_by_shifts_that_are_no_multiple_of_a_tile_and_away_and_back_is_the_identity(ctx):
    c = ctx
    cm, held = _start(c)
    w0 = (0, 0, c.w, c.h)
    grid0, counts0 = cm.to_numpy(), cm.stamps()
    _check(c, cm, held, w0)
    st, away = _reframe(c, cm, held, 13, -7)
    assert st.kept == (c.w - 13) * (c.h - 7) and len(cm) == 3 and all(s in cm for s in held)
    assert not np.array_equal(away, grid0)
    st = cm.reframe(-13, 7)  # back: bit for bit the map and the counts of the start
    assert st.mismatch == 0 and cm.window == w0 and cm.origin == (c.ox, c.oy)
    assert np.array_equal(cm.to_numpy(), grid0) and np.array_equal(cm.stamps(), counts0)
    _reframe(c, cm, held, -13, 7)  # and on to the other side
    cm.reframe(13, -7)
    assert np.array_equal(cm.to_numpy(), grid0) and np.array_equal(cm.stamps(), counts0) and cm.revision == 5
    cm.close()


def test_a_grow_on_all_four_sides_stamps_what_the_old_window_dropped(ctx):
    c = ctx
    cm, held = _start(c)
    dropped_before = W.window_cells(held, _anchor(c), c.res, (0, 0, c.w, c.h))[1]
    st, _ = _reframe(c, cm, held, -9, -6, c.w + 20, c.h + 15)
    assert st.restamped > 0 and st.kept == c.w * c.h and st.dropped == dropped_before - st.restamped
    cm.close()


def test_a_crop_takes_the_taps_of_the_cells_beyond_the_new_border(ctx):
    c = ctx
    cm, held = _start(c)
    old = cm.to_numpy()
    st, want = _reframe(c, cm, held, 5, 4, c.w - 11, c.h - 9)
    assert st.restamped == 0 and st.kept == (c.w - 11) * (c.h - 9) and st.recomputed > 0
    plain_crop = old[4:4 + c.h - 9, 5:5 + c.w - 11]
    assert plain_crop.shape == want.shape and (plain_crop != cm.to_numpy()).any()  # a border cell lost taps
    cm.close()


def test_a_window_without_overlap_the_identity_and_a_grow_from_nothing(ctx):
    c = ctx
    cm, held = _start(c)
    grid0, counts0, rev = cm.to_numpy(), cm.stamps(), cm.revision
    st = cm.reframe(0, 0)  # the identity: nothing changes, the revision neither
    assert (st.kept, st.restamped, st.dropped, st.recomputed, st.mismatch) == (c.w * c.h, 0, 0, 0, 0) and cm.revision == rev
    st = cm.reframe(0, 0, c.w, c.h)
    assert st.kept == c.w * c.h and cm.revision == rev and np.array_equal(cm.to_numpy(), grid0) and np.array_equal(cm.stamps(), counts0)
    st, _ = _reframe(c, cm, held, c.w + 3, 0)  # beside the old window: whatever it holds was stamped now
    assert st.kept == 0 and st.recomputed == 0 and st.restamped == int(cm.stamps().sum())
    st, _ = _reframe(c, cm, held, 40 * c.w, -40 * c.h)  # far from every reading
    assert (st.kept, st.restamped) == (0, 0) and not cm.to_numpy().any() and not cm.stamps().any() and len(cm) == 3
    cm.reframe(-41 * c.w - 3, 40 * c.h)  # and home again, from the held scans alone
    assert np.array_equal(cm.to_numpy(), grid0) and np.array_equal(cm.stamps(), counts0)
    cm.close()


# ---- forgetting goes on in the new window --------------------------------------------------------------------------------------
def test_remove_and_sync_after_a_scroll_leave_the_map_of_the_others_in_the_new_window(ctx):
    c = ctx
    cm, (a, b, s3) = _start(c)
    cm.reframe(13, -7)
    win = (13, -7, c.w, c.h)
    st = cm.remove_scans([b])
    assert st.unmatched == 0 and st.removed == len(W.window_cells([b], _anchor(c), c.res, win)[0]) > 0
    _check(c, cm, [a, s3], win)
    tf = type(a.corrected_pose)
    a.corrected_pose = tf(c.poses[0][0] + 3.7 * c.res, c.poses[0][1] - 2.2 * c.res, 0.0, c.poses[0][2] + 0.11)
    st = cm.sync()
    assert st.unmatched == 0 and st.removed > 0 and st.added > 0
    _check(c, cm, [a, s3], win)
    cm.add_scans(cm.origin[0], cm.origin[1], [b])  # the new origin, and only that, takes scans
    _check(c, cm, [a, b, s3], win)
    with pytest.raises(ValueError, match="origin"):
        cm.add_scans(c.ox, c.oy, [_clone(b)])
    cm.close()


def test_a_scroll_with_more_held_scans_than_a_chunk(ctx):
    """4100 scans of 4 beams (a launch takes 4096) on a lattice of poses near the left side, so that a scroll to the left brings
    readings in that the window had dropped and pushes others out on the right"""
    from yag_slam_amd import models
    c = ctx
    rng = np.random.default_rng(29)
    n = 4100
    scans = []
    for i in range(n):
        px, py = c.ox + (4.37 + (i % 41) * 1.3) * c.res, c.cy + ((i // 41 % 25) - 12.0 + 0.29) * 0.9 * c.res
        scans.append(_scan(rng.uniform(3.0, 11.0, 4) * c.res, (px, py, 0.7 * (i % 9))))
    _guard(scans, c.ox, c.oy, c.res)
    models.native_many(scans, c.m.device)
    cm = c.m.empty_correlation_map(c.w, c.h, counted=True, ox=c.ox, oy=c.oy)
    first = cm.add_scans(c.ox, c.oy, scans)
    assert first.dropped > 0 and len(cm) == n
    old = (0, 0, c.w, c.h)
    new = W.moved(old, -12, 3)
    _, want = W.reframe_counted(cm.stamps().astype(np.int64), scans, _anchor(c), c.res, old, -12, 3, None, None)
    st = cm.reframe(-12, 3)
    assert (st.kept, st.restamped, st.dropped, st.mismatch) == (want["kept"], want["restamped"], want["dropped"], 0)
    assert st.restamped > 0
    grid, counts = W.build(c.kernel, scans, _anchor(c), c.res, new)
    assert np.array_equal(cm.stamps().astype(np.int64), counts)
    _assert_equals_restatement(cm.to_numpy(), grid)
    occ = c.m.correlation_grid_from_occupancy(np.where(counts > 0, 0, 255).astype(np.uint8), occupied_value=0)
    assert np.array_equal(cm.to_numpy(), occ.to_numpy())
    occ.close()
    st = cm.remove_scans(scans[1::2])  # the counts still match the scans: nothing unmatched
    assert st.unmatched == 0
    assert np.array_equal(cm.stamps().astype(np.int64), W.counts(scans[0::2], _anchor(c), c.res, new))
    cm.close()


# ---- a map that keeps no counts ------------------------------------------------------------------------------------------------
def test_an_uncounted_map_is_shifted_into_zeros_and_takes_scans_at_the_origin_the_caller_moved(ctx):
    c = ctx
    a, b, s3 = _abc(c)
    cm = c.m.empty_correlation_map(c.w, c.h)
    cm.add_scans(c.ox, c.oy, [a, b])
    assert cm.window == (0, 0, c.w, c.h) and cm.anchor is None and cm.origin is None
    grid = cm.to_numpy()
    for dx, dy, nw, nh in ((13, -7, c.w, c.h), (-22, 9, c.w + 31, c.h + 5), (6, 3, c.w - 2, c.h - 9)):
        rev = cm.revision
        st = cm.reframe(dx, dy, nw, nh)
        want = W.shifted(grid, dx, dy, nw, nh)
        assert np.array_equal(cm.to_numpy(), want) and cm.shape == (nh, nw) and cm.revision == rev + 1 and cm.origin is None
        assert (st.restamped, st.dropped, st.recomputed, st.mismatch) == (0, 0, 0, 0) and (st.width, st.height) == (nw, nh)
        grid = want
    x0, y0 = cm.window[:2]
    assert (x0, y0) == (13 - 22 + 6, -7 + 9 + 3) and grid.any()
    # the caller's origin follows the window; an add there equals the restatement's add onto the shifted array
    ox, oy = c.ox + x0 * c.res, c.oy + y0 * c.res
    _guard([s3], ox, oy, c.res)
    st = cm.add_scans(ox, oy, [s3])
    _, stamped, dropped, _ = R.add_scans(grid, c.kernel, [s3], ox, oy, c.res)
    assert (st.stamped, st.dropped) == (stamped, dropped) and stamped > 0
    _assert_equals_restatement(cm.to_numpy(), grid)
    # what scoring reads moved with the float grid
    twin = c.m.upload_correlation_grid(cm.to_numpy())
    q = _scan(c.ranges[2], c.poses[2])
    assert _key(c.m.match_scan_sets_with_map(cm, ox, oy, [q], True, True, coarse=_coarse(c))) == _key(
        c.m.match_scan_sets_with_map(twin, ox, oy, [q], True, True, coarse=_coarse(c)))
    twin.close()
    cm.close()


# ---- matching follows the bytes ------------------------------------------------------------------------------------------------
def test_matching_on_a_reframed_map_equals_matching_on_an_upload_of_the_restated_grid(ctx):
    c = ctx
    cm, held = _start(c)
    _, want = _reframe(c, cm, held, 13, -7)
    ox, oy = cm.origin
    twin = c.m.upload_correlation_grid(want)
    p0, p1, p2 = c.poses
    q = _scan(c.ranges[0], (p0[0] + 2.3 * c.res, p0[1] - 1.4 * c.res, p0[2] + 0.02))
    a = c.m.match_scan_sets_with_map(cm, ox, oy, [q], True, True, coarse=_coarse(c))
    b = c.m.match_scan_sets_with_map(twin, ox, oy, [q], True, True, coarse=_coarse(c))
    assert _key(a) == _key(b) and a.response > 0.0, (_key(a), _key(b))
    sets = [[q], [_scan(c.ranges[1], p1), _scan(c.ranges[2], p2)]]
    ra = c.m.match_map_batch(cm, ox, oy, sets, True, True, coarse=_coarse(c))
    rb = c.m.match_map_batch(twin, ox, oy, sets, True, True, coarse=_coarse(c))
    assert [_key(r) for r in ra] == [_key(r) for r in rb]
    out = []
    for mp in (cm, twin):
        track = [_scan(c.ranges[2], p2), _scan(c.ranges[2], p2, odom=(p2[0] + 1.7 * c.res, p2[1] + 0.9 * c.res, p2[2] - 0.015))]
        res, done = c.m.track_in_map(mp, ox, oy, track, 1, True, True, _coarse(c), 0.0)
        assert done == 2
        out.append((res[1].response, res[1].covariance, _tf(res[1].best_pose), res[1].meta["accepted"], _tf(track[1].corrected_pose)))
    assert out[0] == out[1]
    twin.close()
    cm.close()


def test_a_locator_made_before_a_reframe_refuses_and_one_made_after_it_locates(ctx):
    c = ctx
    cm, held = _start(c)
    q = _scan(c.ranges[0], c.poses[0])
    with c.m.map_locator(cm, levels=2) as old:
        assert len(old.locate([q], c.ox, c.oy, n_angles=8)) >= 1
        cm.reframe(0, 0)  # the identity: the map and its revision stay, and so does the locator
        assert len(old.locate([q], c.ox, c.oy, n_angles=8)) >= 1
        cm.reframe(13, -7)
        with pytest.raises(ValueError, match="make a new locator"):
            old.locate([q], cm.origin[0], cm.origin[1], n_angles=8)
    with c.m.map_locator(cm, levels=2) as new:
        cands = new.locate([q], cm.origin[0], cm.origin[1], n_angles=8)
        assert len(cands) >= 1 and cands[0].response > 0
        assert np.array_equal(new.read_level(0), (100 * cm.to_numpy()).astype(np.uint8))
    cm.close()


# ---- through ctypes ------------------------------------------------------------------------------------------------------------
def test_the_library_refuses_what_it_must_and_a_refused_call_changes_nothing(ctx):
    from yag_slam_amd import _capi
    from yag_slam_amd.scan_matching import ScanMatcher
    c = ctx
    L = c.m._lib
    cm, held = _start(c)
    grid, counts = cm.to_numpy(), cm.stamps()
    hs = (C.c_void_p * 3)(*[c.m._require_native(s) for s in held])
    good = np.array([_tf(s.corrected_pose) for s in held], dtype=np.float64)
    dp = C.POINTER(C.c_double)
    st = _capi.YmMapReframeStats()

    def unchanged():
        x0, y0, w, h = (C.c_int32() for _ in range(4))
        assert L.ym_map_window(cm._h, C.byref(x0), C.byref(y0), C.byref(w), C.byref(h)) == 0
        return ((x0.value, y0.value, w.value, h.value) == (0, 0, c.w, c.h) and np.array_equal(cm.to_numpy(), grid)
                and np.array_equal(cm.stamps(), counts))

    # poses the scans were not added at: here so far off that none of their readings falls into the kept cells
    wrong = good.copy()
    wrong[:, 0] += 40.0 * c.w * c.res
    kept_sum = int(W.shifted(counts.astype(np.int64), 13, -7, c.w, c.h).sum())
    assert L.ym_map_reframe(c.m._m, cm._h, 13, -7, c.w, c.h, hs, wrong.ctypes.data_as(dp), 3, C.byref(st)) == -1
    assert st.mismatch == kept_sum > 0 and "nothing was changed" in _capi.last_error() and unchanged()
    assert (st.x0, st.y0, st.width, st.height) == (0, 0, c.w, c.h)
    # a list that lacks a held scan
    assert L.ym_map_reframe(c.m._m, cm._h, 13, -7, c.w, c.h, hs, good.ctypes.data_as(dp), 2, C.byref(st)) == -1
    assert st.mismatch > 0 and unchanged()
    # sizes, offsets, a null scan
    for w, h in ((0, c.h), (c.w, -1), (40000, 40000)):
        assert L.ym_map_reframe(c.m._m, cm._h, 1, 1, w, h, hs, good.ctypes.data_as(dp), 3, None) == -1 and "size" in _capi.last_error()
    assert L.ym_map_reframe(c.m._m, cm._h, 2 ** 30 + 1, 0, c.w, c.h, hs, good.ctypes.data_as(dp), 3, None) == -1
    assert "offset" in _capi.last_error()
    assert L.ym_map_reframe(c.m._m, cm._h, 0, -2 ** 30 - 1, c.w, c.h, hs, good.ctypes.data_as(dp), 3, None) == -1
    two = (C.c_void_p * 2)(hs[0], None)
    assert L.ym_map_reframe(c.m._m, cm._h, 1, 1, c.w, c.h, two, good.ctypes.data_as(dp), 2, None) == -1 and "scan 1" in _capi.last_error()
    assert not L.ym_map_create_counted_window(c.m._m, c.w, c.h, c.ox, c.oy, -2 ** 30 - 1, 0) and "offset" in _capi.last_error()
    assert unchanged()
    # a held list on a map that keeps no counts
    plain = c.m.empty_correlation_map(c.w, c.h)
    plain.add_scans(c.ox, c.oy, held[:1])
    before = plain.to_numpy()
    assert L.ym_map_reframe(c.m._m, plain._h, 1, 1, c.w, c.h, hs, good.ctypes.data_as(dp), 1, None) == -1 and "n_held" in _capi.last_error()
    assert np.array_equal(plain.to_numpy(), before) and plain.window == (0, 0, c.w, c.h)
    plain.close()
    # a matcher of the other semantics
    karto = ScanMatcher(dict(resolution=0.05, smear_deviation=0.05, search_size=0.3), semantics="karto")
    assert karto._lib.ym_map_reframe(karto._m, cm._h, 1, 1, c.w, c.h, hs, good.ctypes.data_as(dp), 3, None) == -4
    assert "YM_SEM_YAGPY" in _capi.last_error()
    assert not karto._lib.ym_map_create_counted_window(karto._m, c.w, c.h, c.ox, c.oy, 1, 1) and "YM_SEM_YAGPY" in _capi.last_error()
    karto.close()
    assert unchanged()
    # through Python: the books stay as they were too
    p = held[0].corrected_pose
    cm._held[id(held[0])] = (held[0], (p.x + 40.0 * c.w * c.res, p.y, p.euler[-1]))
    with pytest.raises(RuntimeError, match="disagree"):
        cm.reframe(13, -7)
    assert cm.window == (0, 0, c.w, c.h) and cm.origin == (c.ox, c.oy) and cm.revision == 1 and unchanged()
    cm.close()


# ---- MapBuilder follows the robot ----------------------------------------------------------------------------------------------
def test_a_scrolling_windowed_builder_walks_the_room_exactly_as_one_on_a_map_of_the_whole_room():
    """tests/test_gpu_map_grow.py's 31-scan walk (4.5 m along the room, range threshold 4 m) with window=4 keyframes, once on a
    map of 176 x 176 cells (8.8 m) that scrolls and once on a fixed map of the whole room, both in the lattice of one anchor.
    The margin is what a step reads or stamps around the pose: 4 m of range, 0.25 m of coarse search and the taps' 0.1 m, 87 of
    the 88 cells between the centre and a side, so the window recentres (to a multiple of 2 cells) whenever the robot is more than
    a cell off its centre."""
    from yag_slam_amd.mapping import MapBuilder
    from yag_slam_amd.scan_matching import ScanMatcher
    res, anchor, n = WALK_RES, (-0.613, -0.437), 176
    m = ScanMatcher(dict(resolution=res, smear_deviation=0.05, range_threshold=4.0), semantics="yagpy")
    truth, scans = _walk()
    _, fixed_scans = _walk()
    start = (int(np.round((truth[0][0] - anchor[0]) / res)) - n // 2, int(np.round((truth[0][1] - anchor[1]) / res)) - n // 2)
    room = (-20, -20, 230, 190)  # the room's 8 m x 6 m and a metre around it
    cm = m.empty_correlation_map(n, n, counted=True, ox=anchor[0], oy=anchor[1], window=start)
    big = m.empty_correlation_map(room[2], room[3], counted=True, ox=anchor[0], oy=anchor[1], window=room[:2])
    kw = dict(min_response=WALK_MIN_RESPONSE, min_distance=0.2, min_rotation=0.1, window=4)
    b = MapBuilder(m, cm, cm.origin[0], cm.origin[1], extent="scroll", step=2, **kw)
    u = MapBuilder(m, big, big.origin[0], big.origin[1], **kw)
    assert b.margin == 4.0 + 0.25 + 2 * res and u.extent == "fixed"
    kernel = R.calculate_kernel(res, 0.05)
    for i, (s, t) in enumerate(zip(scans, fixed_scans)):
        r, q = b.process_scan(s), u.process_scan(t)
        assert _tf(s.corrected_pose) == _tf(t.corrected_pose), i
        if r is not None:
            assert (r.meta["accepted"], r.meta["added"]) == (q.meta["accepted"], q.meta["added"]), i
        assert (b.ox, b.oy) == cm.origin == W.origin(anchor, cm.window, res) and cm.shape == (n, n)
        # every reading of every keyframe in the map lies inside the window: nothing was dropped at a side
        assert W.window_cells(b.added, anchor, res, cm.window)[1] == 0, i
    assert len(b.reframes) >= 2 and all(st.x0 % 2 == start[0] % 2 and st.mismatch == 0 for st in b.reframes)
    assert cm.window[0] > start[0] + 60 and len(b.added) == 4 and [scans.index(x) for x in b.added] == [fixed_scans.index(x) for x in u.added]
    _guard(b.added, anchor[0], anchor[1], res)
    want, counts = W.build(kernel, b.added, anchor, res, cm.window)
    _assert_equals_restatement(cm.to_numpy(), want)
    assert np.array_equal(cm.stamps().astype(np.int64), counts)
    # the two maps hold the same cells where they overlap
    x0, y0 = cm.window[0] - room[0], cm.window[1] - room[1]
    assert np.array_equal(big.to_numpy()[max(0, y0):y0 + n, x0:x0 + n], cm.to_numpy()[max(0, -y0):room[3] - y0, :room[2] - x0])
    err = math.hypot(scans[-1].corrected_pose.x - truth[-1][0], scans[-1].corrected_pose.y - truth[-1][1])
    print("scroll: %d reframes, window %r, lost %d, final error %.4f m" % (len(b.reframes), cm.window, b.lost, err))
    big.close()
    cm.close()
    m.close()


# ---- more rows than one launch has rows of blocks -------------------------------------------------------------------------------
TALL_W, TALL_H = 8, 4 * 65535 + 69  # 262 209 rows: the mark runs in five pieces of 65 535 rows, the gather (tiles of 4 rows) in two
TALL_BANDS = ((0, 6), (65534, 65538), (262138, 262144), (TALL_H - 4, TALL_H))  # [first, last) rows: each holds stamped cells


class _Tall(object):
    pass


@pytest.fixture(scope="module")
def tall():
    """the 5 x 5 tap configuration, a map 8 cells wide and 262 209 high, and six scans of 12 beams that look along +y and reach
    half a cell to five cells: their poses put stamped cells on the first rows, on both sides of the seam between the mark's first
    two pieces (row 65 535), on both sides of the seam between the gather's two pieces (row 262 140) and on the last rows.  The
    scans stand near the east side, so that some readings lie beyond it and a scroll by one column has something to stamp."""
    from yag_slam_amd.scan_matching import ScanMatcher
    from tests.test_gpu_map_grow import CONFIGS, INC, MIN_ANGLE
    from tests import mapforget_ref as F
    _, res, smear, taps, _, _ = CONFIGS[0]
    t = _Tall()
    t.res, t.taps, t.w, t.h = res, taps, TALL_W, TALL_H
    t.kernel = R.calculate_kernel(res, smear)
    assert t.kernel.shape == (5, 5)
    t.ox, t.oy = -0.513, 0.237
    n = 12
    heading = 0.5 * math.pi - MIN_ANGLE - 0.5 * (n - 1) * INC  # the fan's middle beam points along +y
    rng = np.random.default_rng(31)
    t.ranges, t.poses = [], []
    for row in (0.3, 65532.3, 65534.6, 262136.3, 262139.4, TALL_H - 4.6):
        t.ranges.append(rng.uniform(0.5, 5.0, n) * res)
        t.poses.append((t.ox + 6.4 * res, t.oy + row * res, heading))
    t.fresh_scans = lambda: [_scan(r, p) for r, p in zip(t.ranges, t.poses)]
    scans = t.fresh_scans()
    _guard(scans, t.ox, t.oy, res)
    t.cells = [F.cells_of([s], (t.h, t.w), t.ox, t.oy, res) for s in scans]
    rows = set(gy for v in t.cells for _, gy in v)
    for lo, hi in TALL_BANDS:
        assert rows & set(range(lo, hi)), (lo, hi)
    assert {65534, 65535} & rows and {65536, 65537} & rows and {262138, 262139} & rows and {262140, 262141, 262142, 262143} & rows
    assert (TALL_H - 1) in rows and min(rows) <= 3
    cols = set(gx for v in t.cells for gx, _ in v)
    assert {5, 6, 7} <= cols and all(len(v) < n for v in t.cells[:1] + t.cells[-1:])  # (the first and last scans: readings beyond the east side or the top)
    t.m = ScanMatcher(dict(resolution=res, smear_deviation=smear, range_threshold=12.0), semantics="yagpy")
    yield t
    t.m.close()


def _tall_map(t, scans, window=(0, 0)):
    cm = t.m.empty_correlation_map(t.w, t.h, counted=True, ox=t.ox, oy=t.oy, window=window)
    cm.add_scans(cm.origin[0], cm.origin[1], scans)
    return cm


def test_a_removal_whose_released_box_spans_more_tile_rows_than_one_launch_takes(tall):
    """the first and the last scan go in one call: the released box runs from the first rows to the last, 65 553 rows of tiles, and
    the gather takes it in two launches"""
    from tests import mapforget_ref as F
    t = tall
    scans = t.fresh_scans()
    cm = _tall_map(t, scans)
    st = cm.remove_scans([scans[0], scans[-1]])
    gone = t.cells[0] + t.cells[-1]
    assert (st.removed, st.unmatched) == (len(gone), 0) and st.released > 0 and len(cm) == 4
    assert st.y0 <= 3 and st.y1 == t.h and (st.y1 - st.y0 + 3) // 4 > 65535
    got, stamps = cm.to_numpy(), cm.stamps()
    fresh = _tall_map(t, [_clone(s) for s in scans[1:-1]])
    assert np.array_equal(got, fresh.to_numpy()) and np.array_equal(stamps, fresh.stamps())
    fresh.close()
    counts = F.counts_of((t.h, t.w), [x for v in t.cells[1:-1] for x in v])
    assert np.array_equal(stamps.astype(np.int64), counts)
    want = F.from_counts(counts, t.kernel)
    half = t.taps // 2
    for lo, hi in TALL_BANDS:  # the bands, and what the taps reach from them
        lo, hi = max(0, lo - half), min(t.h, hi + half)
        _assert_equals_restatement(got[lo:hi], want[lo:hi])
    assert not got[:8].any() and not got[-8:].any() and got[65530:65545].any() and got[262134:262150].any()
    cm.close()


def test_a_scroll_by_one_column_of_a_map_with_more_rows_than_one_launch_takes(tall):
    """reframe(1, 0): the overlap is seven columns of every row, so the mark covers all 262 209 rows in five launches and the gather
    all 65 553 rows of tiles in two; column 7 of the new window comes from the counts and from the readings the old one dropped"""
    t = tall
    scans = t.fresh_scans()
    cm = _tall_map(t, scans)
    st = cm.reframe(1, 0)
    assert (st.kept, st.mismatch) == (7 * t.h, 0) and st.restamped > 0 and st.recomputed > t.h
    assert cm.window == (1, 0, t.w, t.h) and cm.anchor == (t.ox, t.oy)
    got, stamps = cm.to_numpy(), cm.stamps()
    fresh = _tall_map(t, [_clone(s) for s in scans], window=(1, 0))
    assert fresh.window == cm.window and fresh.origin == cm.origin
    assert np.array_equal(got, fresh.to_numpy()) and np.array_equal(stamps, fresh.stamps())
    fresh.close()
    for lo, hi in TALL_BANDS:
        assert got[max(0, lo - 2):hi + 2, 7].any(), (lo, hi)  # the new column holds values in and around every band
    cm.close()
