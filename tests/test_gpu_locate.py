"""The map locator on the device (ym_locator_*, ScanMatcher.map_locator / locate_in_map, LoopClosingMapper.relocalize) against
the numpy yardstick tests/locate_ref.py: every comparison of candidates is exact, in scores, indices and order.  The
yardstick is evaluated on the point set the search itself used (points_out) and the byte grid read back from the device."""
import ctypes as C
import math

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from tests import locate_ref as R  # noqa: E402

CFG = dict(resolution=R.ROOM_RES, smear_deviation=R.ROOM_RES)
STEP = 2 * math.pi / R.ROOM_ANGLES


def _scan(truth=R.ROOM_TRUTH, pose=(0.0, 0.0, 0.0), index=950):
    from yag_slam_amd import synth
    return synth.resident_scan(synth.Scene().scan_ranges(truth, index=index), pose)


class _Ctx(object):
    pass


@pytest.fixture(scope="module")
def ctx():
    from yag_slam_amd import synth
    from yag_slam_amd.scan_matching import ScanMatcher
    c = _Ctx()
    c.m = ScanMatcher(CFG, semantics="yagpy")
    c.scan = _scan()
    c.image = R.room_image(synth.Scene())
    c.room = c.m.correlation_grid_from_occupancy(c.image, occupied_value=0)
    c.room_g8 = R.byte_grid(c.room.to_numpy())
    c.ref, c.maps = {}, {}
    yield c
    for mp, _ in c.maps.values():
        mp.close()
    c.room.close()
    c.m.close()


def _uploaded(c, name, grid):
    """(resident map, byte grid) of a float grid, uploaded once"""
    if name not in c.maps:
        mp = c.m.upload_correlation_grid(grid)
        c.maps[name] = (mp, R.byte_grid(mp.to_numpy()))
    return c.maps[name]


def _pairs(cands):
    return [(c.score, c.index) for c in cands]


def _reference(c, key, g8, points, n_angles=R.ROOM_ANGLES):
    """(offsets, S) of a map and point set, computed once per key and left unchanged"""
    if key not in c.ref:
        offs = R.offsets(points, R.dir_table(n_angles), R.ROOM_RES)
        c.ref[key] = (points.copy(), offs, R.score_volume(g8, offs))
    assert np.array_equal(c.ref[key][0], points)
    return c.ref[key][1:]


def _locate(c, cmap, g8, key, levels=None, max_nodes=None, scans=None, **kw):
    kw.setdefault("n_angles", R.ROOM_ANGLES)
    kw.setdefault("point_stride", 6)
    with c.m.map_locator(cmap, levels=levels, max_nodes=max_nodes) as loc:
        cands = loc.locate(scans or [c.scan], R.ROOM_ORIGIN[0], R.ROOM_ORIGIN[1], **kw)
        stats, pts, info = loc.last_stats, loc.last_points, (loc.shape, loc.levels, loc.max_nodes)
    offs, S = _reference(c, key, g8, pts, kw["n_angles"])
    assert stats["nq"] == len(pts) == offs.shape[1]
    return cands, stats, S, info


def test_room_top16_is_the_yardsticks_and_lies_at_the_true_pose(ctx):
    cands, stats, S, info = _locate(ctx, ctx.room, ctx.room_g8, "room")
    print("room: stats", stats, "hypotheses", S.size, "best", cands[0])
    assert info[0] == R.ROOM_SHAPE and info[1] == 4 and info[2] == 1 << 25
    assert _pairs(cands) == R.top_k(S, 16)
    H, W = R.ROOM_SHAPE
    for c in cands:
        assert (c.k, c.cx, c.cy) == R.decode(c.index, W, H)
        assert c.response == c.score / (100.0 * stats["nq"])
        assert (c.pose.x, c.pose.y) == (R.ROOM_ORIGIN[0] + c.cx * R.ROOM_RES, R.ROOM_ORIGIN[1] + c.cy * R.ROOM_RES)
        assert abs(c.pose.euler[-1] - math.atan2(math.sin(c.k * STEP), math.cos(c.k * STEP))) < 1e-12
    b = cands[0]
    assert abs(b.pose.x - R.ROOM_TRUTH[0]) <= R.ROOM_RES + 1e-9 and abs(b.pose.y - R.ROOM_TRUTH[1]) <= R.ROOM_RES + 1e-9
    assert abs(b.pose.euler[-1] - R.ROOM_TRUTH[2]) <= STEP / 2
    # one scan: its located pose is the set's centre, its heading turned by the located heading
    assert len(b.poses) == 1 and abs(b.poses[0].x - b.pose.x) < 1e-9 and abs(b.poses[0].y - b.pose.y) < 1e-9
    assert stats["chunks"] == 1 and sum(stats["nodes"]) + stats["probe_nodes"] < 0.5 * S.size


@pytest.mark.parametrize("levels", [0, 2, 5])
def test_random_byte_map_where_pruning_is_weak(ctx, levels):
    cmap, g8 = _uploaded(ctx, "random", R.random_grid())
    assert g8.shape == (53, 61)
    cands, stats, S, info = _locate(ctx, cmap, g8, "random", levels=levels)
    print("random map, levels", levels, stats)
    assert info[1] == levels
    assert _pairs(cands) == R.top_k(S, 16)


def test_levels_beyond_what_the_map_allows_are_refused(ctx):
    """61 x 53: a top-level node of 2^7 cells is wider than the map -- refused (include/yagmatch.h says so), not clamped"""
    from yag_slam_amd._capi import YmError
    cmap, _ = _uploaded(ctx, "random", R.random_grid())
    for levels in (6, 7, 9):
        with pytest.raises(YmError, match="levels"):
            ctx.m.map_locator(cmap, levels=levels)
    with pytest.raises(YmError, match="max_nodes"):  # one top-level node of 32 x 32 cells alone exceeds the budget
        ctx.m.map_locator(cmap, levels=5, max_nodes=1000)
    with ctx.m.map_locator(cmap, levels=5, max_nodes=1024) as loc:
        assert loc.levels == 5 and loc.max_nodes == 1024


def test_all_zero_map_prunes_nothing_and_stays_inside_its_buffers(ctx):
    cmap, g8 = _uploaded(ctx, "zero", np.zeros((29, 37)))
    for max_nodes in (None, 1 << 12, 16):  # one chunk; many; the fewest a top-level node of 4 x 4 cells allows
        cands, stats, S, info = _locate(ctx, cmap, g8, "zero", max_nodes=max_nodes)
        assert info[1] == 2 == R.default_levels(37, 29)
        assert _pairs(cands) == [(0, i) for i in range(16)] == R.top_k(S, 16)
        assert stats["survivors"] == stats["nodes"] and stats["nodes"][0] == S.size
        assert stats["chunks"] == 1 if max_nodes is None else stats["chunks"] >= S.size / max_nodes


def test_occupied_cells_only_at_the_corners(ctx):
    """the best hypotheses sit on the map's edges with most points outside it: a pyramid without its low-side margin, or a
    read outside the map that counts, fails here"""
    cmap, g8 = _uploaded(ctx, "corners", R.corner_grid())
    cands, stats, S, _ = _locate(ctx, cmap, g8, "corners")
    assert _pairs(cands) == R.top_k(S, 16) and cands[0].score > 0
    cands2, _, _, _ = _locate(ctx, cmap, g8, "corners", levels=5)
    assert _pairs(cands2) == _pairs(cands)


def test_map_sides_that_are_no_multiple_of_the_top_level_node(ctx):
    cmap, g8 = _uploaded(ctx, "odd", R.random_grid(97, 83, 9) ** 4)
    cands, stats, S, info = _locate(ctx, cmap, g8, "odd", levels=4)
    assert info[0] == (83, 97) and info[1] == 4
    assert _pairs(cands) == R.top_k(S, 16)


def test_many_chunks_return_what_one_chunk_returns(ctx):
    one, stats1, S, _ = _locate(ctx, ctx.room, ctx.room_g8, "room")
    many, stats, _, _ = _locate(ctx, ctx.room, ctx.room_g8, "room", max_nodes=256 * 100)
    print("chunks", stats["chunks"], stats)
    assert stats1["chunks"] == 1 and stats["chunks"] >= 8
    assert _pairs(many) == _pairs(one) == R.top_k(S, 16)
    assert [(c.pose.x, c.pose.y, c.pose.euler[-1], c.response) for c in many] == [(c.pose.x, c.pose.y, c.pose.euler[-1], c.response) for c in one]


def test_min_response_is_a_floor_on_the_score(ctx):
    _, stats, S, _ = _locate(ctx, ctx.room, ctx.room_g8, "room")
    nq = stats["nq"]
    distinct = np.unique(S)[::-1]
    none, _, _, _ = _locate(ctx, ctx.room, ctx.room_g8, "room", min_response=(int(distinct[0]) + 1) / (100.0 * nq))
    assert none == []
    mr = (distinct[2] + distinct[3]) / 2.0 / (100.0 * nq)
    s_min = R.s_min_of(mr, nq)
    assert distinct[3] < s_min <= distinct[2]
    got, _, _, _ = _locate(ctx, ctx.room, ctx.room_g8, "room", min_response=mr, top_k=64)
    assert _pairs(got) == R.top_k(S, 64, s_min) and 3 <= len(got) < 64


def test_every_pyramid_level_is_the_sliding_maximum(ctx):
    cmap, g8 = _uploaded(ctx, "random", R.random_grid())
    with ctx.m.map_locator(cmap, levels=5) as loc:
        for j in range(6):
            m = (1 << j) - 1
            assert np.array_equal(loc.read_level(j), R.pyramid_level(g8, j)[m:, m:]), j
        from yag_slam_amd._capi import YmError
        with pytest.raises(YmError):
            loc.read_level(6)
    cmap, g8 = _uploaded(ctx, "corners", R.corner_grid())
    with ctx.m.map_locator(cmap, levels=3) as loc:  # the low-side margin shows in the levels above: level 3 from level 2's margin
        assert np.array_equal(loc.read_level(3), R.pyramid_level(g8, 3)[7:, 7:])


def test_two_scans_are_located_as_one_set(ctx):
    """two scans taken 0.5 m and 0.3 rad apart, given in an odometry frame that is not the map's; every point of both counts"""
    t0, t1 = R.ROOM_TRUTH, (R.ROOM_TRUTH[0] + 0.4, R.ROOM_TRUTH[1] + 0.3, R.ROOM_TRUTH[2] + 0.3)
    c, s = math.cos(-t0[2]), math.sin(-t0[2])
    rel = (c * (t1[0] - t0[0]) - s * (t1[1] - t0[1]), s * (t1[0] - t0[0]) + c * (t1[1] - t0[1]), t1[2] - t0[2])
    scans = [_scan(t0, (10.0, -4.0, 0.0), 950), _scan(t1, (10.0 + rel[0], -4.0 + rel[1], rel[2]), 951)]
    with ctx.m.map_locator(ctx.room) as loc:
        cands = loc.locate(scans, R.ROOM_ORIGIN[0], R.ROOM_ORIGIN[1], n_angles=R.ROOM_ANGLES, point_stride=1)
        pts, stats = loc.last_points, loc.last_stats
    want = R.set_points(scans)
    assert stats["nq"] == len(pts) == len(want) > 2000
    assert np.abs(pts - want).max() <= 1e-12
    offs, S = _reference(ctx, "two", ctx.room_g8, pts)
    assert _pairs(cands) == R.top_k(S, 16)
    # the located set: its centre within one cell of where the scans' mean position truly lies, both scans moved rigidly
    b = cands[0]
    centre = (0.5 * (t0[0] + t1[0]), 0.5 * (t0[1] + t1[1]))
    assert abs(b.pose.x - centre[0]) <= R.ROOM_RES + 1e-9 and abs(b.pose.y - centre[1]) <= R.ROOM_RES + 1e-9
    assert abs(b.pose.euler[-1] - t0[2]) <= STEP / 2
    d_in = math.hypot(rel[0], rel[1])
    d_out = math.hypot(b.poses[1].x - b.poses[0].x, b.poses[1].y - b.poses[0].y)
    assert abs(d_in - d_out) < 1e-9 and abs((b.poses[1].euler[-1] - b.poses[0].euler[-1]) - rel[2]) < 1e-9
    for p, t in zip(b.poses, (t0, t1)):
        assert math.hypot(p.x - t[0], p.y - t[1]) <= 2 * R.ROOM_RES and abs(p.euler[-1] - t[2]) <= STEP / 2


def test_locate_polish_and_splice(ctx):
    """locate_in_map(refine=True) on the room lands within one cell and one fine-angle step of the truth; relocalize then
    splice_first_scan on a mapper filled by map_to_graphslam goes through"""
    from yag_slam_amd.mapping import LoopClosingMapper
    from yag_slam_amd.scan_matching import ScanMatcher
    from yag_slam_amd.splicing import map_to_graphslam
    r = ctx.m.locate_in_map(ctx.room, R.ROOM_ORIGIN[0], R.ROOM_ORIGIN[1], [ctx.scan], refine=True, n_angles=R.ROOM_ANGLES, point_stride=6)
    p = r.best_pose[0]
    err = (p.x - R.ROOM_TRUTH[0], p.y - R.ROOM_TRUTH[1], p.euler[-1] - R.ROOM_TRUTH[2])
    print("polished pose off the truth by", err, "response", r.response, "located", r.meta["candidates"][0])
    assert len(r.best_pose) == 1 and len(r.meta["candidates"]) == 16
    assert math.hypot(err[0], err[1]) <= R.ROOM_RES and abs(err[2]) <= 0.00349
    coarse = ctx.m.locate_in_map(ctx.room, R.ROOM_ORIGIN[0], R.ROOM_ORIGIN[1], [ctx.scan], refine=False, n_angles=R.ROOM_ANGLES, point_stride=6)
    assert coarse.best_pose[0].x == r.meta["candidates"][0].pose.x and coarse.response == r.meta["candidates"][0].response
    with pytest.raises(ValueError, match="min_response"):
        ctx.m.locate_in_map(ctx.room, R.ROOM_ORIGIN[0], R.ROOM_ORIGIN[1], [ctx.scan], n_angles=R.ROOM_ANGLES, point_stride=6, min_response=0.999)
    # min_separation: the device's 64 best, thinned on the host
    with ctx.m.map_locator(ctx.room) as loc:
        raw = loc.locate([ctx.scan], R.ROOM_ORIGIN[0], R.ROOM_ORIGIN[1], n_angles=R.ROOM_ANGLES, point_stride=6, top_k=64)
        thin = loc.locate([ctx.scan], R.ROOM_ORIGIN[0], R.ROOM_ORIGIN[1], n_angles=R.ROOM_ANGLES, point_stride=6, top_k=4,
                          min_separation=(0.5, 0.5))
    from yag_slam_amd.scan_matching import filter_min_separation
    assert _pairs(thin) == _pairs(filter_min_separation(raw, 0.5, 0.5)[:4]) and _pairs(thin)[0] == _pairs(raw)[0] and 1 <= len(thin) <= 4
    assert all(math.hypot(a.pose.x - b.pose.x, a.pose.y - b.pose.y) > 0.5 or
               abs((a.pose.euler[-1] - b.pose.euler[-1] + math.pi) % (2 * math.pi) - math.pi) > 0.5 for a in thin for b in thin if a is not b)

    seq = ScanMatcher(None, device=0)
    mp = LoopClosingMapper(seq, None)
    map_to_graphslam(mp, ctx.image, R.ROOM_RES, R.ROOM_ORIGIN, R.room_labels(ctx.image), layout="world")
    k = len(mp.scans)
    live = _scan(index=952)  # switched on somewhere: its pose says nothing
    res = mp.relocalize(live, ctx.room, R.ROOM_ORIGIN[0], R.ROOM_ORIGIN[1], n_angles=R.ROOM_ANGLES, point_stride=6)
    q = live.corrected_pose
    assert (q.x, q.y, q.euler[-1]) == (res.best_pose[0].x, res.best_pose[0].y, res.best_pose[0].euler[-1])
    assert (live.odom_pose.x, live.odom_pose.y, live.odom_pose.euler[-1]) == (q.x, q.y, q.euler[-1])
    assert math.hypot(q.x - R.ROOM_TRUTH[0], q.y - R.ROOM_TRUTH[1]) <= R.ROOM_RES
    spliced = mp.splice_first_scan(live)
    assert spliced is not None and live.num == k and mp.scans[-1] is live and mp.running_scans == [live]
    with pytest.raises(ValueError, match="min_response"):
        mp.relocalize(_scan(index=953), ctx.room, R.ROOM_ORIGIN[0], R.ROOM_ORIGIN[1], n_angles=R.ROOM_ANGLES, point_stride=6, min_response=0.999)


def test_refusals_return_their_codes_and_write_nothing(ctx):
    """(a map on another device needs a second device and is not exercised here)"""
    from yag_slam_amd import _capi
    from yag_slam_amd.scan_matching import ScanMatcher
    L = ctx.m._lib
    karto = ScanMatcher(None)
    assert not L.ym_locator_create(karto._m, ctx.room._h, -1, 0) and "YAGPY" in _capi.last_error()
    assert not L.ym_locator_create(None, ctx.room._h, -1, 0) and not L.ym_locator_create(ctx.m._m, None, -1, 0)
    karto.close()
    h = ctx.m._require_native(ctx.scan)
    dirs = np.ascontiguousarray(R.dir_table(4))
    dp = dirs.ctypes.data_as(C.POINTER(C.c_double))
    with ctx.m.map_locator(ctx.room) as loc:
        def call(lc=loc._h, queries=(h,), n_queries=None, dir_cs=dp, n_angles=4, opts=(16, 6, 0.0), out=True, found=True):
            hs = (C.c_void_p * 66)(*(list(queries) + [None] * (66 - len(queries)))) if queries is not None else None
            o = _capi.YmLocateOpts(*opts) if opts is not None else None
            cand = (_capi.YmLocateCandidate * 64)()
            C.memset(cand, 0x5a, C.sizeof(cand))
            n_found, stats = C.c_int(-77), _capi.YmLocateStats()
            C.memset(C.byref(stats), 0x5a, C.sizeof(stats))
            pts = np.full((70000, 2), -77.0)
            rc = L.ym_locator_locate(lc, 0.0, 0.0, hs, len(queries) if n_queries is None else n_queries, dir_cs, n_angles,
                                     C.byref(o) if o is not None else None, cand if out else None, C.byref(n_found) if found else None,
                                     pts.ctypes.data_as(C.POINTER(C.c_double)), C.byref(stats))
            untouched = (bytes(cand) == b"\x5a" * C.sizeof(cand) and n_found.value == -77 and bytes(stats) == b"\x5a" * C.sizeof(stats) and
                         bool((pts == -77.0).all()))
            return rc, untouched
        INVALID, UNSUPPORTED = -1, -4
        assert call(lc=None) == (INVALID, True)
        assert call(queries=None, n_queries=1) == (INVALID, True)
        assert call(dir_cs=None) == (INVALID, True)
        assert call(out=False) == (INVALID, True) and call(found=False) == (INVALID, True)
        assert call(n_queries=0) == (INVALID, True) and call(queries=(h,) * 65) == (INVALID, True)
        assert call(queries=(h, None)) == (INVALID, True)
        assert call(n_angles=0) == (INVALID, True) and call(n_angles=-3) == (INVALID, True)
        assert call(opts=(0, 6, 0.0)) == (INVALID, True) and call(opts=(65, 6, 0.0)) == (INVALID, True)
        assert call(opts=(16, 0, 0.0)) == (INVALID, True) and call(opts=(16, -1, 0.0)) == (INVALID, True)
        assert call(opts=(16, 6, -0.5)) == (INVALID, True)
        empty = _scan()
        empty_far = type(empty)(np.full(len(empty.ranges), 99.0), *[getattr(empty, k) for k in empty._SENSOR_KEYS], 0.0, 0.0, 0.0)
        assert call(queries=(ctx.m._require_native(empty_far),)) == (INVALID, True)  # no valid reading: the stride leaves no point
        rc, untouched = call(opts=None)  # defaults: top_k 16, every point
        assert rc == 0 and not untouched
        assert call(queries=(h,) * 64)[0] == 0
    # a point more than 32767 cells from the centre: a matcher with 0.1 mm cells, readings beyond 3.3 m
    fine = ScanMatcher(dict(resolution=0.0001, smear_deviation=0.0002, search_size=0.002, range_threshold=0.01), semantics="yagpy")
    tiny = fine.upload_correlation_grid(np.zeros((8, 8)))
    with fine.map_locator(tiny) as loc:
        assert call(lc=loc._h, queries=(fine._require_native(ctx.scan),)) == (UNSUPPORTED, True)
    tiny.close()
    fine.close()
