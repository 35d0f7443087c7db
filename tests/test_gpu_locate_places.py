"""The places search on the device (ym_locator_locate_places, MapLocator.locate_places) against the numpy yardstick
tests/locate_places_ref.py: the greedy rule on the exhaustive volume, evaluated on the point set the search itself used
(points_out) and the byte grid read back from the device.  Every comparison of candidates is exact, in scores, indices and
order.  Maps and point sets are those of tests/test_gpu_locate.py (point_stride 6, 36 headings)."""
import ctypes as C
import math

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from tests import locate_places_ref as P  # noqa: E402
from tests import locate_ref as R  # noqa: E402

CFG = dict(resolution=R.ROOM_RES, smear_deviation=R.ROOM_RES)
STEP = 2 * math.pi / R.ROOM_ANGLES
OX, OY = R.ROOM_ORIGIN


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
    c.room = c.m.correlation_grid_from_occupancy(R.room_image(synth.Scene()), occupied_value=0)
    c.room_g8 = R.byte_grid(c.room.to_numpy())
    c.ref, c.maps = {}, {}
    yield c
    for mp, _ in c.maps.values():
        mp.close()
    c.room.close()
    c.m.close()


def _uploaded(c, name, grid):
    if name not in c.maps:
        mp = c.m.upload_correlation_grid(grid)
        c.maps[name] = (mp, R.byte_grid(mp.to_numpy()))
    return c.maps[name]


def _pairs(cands):
    return [(c.score, c.index) for c in cands]


def _volume(c, key, g8, points):
    """S of a map and point set, computed once per key and left unchanged"""
    if key not in c.ref:
        c.ref[key] = (points.copy(), R.score_volume(g8, R.offsets(points, R.dir_table(R.ROOM_ANGLES), R.ROOM_RES)))
    assert np.array_equal(c.ref[key][0], points)
    return c.ref[key][1]


def _places(c, cmap, g8, key, K, sep, levels=None, max_nodes=None, scans=None, headings=None, **kw):
    """(candidates, stats, S) of one locate_places with separation_cells = sep"""
    with c.m.map_locator(cmap, levels=levels, max_nodes=max_nodes) as loc:
        cands = loc.locate_places(scans or [c.scan], OX, OY, n_places=K, separation_cells=sep, n_angles=R.ROOM_ANGLES, headings=headings,
                                  point_stride=kw.pop("point_stride", 6), **kw)
        stats, pts, used = loc.last_stats, loc.last_points, loc.last_separation
    assert used == (sep[0], sep[1], 1 if headings is None else 0)
    S = _volume(c, key, g8, pts)
    assert stats["nq"] == len(pts)
    assert stats["rounds"] == len(cands) + (1 if len(cands) < K else 0) == len(stats["round_nodes"])
    assert sum(stats["round_nodes"]) == stats["nodes"] + stats["probe_nodes"]
    return cands, stats, S


LINEAR = 2.0 * np.pi * np.arange(R.ROOM_ANGLES) / float(R.ROOM_ANGLES)  # the default table, given explicitly: not circular


def test_room_holds_eight_places_and_the_best_64_do_not(ctx):
    """the test that fails without the call: 8 places at (100, 3), of which thinning the best 64 sees fewer"""
    cands, stats, S = _places(ctx, ctx.room, ctx.room_g8, "room", 8, (100, 3))
    print("room places", _pairs(cands), stats)
    assert _pairs(cands) == P.places(S, 8, 100, 3, 1) and len(cands) == 8
    H, W = R.ROOM_SHAPE
    for c in cands:
        assert (c.k, c.cx, c.cy) == R.decode(c.index, W, H) and c.response == c.score / (100.0 * stats["nq"])
        assert (c.pose.x, c.pose.y) == (OX + c.cx * R.ROOM_RES, OY + c.cy * R.ROOM_RES)
    assert stats["rounds"] == 8 and stats["excluded_leaves"] > 0 and stats["chunks"] == 8
    with ctx.m.map_locator(ctx.room) as loc:
        thin = loc.locate([ctx.scan], OX, OY, n_angles=R.ROOM_ANGLES, point_stride=6, top_k=8, min_separation=(1.0, 3 * STEP + 1e-9))
        by_metres = loc.locate_places([ctx.scan], OX, OY, n_places=8, min_separation=(1.0, 3 * STEP + 1e-9), n_angles=R.ROOM_ANGLES,
                                      point_stride=6)
        assert loc.last_separation == (100, 3, 1)
    print("thinning the best 64 leaves", _pairs(thin))
    assert 1 <= len(thin) < 8 and _pairs(thin)[0] == _pairs(cands)[0]
    assert _pairs(by_metres) == _pairs(cands)


@pytest.mark.parametrize("levels", [0, 2, 5])
def test_random_byte_map_where_pruning_is_weak(ctx, levels):
    cmap, g8 = _uploaded(ctx, "random", R.random_grid())
    cands, stats, S = _places(ctx, cmap, g8, "random", 5, (9, 1), levels=levels)
    print("random map, levels", levels, stats)
    assert _pairs(cands) == P.places(S, 5, 9, 1, 1) and len(cands) == 5


@pytest.mark.parametrize("circular", [1, 0])
@pytest.mark.parametrize("max_nodes", [None, 1 << 12, 16])
def test_all_zero_map_in_one_chunk_and_in_many(ctx, max_nodes, circular):
    """every score ties: index and exclusion alone decide.  Six picks of radius 5 all fit into row 0 of heading 0, so the two
    values of `circular` return the same list here; where they differ is the next test's"""
    cmap, g8 = _uploaded(ctx, "zero", np.zeros((29, 37)))
    cands, stats, S = _places(ctx, cmap, g8, "zero", 6, (25, 2), max_nodes=max_nodes, headings=None if circular else LINEAR)
    assert _pairs(cands) == P.places(S, 6, 25, 2, circular) == [(0, 6 * i) for i in range(6)]
    assert stats["chunks"] == 6 if max_nodes is None else stats["chunks"] >= 6 * S.size / max_nodes
    assert stats["excluded_leaves"] > 0


def test_all_zero_map_where_a_pick_at_heading_0_reaches_the_last_headings(ctx):
    """on a circle a pick at k = 0 is near k = 34, 35 too: exactly that shows in what the search excluded (nothing is pruned on
    this map: every leaf is met in every round) ..."""
    cmap, g8 = _uploaded(ctx, "zero", np.zeros((29, 37)))
    _places(ctx, cmap, g8, "zero", 1, (0, 0))
    S = ctx.ref["zero"][1]
    for circular in (1, 0):  # without levels above the map: the hypotheses near the picks so far, round by round
        _, stats, _ = _places(ctx, cmap, g8, "zero", 6, (25, 2), levels=0, max_nodes=1 << 12, headings=None if circular else LINEAR)
        mask, n_near = np.zeros(S.shape, dtype=bool), 0
        for i in range(5):
            mask |= P.near_mask(S.shape, (0, 6 * i, 0), 25, 2, circular)
            n_near += int(mask.sum())
        assert stats["excluded_leaves"] == n_near and stats["excluded_nodes"] == 0
    # ... and in the lists once a pick covers its whole heading: k = 0, 5, .., 35 in a row, but 35 is near 0 on a circle
    far = 37 * 37 + 29 * 29
    for circular, ks in ((0, range(0, 36, 5)), (1, range(0, 35, 5))):
        cands, stats, S = _places(ctx, cmap, g8, "zero", 8, (far, 4), headings=None if circular else LINEAR)
        assert _pairs(cands) == P.places(S, 8, far, 4, circular) == [(0, k * 29 * 37) for k in ks]
        assert stats["excluded_nodes"] > 0


def test_occupied_cells_only_at_the_corners(ctx):
    cmap, g8 = _uploaded(ctx, "corners", R.corner_grid())
    cands, stats, S = _places(ctx, cmap, g8, "corners", 4, (4, 0))
    assert _pairs(cands) == P.places(S, 4, 4, 0, 1) and len(cands) == 4 and cands[0].score > 0


def test_map_sides_that_are_no_multiple_of_the_top_level_node(ctx):
    cmap, g8 = _uploaded(ctx, "odd", R.random_grid(97, 83, 9) ** 4)
    cands, stats, S = _places(ctx, cmap, g8, "odd", 5, (49, 2), levels=4)
    assert _pairs(cands) == P.places(S, 5, 49, 2, 1) and len(cands) == 5


def test_many_chunks_return_what_one_chunk_returns(ctx):
    one, stats1, S = _places(ctx, ctx.room, ctx.room_g8, "room", 8, (100, 3))
    many, stats, _ = _places(ctx, ctx.room, ctx.room_g8, "room", 8, (100, 3), max_nodes=256 * 100)
    assert stats1["chunks"] == 8 and stats["chunks"] >= 8 * 8
    assert _pairs(many) == _pairs(one) == P.places(S, 8, 100, 3, 1)
    assert [(c.pose.x, c.pose.y, c.pose.euler[-1], c.response) for c in many] == [(c.pose.x, c.pose.y, c.pose.euler[-1], c.response) for c in one]


def test_zero_separations_and_one_place_are_locate(ctx):
    """field for field, poses included, against ym_locator_locate on the same locator -- which still returns top_k(S, 16)
    after the places calls"""
    def fields(cands):
        return [(c.score, c.response, c.index, c.k, c.cx, c.cy, c.pose.x, c.pose.y, c.pose.euler[-1],
                 [(p.x, p.y, p.euler[-1]) for p in c.poses]) for c in cands]
    kw = dict(n_angles=R.ROOM_ANGLES, point_stride=6)
    with ctx.m.map_locator(ctx.room) as loc:
        top16 = loc.locate([ctx.scan], OX, OY, top_k=16, **kw)
        sixteen = loc.locate_places([ctx.scan], OX, OY, n_places=16, separation_cells=(0, 0), **kw)
        assert loc.last_stats["rounds"] == 16 and loc.last_stats["excluded_leaves"] == 15 * 16 // 2
        one = loc.locate_places([ctx.scan], OX, OY, n_places=1, separation_cells=(100, 3), **kw)
        assert loc.last_stats["rounds"] == 1 and loc.last_stats["excluded_leaves"] == 0 == loc.last_stats["excluded_nodes"]
        top1 = loc.locate([ctx.scan], OX, OY, top_k=1, **kw)
        again = loc.locate([ctx.scan], OX, OY, top_k=16, **kw)
        pts = loc.last_points
    S = _volume(ctx, "room", ctx.room_g8, pts)
    assert fields(sixteen) == fields(top16) == fields(again) and _pairs(again) == R.top_k(S, 16)
    assert fields(one) == fields(top1) and len(one) == 1


def test_min_response_is_a_floor_on_every_place(ctx):
    cands, stats, S = _places(ctx, ctx.room, ctx.room_g8, "room", 8, (100, 3))
    nq = stats["nq"]
    mr = (cands[1].score + cands[2].score) / 2.0 / (100.0 * nq)
    s_min = R.s_min_of(mr, nq)
    assert cands[2].score < s_min <= cands[1].score
    two, stats2, _ = _places(ctx, ctx.room, ctx.room_g8, "room", 8, (100, 3), min_response=mr)
    assert _pairs(two) == _pairs(cands)[:2] == P.places(S, 8, 100, 3, 1, s_min) and stats2["rounds"] == 3
    none, stats0, _ = _places(ctx, ctx.room, ctx.room_g8, "room", 8, (100, 3), min_response=(cands[0].score + 1) / (100.0 * nq))
    assert none == [] and stats0["rounds"] == 1


def test_a_separation_that_covers_the_volume_leaves_one_place(ctx):
    H, W = R.ROOM_SHAPE
    cands, stats, S = _places(ctx, ctx.room, ctx.room_g8, "room", 8, (W * W + H * H, 18))
    assert _pairs(cands) == R.top_k(S, 1) == P.places(S, 8, W * W + H * H, 18, 1)
    assert stats["rounds"] == 2 and stats["excluded_nodes"] > 0


def test_two_scans_are_located_as_one_set(ctx):
    t0, t1 = R.ROOM_TRUTH, (R.ROOM_TRUTH[0] + 0.4, R.ROOM_TRUTH[1] + 0.3, R.ROOM_TRUTH[2] + 0.3)
    c, s = math.cos(-t0[2]), math.sin(-t0[2])
    rel = (c * (t1[0] - t0[0]) - s * (t1[1] - t0[1]), s * (t1[0] - t0[0]) + c * (t1[1] - t0[1]), t1[2] - t0[2])
    scans = [_scan(t0, (10.0, -4.0, 0.0), 950), _scan(t1, (10.0 + rel[0], -4.0 + rel[1], rel[2]), 951)]
    cands, stats, S = _places(ctx, ctx.room, ctx.room_g8, "two", 3, (100, 3), scans=scans, point_stride=7)
    want = R.set_points(scans, 7)
    assert stats["nq"] == len(want) > 300 and np.abs(ctx.ref["two"][0] - want).max() <= 1e-12
    assert _pairs(cands) == P.places(S, 3, 100, 3, 1) and len(cands) == 3
    b = cands[0]
    centre = (0.5 * (t0[0] + t1[0]), 0.5 * (t0[1] + t1[1]))
    assert abs(b.pose.x - centre[0]) <= R.ROOM_RES + 1e-9 and abs(b.pose.y - centre[1]) <= R.ROOM_RES + 1e-9
    assert len(b.poses) == 2 and abs(b.pose.euler[-1] - t0[2]) <= STEP / 2


def test_refusals_return_their_code_and_write_nothing(ctx):
    from yag_slam_amd import _capi
    L = ctx.m._lib
    h = ctx.m._require_native(ctx.scan)
    dirs = np.ascontiguousarray(R.dir_table(4))
    dp = dirs.ctypes.data_as(C.POINTER(C.c_double))
    with ctx.m.map_locator(ctx.room) as loc:
        def call(lc=loc._h, queries=(h,), n_queries=None, dir_cs=dp, n_angles=4, opts=(4, 6, 0.0, 100, 1, 1), out=True, found=True):
            hs = (C.c_void_p * 66)(*(list(queries) + [None] * (66 - len(queries)))) if queries is not None else None
            o = _capi.YmLocatePlacesOpts(*opts) if opts is not None else None
            cand = (_capi.YmLocateCandidate * 16)()
            C.memset(cand, 0x5a, C.sizeof(cand))
            n_found, stats = C.c_int(-77), _capi.YmLocatePlacesStats()
            C.memset(C.byref(stats), 0x5a, C.sizeof(stats))
            pts = np.full((70000, 2), -77.0)
            rc = L.ym_locator_locate_places(lc, 0.0, 0.0, hs, len(queries) if n_queries is None else n_queries, dir_cs, n_angles,
                                            C.byref(o) if o is not None else None, cand if out else None,
                                            C.byref(n_found) if found else None, pts.ctypes.data_as(C.POINTER(C.c_double)), C.byref(stats))
            untouched = (bytes(cand) == b"\x5a" * C.sizeof(cand) and n_found.value == -77 and bytes(stats) == b"\x5a" * C.sizeof(stats) and
                         bool((pts == -77.0).all()))
            return rc, untouched
        INVALID = -1
        assert call(opts=None) == (INVALID, True)
        assert call(opts=(0, 6, 0.0, 100, 1, 1)) == (INVALID, True) and call(opts=(17, 6, 0.0, 100, 1, 1)) == (INVALID, True)
        assert call(opts=(4, 6, 0.0, -1, 1, 1)) == (INVALID, True) and call(opts=(4, 6, 0.0, 100, -1, 1)) == (INVALID, True)
        assert call(opts=(4, 6, 0.0, 100, 1, 2)) == (INVALID, True) and call(opts=(4, 6, 0.0, 100, 1, -1)) == (INVALID, True)
        # ym_locator_locate's own
        assert call(lc=None) == (INVALID, True) and call(queries=None, n_queries=1) == (INVALID, True) and call(dir_cs=None) == (INVALID, True)
        assert call(out=False) == (INVALID, True) and call(found=False) == (INVALID, True)
        assert call(n_queries=0) == (INVALID, True) and call(queries=(h,) * 65) == (INVALID, True) and call(queries=(h, None)) == (INVALID, True)
        assert call(n_angles=0) == (INVALID, True)
        assert call(opts=(4, 0, 0.0, 100, 1, 1)) == (INVALID, True) and call(opts=(4, 6, -0.5, 100, 1, 1)) == (INVALID, True)
        rc, untouched = call(opts=(16, 6, 0.0, 0, 0, 0))
        assert rc == 0 and not untouched
