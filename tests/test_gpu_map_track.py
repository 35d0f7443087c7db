"""Localization mode on the device: `ym_match_map_many` (N scan sets against one resident map in one
enqueue, their sums from yag_map_kernel), `ym_map_track`, and the Python surface over them.  The yardstick is `ym_match_map` on each set
alone -- pinned itself against the reference by tests/test_gpu_map.py: results are compared byte for byte and the integer sum
volumes of both passes entry for entry.  Every case asserts through the counters which kernel produced its sums."""
import ctypes as C
import math
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from tests.util import GOLDEN  # noqa: E402

SENSOR = dict(min_angle=-2.35619449, inc=4.71238898 / 180, min_range=0.05, max_range=30.0, range_threshold=12.0)


def _scan(ranges, pose, min_angle=SENSOR["min_angle"], inc=SENSOR["inc"]):
    from yag_slam_amd.models import LocalizedRangeScan
    r = np.asarray(ranges, dtype=np.float64)
    return LocalizedRangeScan(r, min_angle, min_angle + (len(r) - 1) * inc, inc, SENSOR["min_range"], SENSOR["max_range"],
                              SENSOR["range_threshold"], pose[0], pose[1], pose[2])


def _search(coarse):
    from yag_slam_amd.scan_matching import ScanMatcher
    return ScanMatcher._map_search(coarse)


def _single_raw(m, cmap, ox, oy, scans, penalty, fine, coarse):
    """ym_match_map on one set: (the ym_result, [sums of pass 0, sums of pass 1 or None])"""
    from yag_slam_amd import _capi
    hs = (C.c_void_p * len(scans))(*[m._require_native(q) for q in scans])
    cs = _search(coarse)
    res = _capi.YmResult()
    _capi.check(m._lib.ym_match_map(m._m, cmap._h, float(ox), float(oy), hs, len(scans), int(penalty), int(fine),
                                    C.byref(cs) if cs else None, C.byref(res)))
    return res, _volumes(m, res, 0, fine)


def _volumes(m, res, item, fine):
    return [m.debug_map_sums(0, item, tuple(res.coarse_dims)), m.debug_map_sums(1, item, tuple(res.fine_dims)) if fine else None]


def _many_raw(m, cmap, ox, oy, sets, penalty, fine, coarse):
    from yag_slam_amd import _capi
    flat = [q for s in sets for q in s]
    offs = np.cumsum([0] + [len(s) for s in sets]).astype(np.int32)
    hs = (C.c_void_p * len(flat))(*[m._require_native(q) for q in flat])
    cs = _search(coarse)
    per = (_capi.YmResult * len(sets))()
    _capi.check(m._lib.ym_match_map_many(m._m, cmap._h, float(ox), float(oy), hs, offs.ctypes.data_as(C.POINTER(C.c_int32)), len(sets),
                                         int(penalty), int(fine), C.byref(cs) if cs else None, per))
    return per


def _check_against_single(m, cmap, ox, oy, sets, penalty, fine, coarse=None, fallback=False, singles=None, volumes=True):
    """one ym_match_map_many call; every item must equal ym_match_map of its set alone, in the result's bytes and in both sum
    volumes, and the counters must name the kernel.  singles: cache {id(set): single call's outcome}, computed once per set."""
    before = m.debug_counters()
    per = _many_raw(m, cmap, ox, oy, sets, penalty, fine, coarse)
    after = m.debug_counters()
    served = (after["map_kernel_items"] - before["map_kernel_items"], after["map_fallback_items"] - before["map_fallback_items"])
    assert served == ((0, len(sets)) if fallback else (len(sets), 0)), served
    vols = [_volumes(m, per[i], i, fine) for i in range(len(sets))] if volumes else None
    singles = {} if singles is None else singles
    for i, s in enumerate(sets):
        if id(s) not in singles:
            singles[id(s)] = _single_raw(m, cmap, ox, oy, s, penalty, fine, coarse)
        one, one_vols = singles[id(s)]
        assert bytes(per[i]) == bytes(one), (i, per[i].response, one.response, per[i].status, one.status)
        if volumes:
            for p in range(2 if fine else 1):
                assert vols[i][p].dtype == one_vols[p].dtype and vols[i][p].shape == one_vols[p].shape
                assert np.array_equal(vols[i][p], one_vols[p]), (i, p, np.argwhere(vols[i][p] != one_vols[p])[:5])
    return per


# ---- 1, 2: the reference's fixtures ------------------------------------------------------------------------------------------
CASES = ["map_r05_two_scans", "map_r05_coarse_only", "map_r05_dirty_three", "map_r02_quirk"]


def _load(name):
    from tests.test_gpu_map import _load as load
    return load(name)


def _assert_fixture(z, r, scans):
    fin, coarse = z["final"], z["coarse"]
    assert r.meta["n_query_points"] == len(z["pts_local_x"])
    assert abs(r.meta["coarse_response"] - coarse[0]) <= 1e-12
    assert abs(r.response - float(z["response"])) <= 1e-12
    np.testing.assert_allclose(r.meta["corrected_centre"], fin[1:4], rtol=0, atol=1e-9)
    np.testing.assert_allclose(r.meta["centre"][:2], z["centre"], rtol=0, atol=0)
    np.testing.assert_allclose(np.array(r.covariance), z["covariance"], rtol=1e-9, atol=1e-15)
    assert len(r.best_pose) == len(scans) == len(r.meta["rigid_poses"])


@pytest.mark.parametrize("name", CASES)
def test_each_reference_fixture_as_a_one_item_call(name):
    from yag_slam_amd.scan_matching import ScanMatcher, _map_set_result
    z, cfg, scans = _load(name)
    m = ScanMatcher(cfg, semantics="yagpy")
    mp = m.correlation_grid_from_occupancy(z["image"], occupied_value=0)
    per = _check_against_single(m, mp, float(z["ox"]), float(z["oy"]), [scans], bool(z["penalty"]), bool(z["do_fine"]))
    assert per[0].status == 0
    _assert_fixture(z, _map_set_result(per[0], scans), scans)
    # the Python entry builds the same result
    r = m.match_map_batch(mp, float(z["ox"]), float(z["oy"]), [scans], bool(z["penalty"]), bool(z["do_fine"]))[0]
    _assert_fixture(z, r, scans)
    assert r.response == per[0].response


@pytest.mark.parametrize("fine", [True, False])
def test_two_fixtures_that_share_a_map_as_one_ragged_call(fine):
    from yag_slam_amd.scan_matching import ScanMatcher, _map_set_result
    za, cfg, two = _load("map_r05_two_scans")
    zb, _, one = _load("map_r05_coarse_only")
    assert np.array_equal(za["image"], zb["image"]) and float(za["ox"]) == float(zb["ox"]) and bool(za["penalty"]) == bool(zb["penalty"])
    m = ScanMatcher(cfg, semantics="yagpy")
    mp = m.correlation_grid_from_occupancy(za["image"], occupied_value=0)
    per = _check_against_single(m, mp, float(za["ox"]), float(za["oy"]), [two, one], bool(za["penalty"]), fine)
    if fine:  # (map_r05_two_scans wants the fine pass, map_r05_coarse_only does not)
        _assert_fixture(za, _map_set_result(per[0], two), two)
    else:
        _assert_fixture(zb, _map_set_result(per[1], one), one)


# ---- 3, 4: where the kernel can go wrong, at the smallest shapes -------------------------------------------------------------
class _Small(object):
    pass


# rint meets exact ties: cells of 0.25, lattice steps of 0.125, every coordinate a multiple of 0.125, the angle lattice holds 0.0
TIE = dict(xy_search=0.25, xy_step=0.125, angle_search=0.25, angle_step=0.125, grid_resolution=0.25)


@pytest.fixture(scope="module")
def small():
    """a 37 x 29 map at 0.05 with its corner at the world's origin, and the seven sets"""
    from yag_slam_amd.scan_matching import ScanMatcher
    c = _Small()
    c.m = ScanMatcher(dict(resolution=0.05, smear_deviation=0.05, range_threshold=12.0), semantics="yagpy")
    im = np.full((29, 37), 255, dtype=np.uint8)
    im[3, 3:34] = 0; im[25, 3:34] = 0; im[3:26, 3] = 0; im[3:26, 33] = 0          # a box
    for i in range(20):
        im[5 + i, 8 + i] = 0                                                         # a diagonal
    im[14, 20:30] = 0; im[8:20, 26] = 0                                            # a cross
    c.map = c.m.correlation_grid_from_occupancy(im, occupied_value=0)
    rng = np.random.default_rng(5)
    far = 100.0  # beyond the range threshold: no reading
    middle = [_scan(rng.uniform(0.2, 0.9, 181), (0.875, 0.75, 0.25))]
    outside = [_scan(rng.uniform(0.1, 0.3, 91), (-1.0, 2.45, 0.0)), _scan(rng.uniform(0.1, 0.3, 91), (2.85, 2.45, 3.0))]
    corner = [_scan(rng.uniform(0.2, 0.8, 181), (0.1, 0.1, 0.5))]
    tie = [_scan([0.375], (0.5, 0.5, 0.0), min_angle=0.0)]
    blind = [_scan(np.full(31, far), (0.9, 0.7, 0.0))]
    many = [_scan(rng.uniform(0.2, 0.7, 5), (0.6 + 0.01 * (i % 8), 0.5 + 0.02 * (i // 8), 0.1 * i)) for i in range(64)]
    r257 = rng.uniform(0.2, 0.9, 300)
    r257[rng.permutation(300)[:43]] = far
    block_plus_one = [_scan(r257, (1.0, 0.8, -0.4), inc=4.71238898 / 299)]
    c.sets = [middle, outside, corner, tie, blind, many, block_plus_one]
    c.singles = {None: {}, "tie": {}}
    yield c
    c.map.close()
    c.m.close()


@pytest.mark.parametrize("coarse", [None, "tie"])
@pytest.mark.parametrize("how", ["in_order", "permuted", "repeated_67", "chunks_of_3"])
def test_seven_sets_in_one_call(small, how, coarse):
    c = small
    cs = TIE if coarse == "tie" else None
    sets = c.sets
    if how == "permuted":
        sets = [c.sets[i] for i in (5, 2, 6, 4, 0, 3, 1)]
    elif how == "repeated_67":
        sets = [c.sets[i % 7] for i in range(67)]
    if how == "chunks_of_3":
        c.m.debug_option(47, 3)
    try:
        per = _check_against_single(c.m, c.map, 0.0, 0.0, sets, True, True, cs, singles=c.singles[coarse])
    finally:
        c.m.debug_option(47, 0)
    by_set = {id(s): per[i] for i, s in enumerate(sets)}
    blind, outside, tie, plus = (by_set[id(c.sets[i])] for i in (4, 1, 3, 6))
    assert blind.status != 0 and blind.n_query_points == 0
    assert [by_set[id(s)].status for s in c.sets if s is not c.sets[4]] == [0] * 6
    assert outside.response == 0.0 and outside.n_query_points == 182
    assert tie.n_query_points == 1 and plus.n_query_points == 257 and by_set[id(c.sets[5])].n_query_points == 320
    if coarse == "tie":
        assert tuple(tie.coarse_dims) == (4, 4, 4)
        # the point is (0.875, 0.5) exactly; at angle 0 the four columns are rint(2.5), rint(3), rint(3.5), rint(4) = 2, 3, 4, 4 and
        # the four rows rint(1), rint(1.5), rint(2), rint(2.5) = 1, 2, 2, 2 of the byte grid
        _, vols = c.singles[coarse][id(c.sets[3])]
        g8 = (100 * c.map.to_numpy()).astype(np.int64)
        want = np.array([[g8[y, x] for x in (2, 3, 4, 4)] for y in (1, 2, 2, 2)])
        assert np.array_equal(vols[0][2], want), (vols[0][2], want)


@pytest.mark.parametrize("name, coarse, dims, fallback", [
    ("at_the_limit", dict(xy_search=0.5, xy_step=1.0 / 64), (64, 64, None), False),
    ("above_the_limit", dict(xy_search=65.0 / 128, xy_step=1.0 / 64), (65, 65, None), True),
    ("one_position", dict(xy_search=1.0 / 256, xy_step=1.0 / 128), (1, 1, None), False),
    ("one_angle", dict(angle_search=1.0 / 256, angle_step=1.0 / 128), (None, None, 1), False),
    ("other_cell_size", dict(grid_resolution=0.02), (None, None, None), False),
])
def test_lattice_shapes(small, name, coarse, dims, fallback):
    c = small
    per = _check_against_single(c.m, c.map, 0.0, 0.0, [c.sets[0]], True, True, coarse, fallback=fallback)
    assert per[0].status == 0 and per[0].response > 0
    for got, want in zip(per[0].coarse_dims, dims):
        assert want is None or got == want, (name, tuple(per[0].coarse_dims))


def test_python_batch_entry_on_the_seven_sets(small):
    from yag_slam_amd._capi import YmError
    c = small
    with pytest.raises(YmError):
        c.m.match_map_batch(c.map, 0.0, 0.0, c.sets)
    rs = c.m.match_map_batch(c.map, 0.0, 0.0, c.sets, strict=False)
    assert rs[4] is None and all(r is not None for i, r in enumerate(rs) if i != 4)
    one = c.m.match_scan_sets_with_map(c.map, 0.0, 0.0, c.sets[5], True, True)
    assert rs[5].response == one.response and rs[5].covariance == one.covariance
    assert sorted(k for k in rs[5].meta if k != "rigid_poses") == sorted(one.meta)
    for a, b in zip(rs[5].best_pose, one.best_pose):
        assert (a.x, a.y, a.euler[-1]) == (b.x, b.y, b.euler[-1])
    assert len(rs[5].meta["rigid_poses"]) == 64


# ---- 5: the tracker against the reference ------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def hall():
    """the map of tests/golden/map_track.npz, resident"""
    from yag_slam_amd.scan_matching import ScanMatcher
    z = np.load(os.path.join(GOLDEN, "map_track.npz"))
    c = _Small()
    c.z = z
    c.m = ScanMatcher(dict(resolution=float(z["res"]), smear_deviation=float(z["smear"]), range_threshold=12.0), semantics="yagpy")
    c.map = c.m.correlation_grid_from_occupancy(z["image"], occupied_value=0)
    c.ox, c.oy = float(z["ox"]), float(z["oy"])
    yield c
    c.map.close()
    c.m.close()


def _fixture_track(z):
    from yag_slam_amd.transform import Transform
    scans = []
    for r, o in zip(z["ranges"], z["odom"]):
        s = _scan(r, z["start_pose"], min_angle=float(z["sensor_min_angle"]), inc=float(z["sensor_angle_increment"]))
        s.odom_pose = Transform(float(o[0]), float(o[1]), 0.0, float(o[2]))
        scans.append(s)
    return scans


def test_tracker_against_the_reference_loop(hall):
    z = hall.z
    scans = _fixture_track(z)
    before = hall.m.debug_counters()
    res, done = hall.m.track_in_map(hall.map, hall.ox, hall.oy, scans, 1, True, True, None, float(z["min_response"]))
    after = hall.m.debug_counters()
    assert (after["map_kernel_items"] - before["map_kernel_items"], after["map_fallback_items"] - before["map_fallback_items"]) == (5, 0)
    assert done == 6 and res[0] is None
    # the prior of a step is the pose the scan has when it is matched: recomputed from the pose before it, as the library does
    prev = scans[0].corrected_pose
    for i in range(1, 6):
        prior = prev + (scans[i].odom_pose - scans[i - 1].odom_pose)
        got = (prior.x, prior.y, prior.euler[-1])
        if i == 1:
            assert got == tuple(z["priors"][0]), (got, z["priors"][0])
        np.testing.assert_allclose(got, z["priors"][i - 1], rtol=0, atol=1e-9)
        r = res[i]
        print("step", i, "response", r.response, "fixture", z["responses"][i - 1])
        assert r.meta["accepted"] == bool(z["accepted"][i - 1])
        assert abs(r.response - z["responses"][i - 1]) <= 1e-12
        assert abs(r.meta["coarse_response"] - z["coarse"][i - 1][0]) <= 1e-12
        np.testing.assert_allclose(np.array(r.covariance), z["covariances"][i - 1], rtol=1e-9, atol=1e-15)
        p = scans[i].corrected_pose
        np.testing.assert_allclose((p.x, p.y, p.euler[-1]), z["poses"][i], rtol=0, atol=1e-9)
        np.testing.assert_allclose((r.best_pose.x, r.best_pose.y, r.best_pose.euler[-1]), z["fine"][i - 1][1:4], rtol=0, atol=1e-9)
        prev = p


# ---- 6: the tracker against the per-scan loop, bit for bit -------------------------------------------------------------------
def _three_tracks():
    """tracks of 6, 4 and 1 scans in the hall; scan 2 of the second track has an odometry that jumps far off and back"""
    from yag_slam_amd import synth
    from yag_slam_amd.transform import Transform
    scene = synth.Scene()
    inc = synth.ANGLE_INCREMENT * (1081 - 1) / 180
    truths = [[(3.0 + 0.11 * i, 3.0 + 0.03 * i, 0.04 * i) for i in range(6)],
              [(5.2 - 0.08 * i, 2.2 + 0.06 * i, 1.0 + 0.05 * i) for i in range(4)],
              [(2.0, 2.0, -0.5)]]
    tracks = []
    for t, truth in enumerate(truths):
        tr = []
        for i, p in enumerate(truth):
            s = _scan(scene.scan_ranges(p, index=800 + 10 * t + i, n_beams=181, min_angle=synth.MIN_ANGLE, inc=inc), truth[0],
                      min_angle=synth.MIN_ANGLE, inc=inc)
            o = (p[0] + 0.02 * i, p[1] - 0.015 * i, p[2] + 0.015 * i)
            if t == 1 and i == 2:
                o = (p[0] + 1.3, p[1] + 0.9, p[2] + 1.1)
            s.odom_pose = Transform(o[0], o[1], 0.0, o[2])
            tr.append(s)
        tracks.append(tr)
    return tracks


def _python_loop(m, cmap, ox, oy, track, min_response):
    """the loop ym_map_track stands for, on the per-scan entry"""
    from yag_slam_amd.transform import Transform
    out = [None]
    for i in range(1, len(track)):
        prior = track[i - 1].corrected_pose + (track[i].odom_pose - track[i - 1].odom_pose)
        track[i].corrected_pose = prior
        r = m.match_scan_sets_with_map(cmap, ox, oy, [track[i]], True, True)
        ok = not r.response < min_response
        if ok:
            cc = r.meta["corrected_centre"]
            track[i].corrected_pose = Transform(cc[0], cc[1], 0.0, prior.euler[-1] + cc[2])
        out.append((r, ok))
    return out


def _pose(s):
    p = s.corrected_pose
    return (p.x, p.y, p.euler[-1])


def test_tracker_equals_the_per_scan_loop_bit_for_bit(hall):
    from yag_slam_amd.mapping import MapLocalizer
    want_tracks, got_tracks, one_by_one = _three_tracks(), _three_tracks(), _three_tracks()
    want = [_python_loop(hall.m, hall.map, hall.ox, hall.oy, t, 0.3) for t in want_tracks]
    before = hall.m.debug_counters()
    got = hall.m.track_in_map(hall.map, hall.ox, hall.oy, got_tracks, 1, True, True, None, 0.3)
    after = hall.m.debug_counters()
    assert (after["map_kernel_items"] - before["map_kernel_items"], after["map_fallback_items"] - before["map_fallback_items"]) == (8, 0)
    assert [d for _, d in got] == [6, 4, 1] and got[2][0] == [None]
    for t in range(3):
        for i in range(1, len(want_tracks[t])):
            (w, ok), g = want[t][i], got[t][0][i]
            print("track", t, "step", i, "response", g.response, "accepted", g.meta["accepted"])
            assert g.response == w.response and g.covariance == w.covariance and g.meta["accepted"] == ok
            assert (g.best_pose.x, g.best_pose.y, g.best_pose.euler[-1]) == tuple(w.meta["corrected_centre"])
            assert _pose(got_tracks[t][i]) == _pose(want_tracks[t][i])
    assert not got[1][0][2].meta["accepted"] and all(got[1][0][i].meta["accepted"] for i in (1, 3))
    assert all(r.meta["accepted"] for r in got[0][0][1:])
    # the same scan by scan through MapLocalizer
    for t in range(3):
        loc = MapLocalizer(hall.m, hall.map, hall.ox, hall.oy, min_response=0.3)
        lost = []
        for i, s in enumerate(one_by_one[t]):
            r = loc.process_scan(s)
            assert (r is None) == (i == 0)
            lost.append(loc.lost)
            if i:
                assert r.response == want[t][i][0].response and r.covariance == want[t][i][0].covariance
            assert _pose(s) == _pose(want_tracks[t][i])
        assert loc.last is one_by_one[t][-1] and len(loc.results) == len(one_by_one[t]) - 1
        assert lost == ([0, 0, 1, 0] if t == 1 else [0] * len(one_by_one[t]))


# ---- 7: locate_in_map(polish_top=4) ------------------------------------------------------------------------------------------
def test_locate_polishes_the_first_four_candidates_in_one_batch():
    from tests import locate_ref as R
    from yag_slam_amd import synth
    from yag_slam_amd.scan_matching import ScanMatcher
    m = ScanMatcher(dict(resolution=R.ROOM_RES, smear_deviation=R.ROOM_RES), semantics="yagpy")
    room = m.correlation_grid_from_occupancy(R.room_image(synth.Scene()), occupied_value=0)
    scan = synth.resident_scan(synth.Scene().scan_ranges(R.ROOM_TRUTH, index=950), (0.0, 0.0, 0.0))
    kw = dict(n_angles=R.ROOM_ANGLES, point_stride=6)
    ox, oy = R.ROOM_ORIGIN
    today = m.locate_in_map(room, ox, oy, [scan], refine=True, **kw)
    again = m.locate_in_map(room, ox, oy, [scan], refine=True, polish_top=1, **kw)
    assert again.response == today.response and again.covariance == today.covariance and "polished" not in again.meta
    assert _tf(again.best_pose[0]) == _tf(today.best_pose[0])
    before = m.debug_counters()
    r = m.locate_in_map(room, ox, oy, [scan], refine=True, polish_top=4, **kw)
    after = m.debug_counters()
    assert (after["map_kernel_items"] - before["map_kernel_items"], after["map_fallback_items"] - before["map_fallback_items"]) == (4, 0)
    pol = r.meta["polished"]
    assert len(pol) == 4
    res, step = R.ROOM_RES, 2 * math.pi / R.ROOM_ANGLES
    coarse = dict(xy_search=2 * res, xy_step=res / 4, angle_search=step, angle_step=step / 20, grid_resolution=res)
    for cand, p in zip(r.meta["candidates"][:4], pol):
        c = scan.copy()
        c.corrected_pose = cand.poses[0]
        one = m.match_scan_sets_with_map(room, ox, oy, [c], True, True, coarse=coarse)
        assert p.response == one.response and p.covariance == one.covariance
        assert p.meta["corrected_centre"] == one.meta["corrected_centre"] and p.meta["centre"] == one.meta["centre"]
    best = max(range(4), key=lambda i: (pol[i].response, -i))
    assert r.meta["polished_index"] == best and r.response == pol[best].response
    assert _tf(r.best_pose[0]) == _tf(pol[best].best_pose[0])
    assert r.response >= today.response  # (candidate 0 is among the four)
    room.close()
    m.close()


def _tf(p):
    return (p.x, p.y, p.euler[-1])
