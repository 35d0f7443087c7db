"""The segment graph of a prior map on the device (include/yagmatch.h ym_segments_*, yag_slam_amd/splicing.py
segment_centroids / segment_edges / map_to_graph / map_to_graphslam, mapping.LoopClosingMapper.splice_first_scan) against
the reference's determine_centroids and create_edges as recorded in tests/golden/segments.npz
(tests/golden/make_golden_segments.py): integers, float64 centroids, the boundary mask and the pair table all exactly equal;
then the ROS node's "start in a prior map" sequence end to end in this package's own frame."""
import ctypes as C
import math
import os

import numpy as np
import pytest

from tests.util import GOLDEN

pytestmark = pytest.mark.gpu

CASES = ["walls", "small", "raytrace", "borders", "one", "three"]


@pytest.fixture(scope="module")
def fx():
    z = np.load(os.path.join(GOLDEN, "segments.npz"), allow_pickle=False)
    assert list(z["names"]) == CASES
    return z


def _assert_table(got, fx, name):
    pairs, counts, first = got
    assert pairs.dtype == np.int32 and counts.dtype == np.int32 and first.dtype == np.int64
    assert np.array_equal(pairs, fx[name + "_pairs"]), name
    assert np.array_equal(counts, fx[name + "_pair_counts"]), name
    assert np.array_equal(first, fx[name + "_pair_first"]), name


def _assert_stats(got, fx, name):
    for g, key in zip(got, ("_count", "_sum_x", "_sum_y")):
        assert g.dtype == np.int64 and np.array_equal(g, fx[name + key]), (name, key)


def _assert_centroids(cent, fx, name):
    want = fx[name + "_centroids"]
    assert sorted(cent) == list(range(len(want)))
    for i, (x, y) in enumerate(want):
        assert cent[i][0] == x and cent[i][1] == y, (name, i, cent[i], (x, y))  # float64 ==: one division of exact sums


@pytest.mark.parametrize("name", CASES)
def test_counts_sums_and_centroids_are_the_references(fx, name):
    from yag_slam_amd.splicing import SegmentMap, segment_centroids
    lab = fx[name + "_labels"]
    with SegmentMap(lab) as sm:
        assert sm.label_range() == (int(lab.min()), int(lab.max()))
        _assert_stats(sm.stats(int(lab.max()) + 1), fx, name)
        # more room than labels: the tail stays zero
        wide = sm.stats(int(lab.max()) + 8)
        assert all(np.array_equal(w[:-7], fx[name + k]) and not w[-7:].any() for w, k in zip(wide, ("_count", "_sum_x", "_sum_y")))
    _assert_centroids(segment_centroids(lab), fx, name)


@pytest.mark.parametrize("name", CASES)
def test_boundary_mask_is_find_boundaries(fx, name):
    from yag_slam_amd.splicing import SegmentMap
    with SegmentMap(fx[name + "_labels"]) as sm:
        mask = sm.boundaries()
    assert mask.dtype == bool and np.array_equal(mask, fx[name + "_mask"]), int((mask != fx[name + "_mask"]).sum())


@pytest.mark.parametrize("name", CASES)
def test_pair_table_and_edges_are_the_references(fx, name):
    from yag_slam_amd.splicing import SegmentMap, segment_edges
    lab = fx[name + "_labels"]
    with SegmentMap(lab) as sm:
        _assert_table(sm.pairs(), fx, name)
    edges = segment_edges(lab)
    assert edges == [tuple(e) for e in fx[name + "_edges"].tolist()]
    assert all(type(a) is int and type(b) is int for a, b in edges)
    # min_count moves the threshold: 0 keeps every pair
    assert segment_edges(lab, min_count=0) == [tuple(p) for p in fx[name + "_pairs"].tolist()]


@pytest.mark.parametrize("name", ["walls", "borders", "small"])
def test_a_table_that_starts_too_small_grows_to_the_same_answer(fx, name):
    """table_slots = 16 cannot hold the pairs: the library counts again in a larger table (or reports the error), it never
    returns a shorter table"""
    from yag_slam_amd import _capi
    from yag_slam_amd.splicing import SegmentMap
    assert len(fx["walls_pairs"]) > 16 and len(fx["borders_pairs"]) > 16
    with SegmentMap(fx[name + "_labels"]) as sm:
        try:
            got = sm.pairs(table_slots=16)
        except _capi.YmError as e:
            assert e.code == -4, e
        else:
            _assert_table(got, fx, name)


def test_other_dtypes_strides_and_pitches(fx):
    from yag_slam_amd.splicing import SegmentMap, segment_centroids, segment_edges
    for name in ("walls", "borders"):
        lab = fx[name + "_labels"]
        h, w = lab.shape
        # a non-contiguous int64 view: every second column and row of a larger array
        big = np.full((2 * h, 2 * w), 77, dtype=np.int64)
        big[::2, ::2] = lab
        view = big[::2, ::2]
        assert not view.flags["C_CONTIGUOUS"] and view.dtype == np.int64
        # a padded pitch: int32 rows of w + 13 elements, the padding holds labels that must never be read
        pad = np.full((h, w + 13), 999999, dtype=np.int32)
        pad[:, :w] = lab
        pitched = pad[:, :w]
        assert pitched.strides[0] == 4 * (w + 13)
        for arr in (view, pitched, lab.astype(np.uint8), lab.astype(np.int16)):
            with SegmentMap(arr) as sm:
                assert sm.label_range() == (0, int(lab.max()))
                _assert_stats(sm.stats(int(lab.max()) + 1), fx, name)
                assert np.array_equal(sm.boundaries(), fx[name + "_mask"])
                _assert_table(sm.pairs(), fx, name)
            _assert_centroids(segment_centroids(arr), fx, name)
            assert segment_edges(arr) == [tuple(e) for e in fx[name + "_edges"].tolist()]


def test_two_calls_on_one_handle_agree(fx):
    from yag_slam_amd.splicing import SegmentMap
    with SegmentMap(fx["walls_labels"]) as sm:
        for _ in range(2):
            _assert_stats(sm.stats(61), fx, "walls")
            _assert_table(sm.pairs(), fx, "walls")
            _assert_table(sm.pairs(table_slots=64), fx, "walls")
            assert np.array_equal(sm.boundaries(), fx["walls_mask"])


def test_widths_that_are_no_multiple_of_the_tile(fx):
    """sub-images of every width 1 .. 9 and 61 .. 70 and a few heights: against the numpy statement of the rule"""
    from tests.test_segments_host import host_pair_table, host_boundaries
    from yag_slam_amd.splicing import SegmentMap
    lab = fx["walls_labels"]
    for w in list(range(1, 10)) + list(range(61, 71)) + [127, 129]:
        for h in (1, 2, 3, 15, 17, 33):
            sub = np.ascontiguousarray(lab[40:40 + h, 30:30 + w])
            with SegmentMap(sub) as sm:
                k = int(sub.max())
                count, sx, sy = sm.stats(k + 1)
                assert np.array_equal(count, np.bincount(sub.ravel(), minlength=k + 1)), (w, h)
                yy, xx = np.mgrid[0:h, 0:w]
                assert np.array_equal(sx, np.bincount(sub.ravel(), weights=xx.ravel(), minlength=k + 1).astype(np.int64))
                assert np.array_equal(sy, np.bincount(sub.ravel(), weights=yy.ravel(), minlength=k + 1).astype(np.int64))
                assert np.array_equal(sm.boundaries(), host_boundaries(sub)), (w, h)
                want = host_pair_table(sub)
                got = sm.pairs()
                assert all(np.array_equal(g, t) for g, t in zip(got, want)), (w, h)


def test_many_labels_in_one_tile_overflow_the_block_table_exactly():
    """every pixel its own label: a 64 x 64 tile holds 4096 labels, the block's 128-entry table overflows into the global sums"""
    from yag_slam_amd.splicing import SegmentMap
    h, w = 70, 131
    lab = np.arange(h * w, dtype=np.int32).reshape(h, w)
    with SegmentMap(lab) as sm:
        count, sx, sy = sm.stats(h * w)
    yy, xx = np.mgrid[0:h, 0:w]
    assert (count == 1).all() and np.array_equal(sx, xx.ravel()) and np.array_equal(sy, yy.ravel())


def test_map_to_graph_reference_layout_is_the_references(fx):
    from yag_slam_amd.splicing import REFERENCE_SENSOR, map_to_graph
    rt = np.load(os.path.join(GOLDEN, "raytrace.npz"), allow_pickle=False)
    scans, edges = map_to_graph(rt["image"], float(rt["resolution"]), tuple(rt["origin"]), fx["raytrace_labels"], layout="reference")
    assert edges == [tuple(e) for e in fx["raytrace_edges"].tolist()]
    assert np.array_equal(fx["raytrace_centroids"], rt["centroids"])
    want = rt["graph_ranges"]
    assert len(scans) == len(want)
    for s, r, p, num in zip(scans, want, rt["graph_poses"], rt["graph_nums"]):
        assert s.ranges.shape == (1439,)
        assert np.array_equal(s.ranges == 100, r == 100)
        np.testing.assert_allclose(s.ranges, r, rtol=1e-6, atol=0)
        pose = s.corrected_pose
        assert (pose.x, pose.y, pose.euler[-1]) == (p[0], p[1], p[2])
        assert s.num == num
        assert (s.min_angle, s.max_angle, s.angle_increment, s.min_range, s.max_range, s.range_threshold) == REFERENCE_SENSOR
        assert s._native is not None and s._native_device == 0
    assert (scans[3].ranges == 100).all()


def test_error_paths(fx):
    from yag_slam_amd import _capi
    from yag_slam_amd.splicing import SegmentMap, map_to_graph, segment_centroids, segment_edges
    L = _capi.lib()
    lab = fx["small_labels"]
    k = int(lab.max())
    lp, ip = C.POINTER(C.c_int64), C.POINTER(C.c_int32)
    with SegmentMap(lab) as sm:
        # a label >= n_labels: an error, nothing written
        out = [np.full(k, -7, dtype=np.int64) for _ in range(3)]
        rc = L.ym_segments_stats(sm._h, k, *[o.ctypes.data_as(lp) for o in out])
        assert rc == -1 and "[0, %d)" % k in _capi.last_error()
        assert all((o == -7).all() for o in out)
        # null pointers
        assert L.ym_segments_stats(None, k + 1, *[o.ctypes.data_as(lp) for o in out]) == -1
        assert L.ym_segments_stats(sm._h, k + 1, None, out[1].ctypes.data_as(lp), out[2].ctypes.data_as(lp)) == -1
        assert L.ym_segments_boundaries(sm._h, None, lab.size) == -1
        assert L.ym_segments_pairs(sm._h, 0, 4, None, None, None, None) == -1
        assert not L.ym_segments_create(0, None, 4, 4, 4) and "label image" in _capi.last_error()
        # a mask buffer that is too short
        short = np.full(lab.size - 1, 9, dtype=np.uint8)
        assert L.ym_segments_boundaries(sm._h, short.ctypes.data_as(C.POINTER(C.c_uint8)), short.size) == -1 and (short == 9).all()
        # cap too small: an error, *n_pairs = the needed size, nothing else written
        need = len(fx["small_pairs"])
        assert need > 2
        pairs, counts, first = np.full((2, 2), -7, dtype=np.int32), np.full(2, -7, dtype=np.int32), np.full(2, -7, dtype=np.int64)
        n = C.c_int32(-7)
        rc = L.ym_segments_pairs(sm._h, 0, 2, pairs.ctypes.data_as(ip), counts.ctypes.data_as(ip), first.ctypes.data_as(lp), C.byref(n))
        assert rc == -1 and n.value == need
        assert (pairs == -7).all() and (counts == -7).all() and (first == -7).all()
        # the Python side retries with the size it was told
        _assert_table(sm.pairs(cap=2), fx, "small")
    # a negative label
    neg = lab.copy()
    neg[5, 5] = -3
    with SegmentMap(neg) as sm:
        assert sm.label_range()[0] == -3
        with pytest.raises(_capi.YmError):
            sm.stats(k + 1)
        with pytest.raises(_capi.YmError):
            sm.pairs()
    with pytest.raises(ValueError, match="negative"):
        segment_centroids(neg)
    with pytest.raises(ValueError, match="negative"):
        segment_edges(neg)
    with pytest.raises(ValueError, match="negative"):
        map_to_graph(np.full(lab.shape, 254, dtype=np.uint8), 0.05, (0.0, 0.0), neg)
    # no zero pixel: the reference would drop segment 1
    with pytest.raises(ValueError, match="label 0"):
        segment_centroids(np.where(lab == 0, 1, lab))
    # a gap in the labels
    gap = np.where(lab == 3, 0, lab)
    assert k > 3
    with pytest.raises(ValueError, match="gap"):
        segment_centroids(gap)
    with pytest.raises(ValueError, match="gap"):
        map_to_graph(np.full(lab.shape, 254, dtype=np.uint8), 0.05, (0.0, 0.0), gap)
    with pytest.raises(ValueError, match="gap"):
        segment_centroids(np.array([[0, 1], [10 ** 6, 1]]))
    with pytest.raises(_capi.YmError):
        SegmentMap(lab, device=99)


def _room_with_segments():
    from tests.test_gpu_raytrace import _rendered_room
    from yag_slam_amd.synth import seeded_partition
    scene, g = _rendered_room()
    im = g.image
    lab = seeded_partition(im.shape[0], im.shape[1], 48, 21) * (im == 255)
    _, inv = np.unique(lab, return_inverse=True)  # labels 0 and 1 .. K without gaps (a seed's cell may hold no free pixel)
    return scene, g, inv.reshape(im.shape)


def test_ingest_a_rendered_room_and_splice_the_first_scan():
    """map_to_graphslam(layout="world") into a LoopClosingMapper, then the node's first scan (slam_node_ros1:234-253):
    bit-equal to the matcher called by hand, the node's bookkeeping, a pose nearer the truth, and process_scan goes on"""
    from yag_slam_amd import synth
    from yag_slam_amd.mapping import LoopClosingMapper
    from yag_slam_amd.scan_matching import ScanMatcher
    from yag_slam_amd.splicing import map_to_graphslam, segment_centroids, segment_edges
    from yag_slam_amd.transform import Transform
    scene, g, lab = _room_with_segments()
    res, origin = g.resolution, (g.offset.x, g.offset.y)
    seq = ScanMatcher(None, device=0)
    mp = LoopClosingMapper(seq, None)
    assert map_to_graphslam(mp, g.image, res, origin, lab, layout="world") is mp
    cent, edges = segment_centroids(lab), segment_edges(lab)
    k = int(lab.max())
    assert k > 20 and len(mp.scans) == k == len(cent) and len(edges) > k / 2
    assert mp.running_scans == [] and [s.num for s in mp.scans] == list(range(k))
    for i, s in enumerate(mp.scans):
        p = s.corrected_pose
        assert (p.x, p.y, p.euler[-1]) == (origin[0] + cent[i][0] * res, origin[1] + cent[i][1] * res, 0.0)
    assert [(c[0], c[1]) for c in mp.constraints] == edges
    assert all(np.array_equal(c[3], np.identity(3) * 1e-12) for c in mp.constraints)
    with pytest.raises(ValueError, match="empty"):
        map_to_graphslam(mp, g.image, res, origin, lab, layout="world")

    truth = (3.3, 2.7, 0.4)
    off = seq.config.search_size / 2 / 3  # well inside the sequential matcher's window
    initial = (truth[0] + off * math.cos(0.9), truth[1] + off * math.sin(0.9), truth[2] + 0.04)

    def live(index):
        s = synth.resident_scan(scene.scan_ranges(truth, index=index), truth)
        s.odom_pose = Transform(initial[0], initial[1], 0.0, initial[2])
        s.corrected_pose = Transform(initial[0], initial[1], 0.0, initial[2])
        return s

    # the matcher by hand on the same ordered candidates
    probe = live(950)
    candidates = mp.index.near_ordered(probe.odom_pose, 5)
    assert candidates and set(id(s) for s in candidates) == set(id(s) for s in mp.index.near(probe.odom_pose, 5))
    by_hand = seq.match_scan(probe, candidates, True, True)

    scan = live(950)
    n_constraints = len(mp.constraints)
    r = mp.splice_first_scan(scan)
    assert r.response == by_hand.response
    assert (r.best_pose.x, r.best_pose.y, r.best_pose.euler[-1]) == (by_hand.best_pose.x, by_hand.best_pose.y, by_hand.best_pose.euler[-1])
    assert np.array_equal(np.asarray(r.covariance), np.asarray(by_hand.covariance))
    bp = scan.corrected_pose
    assert (bp.x, bp.y, bp.euler[-1]) == (r.best_pose.x, r.best_pose.y, r.best_pose.euler[-1])
    # the node's bookkeeping
    assert scan.num == k and len(mp.scans) == k + 1 and mp.scans[-1] is scan
    assert len(mp.constraints) == n_constraints + 1 and mp.constraints[-1][:2] == (k, candidates[0].num)
    assert mp.running_scans == [scan]
    # nearer the truth than the initial pose
    d_initial = math.hypot(initial[0] - truth[0], initial[1] - truth[1])
    d_spliced = math.hypot(bp.x - truth[0], bp.y - truth[1])
    print("initial %.4f m, spliced %.4f m off the true position" % (d_initial, d_spliced))
    assert d_spliced < d_initial, (d_spliced, d_initial)
    # and mapping continues
    truth2 = (3.4, 2.75, 0.45)
    nxt = synth.resident_scan(scene.scan_ranges(truth2, index=951), truth2)
    nxt.odom_pose = Transform(initial[0] + 0.1, initial[1] + 0.05, 0.0, initial[2] + 0.05)
    res2, closed = mp.process_scan(nxt)
    assert res2 is not None and nxt.num == k + 1 and len(mp.scans) == k + 2 and mp.running_scans == [scan, nxt]

    # no candidate: a ValueError before anything changes
    mp2 = LoopClosingMapper(seq, None)
    map_to_graphslam(mp2, g.image, res, origin, lab, layout="world")
    far = live(952)
    far.odom_pose = Transform(500.0, 500.0, 0.0, 0.0)
    with pytest.raises(ValueError, match="no scan"):
        mp2.splice_first_scan(far)
    assert len(mp2.scans) == k and mp2.running_scans == [] and getattr(far, "num", None) != k
