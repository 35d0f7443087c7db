"""Host side of the segment graph (yag_slam_amd/splicing.py segment_* / map_to_graph / map_to_graphslam, mapping.PoseBuckets
.near_ordered, LoopClosingMapper.splice_first_scan): the numpy statement of the boundary and window rules against the
reference's recorded results (tests/golden/segments.npz), the argument checks that run before any device work, the ordered
pose query against the reference's search restated, and the bookkeeping with stubs in place of the device."""
import hashlib
import os
import subprocess
import sys

import numpy as np
import pytest

from tests.util import GOLDEN


@pytest.fixture(scope="module")
def fx():
    return np.load(os.path.join(GOLDEN, "segments.npz"), allow_pickle=False)


def host_boundaries(lab):
    """find_boundaries(lab) with its defaults as include/yagmatch.h states it: the maximum and the minimum over the pixel and
    its 4 neighbours inside the image differ"""
    lab = np.asarray(lab)
    lo, hi = lab.copy(), lab.copy()
    for src, dst in ((np.s_[1:, :], np.s_[:-1, :]), (np.s_[:-1, :], np.s_[1:, :]), (np.s_[:, 1:], np.s_[:, :-1]), (np.s_[:, :-1], np.s_[:, 1:])):
        lo[dst] = np.minimum(lo[dst], lab[src])
        hi[dst] = np.maximum(hi[dst], lab[src])
    return lo != hi


def host_pair_table(lab):
    """ym_segments_pairs as include/yagmatch.h states it -> (pairs, counts, first_index)"""
    lab = np.asarray(lab)
    h, w = lab.shape
    table = {}
    for y, x in zip(*np.where(host_boundaries(lab))):
        if y < 2 or x < 2:
            continue
        u = [int(v) for v in np.unique(lab[y - 2:y + 2, x - 2:x + 2]) if v]
        if len(u) == 2:
            e = table.setdefault((u[0] - 1, u[1] - 1), [0, int(y) * w + int(x)])
            e[0] += 1
    keys = list(table)
    return (np.array(keys, dtype=np.int32).reshape(-1, 2), np.array([table[k][0] for k in keys], dtype=np.int32),
            np.array([table[k][1] for k in keys], dtype=np.int64))


def test_the_stated_rules_reproduce_the_recorded_reference(fx):
    for name in fx["names"]:
        lab = fx[name + "_labels"]
        assert np.array_equal(host_boundaries(lab), fx[name + "_mask"]), name
        pairs, counts, first = host_pair_table(lab)
        assert np.array_equal(pairs, fx[name + "_pairs"]) and np.array_equal(counts, fx[name + "_pair_counts"])
        assert np.array_equal(first, fx[name + "_pair_first"])
        # an edge is a pair counted more than 3 times, in the order of the first index: create_edges' list
        assert np.array_equal(pairs[counts > 3], fx[name + "_edges"]), name
        # determine_centroids = one float64 division of the exact integer sums
        k = int(lab.max())
        assert len(fx[name + "_centroids"]) == k
        cx, cy = fx[name + "_sum_x"][1:] / fx[name + "_count"][1:], fx[name + "_sum_y"][1:] / fx[name + "_count"][1:]
        assert np.array_equal(np.stack([cx, cy], axis=1).reshape(-1, 2), fx[name + "_centroids"]), name
    # what the fixture was built to hold
    counts = set(fx["walls_pair_counts"].tolist())
    assert {2, 3, 4} <= counts
    assert len(fx["one_centroids"]) == 0 and len(fx["one_edges"]) == 0 and fx["one_labels"].shape == (1, 1)
    assert fx["three_labels"].shape == (3, 3)
    assert (fx["raytrace_count"][1:] == 1).sum() >= 5 and fx["raytrace_labels"][1, 1] == 2
    b = fx["borders_labels"]
    assert b[0].any() and b[-1].any() and b[:, 0].any() and b[:, -1].any()


def test_argument_checks_run_before_any_device_work(monkeypatch):
    from yag_slam_amd import _capi, splicing

    def no_device():
        raise AssertionError("the library was reached")
    monkeypatch.setattr(_capi, "lib", no_device)
    ok = np.zeros((4, 4), dtype=np.int32)
    for bad in (np.zeros((4, 4), dtype=np.float32), np.zeros((2, 3, 4), dtype=np.int32), np.zeros(5, dtype=np.int32),
                np.zeros((0, 4), dtype=np.int32), np.zeros((4, 4), dtype=bool)):
        for fn in (splicing.segment_centroids, splicing.segment_edges, splicing.SegmentMap):
            with pytest.raises(ValueError, match="2-D integer"):
                fn(bad)
    wide = np.lib.stride_tricks.as_strided(np.zeros(1, dtype=np.int32), shape=(2, 65537), strides=(0, 0))
    with pytest.raises(ValueError, match="65536"):
        splicing.segment_centroids(wide)
    with pytest.raises(ValueError, match="int32"):
        splicing.segment_edges(np.array([[0, 2 ** 31]], dtype=np.int64))
    with pytest.raises(ValueError, match="int32"):
        splicing.segment_edges(np.array([[0, 2 ** 32 - 1]], dtype=np.uint32))
    im = np.full((4, 4), 254, dtype=np.uint8)
    with pytest.raises(ValueError, match="layout"):
        splicing.map_to_graph(im, 0.05, (0, 0), ok, layout="pixels")
    with pytest.raises(ValueError, match="shape"):
        splicing.map_to_graph(im, 0.05, (0, 0), np.zeros((4, 5), dtype=np.int32))


def test_label_image_is_converted_once():
    from yag_slam_amd.splicing import _label_image
    a = np.arange(12, dtype=np.int32).reshape(3, 4)
    assert _label_image(a) is a                                  # already int32, unit column stride
    pad = np.zeros((3, 9), dtype=np.int32)
    assert _label_image(pad[:, :4]).base is pad                  # a padded pitch goes as it is
    for other in (a.astype(np.int64), a.astype(np.uint8), a.T, a[:, ::2], a.astype(np.int64)[::2, ::2]):
        got = _label_image(other)
        assert got.dtype == np.int32 and got.flags["C_CONTIGUOUS"] and np.array_equal(got, other)


def _reference_search(buckets_in_order, res, pose, radius):
    """crude_radius_search (helpers.py:420-431) restated: every bucket in insertion order, corner within radius + res"""
    r2 = (radius + res) ** 2
    out = []
    for (ix, iy), elements in buckets_in_order:
        if (float(ix) * res - pose.x) ** 2 + (float(iy) * res - pose.y) ** 2 < r2:
            out.extend(elements)
    return out


def test_pose_buckets_ordered_query_is_the_references_search():
    from tests.util import PlainPose
    from yag_slam_amd.mapping import PoseBuckets

    class S:
        def __init__(self, num, pose):
            self.num, self.corrected_pose = num, pose
    rng = np.random.default_rng(5)
    for res in (1.0, 3.0, 0.7):
        pb = PoseBuckets(res)
        hmap = {}  # the reference's table, built as add_new_element builds it
        scans = [S(i, PlainPose(*rng.uniform(-20, 20, 2), 0.0)) for i in range(400)]
        for s in scans:
            pb.add(s)
            hmap.setdefault((int(s.corrected_pose.x / res), int(s.corrected_pose.y / res)), []).append(s)
        for _ in range(60):
            q = PlainPose(*rng.uniform(-25, 25, 2), 0.0)
            radius = float(rng.choice([0.0, 0.5, 2.0, 5.0, 11.0]))
            got = pb.near_ordered(q, radius)
            want = _reference_search(list(hmap.items()), res, q, radius)
            assert [s.num for s in got] == [s.num for s in want]
            assert sorted(s.num for s in pb.near(q, radius)) == sorted(s.num for s in got)
        # after a rebuild the order is that of the rebuilt table
        pb.rebuild(scans[::-1])
        hmap = {}
        for s in scans[::-1]:
            hmap.setdefault((int(s.corrected_pose.x / res), int(s.corrected_pose.y / res)), []).append(s)
        q = PlainPose(1.0, -2.0, 0.0)
        got = [s.num for s in pb.near_ordered(q, 5.0)]
        assert got and got == [s.num for s in _reference_search(list(hmap.items()), res, q, 5.0)]


class _Scan:
    def __init__(self, num, x, y):
        from yag_slam_amd.transform import Transform
        self.num = num
        self.corrected_pose = Transform(x, y, 0.0, 0.0)
        self.odom_pose = Transform(x, y, 0.0, 0.0)


def test_map_to_graphslam_bookkeeping_with_a_stub_for_the_device(monkeypatch):
    from yag_slam_amd import splicing
    from yag_slam_amd.mapping import LoopClosingMapper
    scans = [_Scan(i, 0.5 * i, 0.25 * i) for i in range(6)]
    edges = [(0, 1), (1, 4), (2, 3)]
    seen = {}

    def stub(map_image, resolution, origin, segments, layout="reference", device=0):
        seen.update(layout=layout, device=device, resolution=resolution, origin=origin)
        return scans, edges
    monkeypatch.setattr(splicing, "map_to_graph", stub)
    mp = LoopClosingMapper(None, None)
    assert splicing.map_to_graphslam(mp, None, 0.05, (1.0, 2.0), None, layout="world", device=3) is mp
    assert seen == dict(layout="world", device=3, resolution=0.05, origin=(1.0, 2.0))
    assert mp.scans == scans and mp.running_scans == [] and mp.results == []
    assert [c[:2] for c in mp.constraints] == edges
    for (a, b, mean, cov) in mp.constraints:
        assert np.array_equal(cov, np.identity(3) * 10 ** -12)
        assert (mean.x, mean.y) == pytest.approx((0.5 * (b - a), 0.25 * (b - a)))
    assert mp.adjacent == [{1}, {0, 4}, {3}, {2}, {1}, set()]  # scan 5 has no edge and stays a vertex
    assert sorted(s.num for s in mp.index.near(scans[0].corrected_pose, 50)) == list(range(6))
    with pytest.raises(ValueError, match="empty"):
        splicing.map_to_graphslam(mp, None, 0.05, (1.0, 2.0), None)


def test_splice_first_scan_bookkeeping_with_a_stub_matcher():
    from yag_slam_amd.mapping import LoopClosingMapper
    from yag_slam_amd.transform import Transform

    class Result:
        def __init__(self, pose):
            self.best_pose, self.covariance, self.response = pose, [[1e-3, 0, 0], [0, 2e-3, 0], [0, 0, 3e-3]], 0.8

    class Matcher:
        def __init__(self):
            self.calls = []

        def match_scan(self, query, base, penalty=True, do_fine=False):
            self.calls.append((query, list(base), penalty, do_fine))
            return Result(Transform(1.1, 0.9, 0.0, 0.2))
    m = Matcher()
    mp = LoopClosingMapper(m, None, loop_search_dist=3)
    live = _Scan(None, 1.0, 1.0)
    with pytest.raises(ValueError, match="no map"):
        mp.splice_first_scan(live)
    # buckets are first filled far away, then near: the reference's candidates[0] is the first scan of the first bucket
    for i, (x, y) in enumerate([(40.0, 40.0), (4.0, 1.0), (1.0, 1.5), (4.5, 1.2), (-30.0, 2.0)]):
        mp.add_vertex(_Scan(i, x, y))
    far = _Scan(None, 300.0, 300.0)
    with pytest.raises(ValueError, match="no scan"):
        mp.splice_first_scan(far)
    assert far.num is None and len(mp.scans) == 5 and not m.calls and mp.running_scans == []
    res = mp.splice_first_scan(live)
    (query, base, penalty, do_fine), = m.calls
    assert query is live and [s.num for s in base] == [1, 3, 2] and penalty is True and do_fine is True
    assert res.response == 0.8 and live.corrected_pose is res.best_pose
    assert live.num == 5 and mp.scans[5] is live and mp.running_scans == [live]
    assert mp.constraints == [(5, 1, mp.constraints[0][2], res.covariance)] and mp.adjacent[5] == {1} and 5 in mp.adjacent[1]
    # process_scan continues: the vertex list and num agree
    nxt = _Scan(None, 1.2, 1.0)
    r2, closed = mp.process_scan(nxt)
    assert nxt.num == 6 and len(mp.scans) == 7 and mp.running_scans == [live, nxt] and closed is False


@pytest.mark.skipif(not (os.path.isdir("/root/reference") and os.environ.get("YM_REGENERATE_GOLDENS") == "1"),
                    reason="opt-in (YM_REGENERATE_GOLDENS=1) and only where the reference is: the build container")
def test_segments_golden_regenerates_bit_identically():
    path = os.path.join(GOLDEN, "segments.npz")
    before = hashlib.sha256(open(path, "rb").read()).hexdigest()
    subprocess.check_call([sys.executable, os.path.join(GOLDEN, "make_golden_segments.py")], stdout=subprocess.DEVNULL,
                          stderr=subprocess.DEVNULL)
    assert hashlib.sha256(open(path, "rb").read()).hexdigest() == before


def test_splice_first_scan_leaves_everything_as_it_was_when_the_matcher_raises():
    from yag_slam_amd.mapping import LoopClosingMapper

    class Failing:
        def match_scan(self, query, base, penalty=True, do_fine=False):
            assert query.num == 2  # the node's order: the num is set before the match
            raise RuntimeError("unable to find best position")
    mp = LoopClosingMapper(Failing(), None, loop_search_dist=3)
    for i in range(2):
        mp.add_vertex(_Scan(i, 1.0 + i, 1.0))
    for live in (_Scan(17, 1.2, 1.1), _Scan(None, 1.2, 1.1)):
        if live.num is None:
            del live.num
        before = getattr(live, "num", "absent")
        with pytest.raises(RuntimeError):
            mp.splice_first_scan(live)
        assert getattr(live, "num", "absent") == before
        assert len(mp.scans) == 2 and mp.constraints == [] and mp.running_scans == []
