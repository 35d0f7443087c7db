"""The map segmenter on the device (include/yagmatch.h ym_map_free_space / ym_segments_from_map / ym_segments_labels,
yag_slam_amd/splicing.py free_space / segment_map / SegmentMap.from_map and map_to_graph with segments=None) against
tests/segmenter_ref.py, the numpy / scipy restatement of DESIGN.md "Map segmenter": every integer and every label image
exactly equal, on the smallest shapes at which each stage can go wrong.

The spiral is this file's own drawing of the 170 x 170 corridor (14-pixel corridor, 3-pixel walls): with n_segments = 6 the
reference finds 33 components from 9 seeds of which 5 reach the default minimum size; the counts asserted are the
reference's, whatever they are, and that the components outnumber the seeds."""
import ctypes as C

import numpy as np
import pytest

from tests import segmenter_ref as ref

pytestmark = pytest.mark.gpu

INFO_KEYS = ("sum", "n_free", "n_segments", "step", "seeds", "iterations_run", "min_size")


def _random_image(shape, seed):
    return np.random.RandomState(seed).choice(np.array([0, 100, 200, 254, 255], np.uint8), size=shape, p=[.1, .05, .05, .3, .5])


def _sparse_image():
    r = np.random.RandomState(7)
    return np.where(r.rand(47, 61) < 0.9, 255, 0).astype(np.uint8)


# name -> (image, options): the inputs of the assignment and component tests
CASES = {
    "square": (lambda: ref.walled_square(94), dict(n_segments=4)),
    "floorplan131": (lambda: ref.floorplan(131, 197, 4), dict()),
    "sparse": (_sparse_image, dict(n_segments=150, close_size=3)),
    "pixels": (lambda: ref.walled_square(14, 254), dict(n_segments=196, close_size=3)),
    "spiral_all": (ref.spiral, dict(n_segments=6, min_size_div=1 << 30)),
    "spiral": (ref.spiral, dict(n_segments=6)),
    "floorplan240": (lambda: ref.floorplan(240, 320, 2), dict()),
    "floorplan384": (lambda: ref.floorplan(384, 512, 1), dict()),
}
_cache = {}


def want(name, **more):
    """the reference's (image, labels, info) of a case, computed once"""
    key = (name, tuple(sorted(more.items())))
    if key not in _cache:
        make, opts = CASES[name]
        im = make()
        labels, info = ref.segment(im, **dict(opts, **more))
        labels.setflags(write=False)
        _cache[key] = (im, labels, info)
    return _cache[key]


def got(name, **more):
    from yag_slam_amd.splicing import SegmentMap
    make, opts = CASES[name]
    if "stage" in more:
        more = dict(more, stage={ref.STAGE_FINAL: "final", ref.STAGE_ASSIGNED: "assigned"}[more["stage"]])
    with SegmentMap.from_map(make(), **dict(opts, **more)) as sm:
        return sm.labels(), sm.info


def _assert_info(info, winfo, final):
    for k in INFO_KEYS + (("segments", "unlabelled") if final else ()):
        assert info[k] == winfo[k], (k, info, winfo)


@pytest.mark.parametrize("shape", [(7, 5), (23, 40), (67, 130)])
@pytest.mark.parametrize("close_size", [3, 11])
def test_closing_and_sum(shape, close_size):
    from yag_slam_amd.splicing import free_space
    im = _random_image(shape, shape[0])
    closed, total, n_free = free_space(im, close_size)
    wc, wt, wn = ref.free_space(im, close_size)
    assert closed.dtype == np.uint8 and np.array_equal(closed, wc), int((closed != wc).sum())
    assert (total, n_free) == (wt, wn)


def test_closing_of_a_strided_view():
    from yag_slam_amd.splicing import free_space
    big = _random_image((70, 150), 3)
    view = big[2:69, 11:141]  # 67 x 130 with a pitch of 150 bytes
    assert view.strides == (150, 1)
    closed, total, n_free = free_space(view)
    wc, wt, wn = ref.free_space(np.ascontiguousarray(view))
    assert np.array_equal(closed, wc) and (total, n_free) == (wt, wn)


@pytest.mark.parametrize("iterations", [1, 2, 10])
@pytest.mark.parametrize("name", ["square", "floorplan131", "sparse", "pixels"])
def test_assignment_is_the_references(name, iterations):
    _, wl, winfo = want(name, iterations=iterations, stage=ref.STAGE_ASSIGNED)
    labels, info = got(name, iterations=iterations, stage=ref.STAGE_ASSIGNED)
    assert labels.dtype == np.int32 and np.array_equal(labels, wl), int((labels != wl).sum())
    _assert_info(info, winfo, False)


def test_the_cases_are_the_ones_meant():
    assert want("square", stage=ref.STAGE_ASSIGNED)[2]["step"] == 47
    assert list(np.bincount(want("square", stage=ref.STAGE_ASSIGNED)[1].reshape(-1))[1:]) == [2209] * 4
    i = want("floorplan131")[2]
    assert (i["n_segments"], i["step"], i["seeds"]) == (7, 51, 11)
    i = want("sparse")[2]
    assert (i["step"], i["seeds"]) == (4, 180)
    i = want("pixels")[2]
    assert (i["step"], i["seeds"], i["min_size"], i["segments"]) == (1, 196, 0, 196)
    i, j = want("spiral_all")[2], want("spiral")[2]
    assert i["components"] == i["segments"] > i["seeds"] == 9 and 0 < j["segments"] < i["segments"] and j["unlabelled"] > 0


@pytest.mark.parametrize("name", ["spiral_all", "spiral", "floorplan240", "floorplan131", "sparse", "pixels", "square"])
def test_components_and_numbering_are_the_references(name):
    _, wl, winfo = want(name)
    labels, info = got(name)
    assert labels.dtype == np.int32 and np.array_equal(labels, wl), int((labels != wl).sum())
    _assert_info(info, winfo, True)


def test_resident_handle_serves_stats_centroids_and_edges():
    from yag_slam_amd.splicing import SegmentMap, segment_centroids, segment_edges, segment_map
    im, wl, winfo = want("floorplan240")
    k = winfo["segments"]
    ys, xs = np.indices(wl.shape)
    with SegmentMap.from_map(im) as sm:
        assert sm.label_range() == (0, k)
        count, sum_x, sum_y = sm.stats(k + 1)
        pairs = sm.pairs()
    flat = wl.reshape(-1)
    assert np.array_equal(count, np.bincount(flat, minlength=k + 1))
    assert np.array_equal(sum_x, np.bincount(flat, weights=xs.reshape(-1), minlength=k + 1).astype(np.int64))
    assert np.array_equal(sum_y, np.bincount(flat, weights=ys.reshape(-1), minlength=k + 1).astype(np.int64))
    with SegmentMap(wl) as sm:
        for a, b in zip(pairs, sm.pairs()):
            assert np.array_equal(a, b)
    labels = segment_map(im)
    assert segment_centroids(labels) == segment_centroids(wl)
    assert segment_edges(labels) == segment_edges(wl)


def test_map_to_graph_segments_the_map_itself():
    from yag_slam_amd.mapping import LoopClosingMapper
    from yag_slam_amd.splicing import map_to_graph, map_to_graphslam
    im, wl, winfo = want("floorplan240")
    res, origin = 0.05, (-3.0, -2.0)
    scans, edges = map_to_graph(im, res, origin)
    wscans, wedges = map_to_graph(im, res, origin, segments=wl)
    assert edges == wedges and len(edges) > 0
    assert len(scans) == len(wscans) == winfo["segments"]
    for s, ws in zip(scans, wscans):
        assert np.array_equal(s.ranges, ws.ranges)
        p, wp = s.corrected_pose, ws.corrected_pose
        assert (p.x, p.y, p.euler[-1]) == (wp.x, wp.y, wp.euler[-1])
    mp = LoopClosingMapper(None, None)
    assert map_to_graphslam(mp, im, res, origin) is mp
    assert len(mp.scans) == winfo["segments"] and not mp.running_scans


def test_two_calls_return_the_same_labels():
    im, wl, _ = want("floorplan384")
    a, ia = got("floorplan384")
    b, ib = got("floorplan384")
    assert np.array_equal(a, b) and ia == ib
    assert np.array_equal(a, wl)


def test_error_paths_name_the_argument_and_write_nothing():
    from yag_slam_amd import _capi
    from yag_slam_amd.splicing import SegmentError, SegmentMap, segment_map
    L = _capi.lib()
    bp, lp = C.POINTER(C.c_uint8), C.POINTER(C.c_int64)
    im = ref.floorplan(131, 197, 4)
    h, w = im.shape
    ptr = im.ctypes.data_as(bp)

    def free_space(image, w_, close_size):
        closed = np.full((h, w), 9, np.uint8)
        total, n_free = C.c_int64(9), C.c_int64(9)
        rc = L.ym_map_free_space(0, image, w_, h, w, close_size, closed.ctypes.data_as(bp), C.byref(total), C.byref(n_free))
        assert rc == -1 and (closed == 9).all() and total.value == 9 and n_free.value == 9
        return _capi.last_error()

    def from_map(image, w_, **o):
        opts = _capi.YmSegmentOpts(o.get("n_segments", 0), 1.0, o.get("close_size", 11), 10, 4, 0)
        info = _capi.YmSegmentInfo()
        C.memset(C.byref(info), 9, C.sizeof(info))
        assert not L.ym_segments_from_map(0, image, w_, h, w, C.byref(opts), C.byref(info))
        assert bytes(info) == b"\x09" * C.sizeof(info)
        return _capi.last_error()

    assert "image" in free_space(None, w, 11) and "image" in from_map(None, w)
    assert "w 0" in free_space(ptr, 0, 11) and "w 0" in from_map(ptr, 0)
    assert "close_size 4" in free_space(ptr, w, 4) and "close_size 4" in from_map(ptr, w, close_size=4)
    # a map whose closed image sums to less than 600000: the rule gives no segment
    small = ref.walled_square(30)
    opts = _capi.YmSegmentOpts(0, 1.0, 11, 10, 4, 0)
    info = _capi.YmSegmentInfo()
    C.memset(C.byref(info), 9, C.sizeof(info))
    assert not L.ym_segments_from_map(0, small.ctypes.data_as(bp), 32, 32, 32, C.byref(opts), C.byref(info))
    assert "n_segments 0" in _capi.last_error() and bytes(info) == b"\x09" * C.sizeof(info)
    with pytest.raises(ValueError, match="n_segments 0"):
        segment_map(small)
    with pytest.raises(SegmentError, match="no free pixel"):
        SegmentMap.from_map(np.zeros((20, 20), np.uint8), n_segments=3)
    with pytest.raises(ValueError, match="uint8"):
        segment_map(im.astype(np.int32))
    buf = np.full(5, 9, np.int32)
    with SegmentMap.from_map(im) as sm:
        assert L.ym_segments_labels(sm._h, buf.ctypes.data_as(C.POINTER(C.c_int32)), 5) == -1 and (buf == 9).all()
        assert "labels" in _capi.last_error()


def test_a_map_without_a_zero_pixel_is_returned_as_it_is():
    """every pixel free and in one segment: no label 0, which map_to_graph refuses as it does for any such label image"""
    from yag_slam_amd.splicing import SegmentMap, map_to_graph, segment_map
    full = np.full((50, 49), 255, np.uint8)  # 624 750 // 600 000: one segment by the rule
    wl, winfo = ref.segment(full)
    assert winfo["segments"] == 1 and (wl == 1).all()
    assert np.array_equal(segment_map(full), wl)
    with SegmentMap.from_map(full) as sm:
        assert sm.label_range() == (1, 1) and sm.info["unlabelled"] == 0
    with pytest.raises(ValueError, match="label 0"):
        map_to_graph(full, 0.05, (0.0, 0.0))
