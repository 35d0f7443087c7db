"""Virtual scans ray-traced on the device (include/yagmatch.h ym_raymap_*, yag_slam_amd/splicing.py) against the reference's
recorded rays (tests/golden/raytrace.npz, tests/golden/make_golden_raytrace.py) and against the numpy restatement of the
walk (tests/test_raytrace_host.py): end points bit for bit, lengths to the float32 norm the reference takes; then the
"start in a prior map" call of the ROS node (/root/reference/ros1/slam_node_ros1:242-248) in this package's own frame."""
import ctypes as C
import math
import os

import numpy as np
import pytest

from tests.test_raytrace_host import walk
from tests.util import GOLDEN

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def fx():
    return np.load(os.path.join(GOLDEN, "raytrace.npz"), allow_pickle=False)


def test_fixture_rays_are_bit_identical(fx):
    from yag_slam_amd.splicing import RayMap, trace_rays
    with RayMap(fx["image"]) as rm:
        ends, lengths = rm.trace(fx["sweep_viewpoints"], fx["sweep_angles"])
        assert rm.capped == 0
        assert ends.dtype == np.float32 and ends.shape == fx["sweep_ends"].shape
        assert np.array_equal(ends, fx["sweep_ends"])
        np.testing.assert_allclose(lengths, fx["sweep_lengths"], rtol=1e-6, atol=0)
    ends, lengths = trace_rays(fx["image"], fx["full_angles"], fx["full_viewpoint"][None])
    assert np.array_equal(ends[0], fx["full_ends"])
    np.testing.assert_allclose(lengths[0], fx["full_lengths"], rtol=1e-6, atol=0)


def test_virtual_scans_reference_layout_are_map_to_graphs(fx):
    from yag_slam_amd.splicing import REFERENCE_SENSOR, virtual_scans
    cent = {i: tuple(c) for i, c in enumerate(fx["centroids"])}  # determine_centroids' dict
    scans = virtual_scans(fx["image"], float(fx["resolution"]), tuple(fx["origin"]), cent, layout="reference")
    want = fx["graph_ranges"]
    assert len(scans) == len(want)
    for s, r, p, num in zip(scans, want, fx["graph_poses"], fx["graph_nums"]):
        assert s.ranges.shape == (1439,)
        assert np.array_equal(s.ranges == 100, r == 100)
        np.testing.assert_allclose(s.ranges, r, rtol=1e-6, atol=0)
        pose = s.corrected_pose
        assert (pose.x, pose.y, pose.euler[-1]) == (p[0], p[1], p[2])
        assert s.num == num
        assert (s.min_angle, s.max_angle, s.angle_increment, s.min_range, s.max_range, s.range_threshold) == REFERENCE_SENSOR
        assert s._native is not None and s._native_device == 0  # the twins exist (one ym_scans_create)
    assert (scans[3].ranges == 100).all()  # the centroid on an unknown pixel


def _random_map(seed, w=1021, h=767, pitch=1100):
    rng = np.random.default_rng(seed)
    buf = np.full((h, pitch), 254, dtype=np.uint8)
    buf[:, w:] = 0  # beyond the image: must never be read
    im = buf[:, :w]
    for _ in range(40):
        x0, y0 = rng.integers(0, w - 20), rng.integers(0, h - 20)
        ww, hh = rng.integers(2, 120), rng.integers(2, 120)
        im[y0:y0 + hh, x0:x0 + ww] = rng.choice([0, 205, 254, 211, 200])
    speck = rng.random((h, w)) < 0.002
    im[speck] = rng.choice(np.array([0, 179, 180, 181, 205, 209, 210, 211], dtype=np.uint8), size=int(speck.sum()))
    return im


@pytest.mark.parametrize("seed", [1, 2, 3])
def test_random_maps_bit_identical_to_the_walk(seed):
    from yag_slam_amd.splicing import REFERENCE_ANGLES, RayMap, direction_table
    im = _random_map(seed)
    assert im.strides[0] != im.shape[1] and im.shape[1] % 64 and im.shape[0] % 64
    h, w = im.shape
    rng = np.random.default_rng(100 + seed)
    vp = np.stack([rng.uniform(-0.49, w - 0.51, 64), rng.uniform(-0.49, h - 0.51, 64)], axis=1)
    vp[:4] = [[0.0, 0.0], [w - 1, h - 1], [0.5, h / 2], [w / 2, 1.5]]  # corners and ties
    with RayMap(im) as rm:
        for angles in (REFERENCE_ANGLES, rng.uniform(-400, 400, 97), np.array([0.0, 90.0, -90.0, 180.0, 45.0])):
            ends, lengths = rm.trace(vp, angles)
            assert rm.capped == 0
            want_e, want_l, _ = walk(im, vp, direction_table(angles))
            assert np.array_equal(ends, want_e), int((ends != want_e).any(axis=2).sum())
            np.testing.assert_allclose(lengths, want_l, rtol=1e-12, atol=0)


def test_edge_cases():
    from yag_slam_amd import _capi
    from yag_slam_amd.splicing import REFERENCE_ANGLES, RayMap, direction_table, virtual_scans
    im = np.full((50, 70), 254, dtype=np.uint8)
    im[20, 30] = 0
    im[25, 40] = 205
    cs = direction_table(REFERENCE_ANGLES)
    with RayMap(im) as rm:
        # a start on an occupied pixel takes one step
        ends, lengths = rm.trace_dirs([[30.0, 20.0]], cs)
        step = np.stack([(np.float32(30.0) + cs[:, 0]).astype(np.float32), (np.float32(20.0) + cs[:, 1]).astype(np.float32)], axis=1)
        assert np.array_equal(ends[0], step) and np.allclose(lengths, 1.0, rtol=0, atol=1e-5)
        # a start on an unknown pixel jumps 1000 pixels
        _, lengths = rm.trace_dirs([[40.0, 25.0]], cs)
        assert (lengths > 1000).all()
        # repeated traces are identical
        a = rm.trace_dirs([[10.0, 40.0], [33.3, 12.7]], cs)
        b = rm.trace_dirs([[10.0, 40.0], [33.3, 12.7]], cs)
        assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])
        # empty inputs: empty results, nothing launched
        e, l_ = rm.trace(np.zeros((0, 2)), REFERENCE_ANGLES)
        assert e.shape == (0, 1439, 2) and l_.shape == (0, 1439)
        e, l_ = rm.trace([[10.0, 10.0]], [])
        assert e.shape == (1, 0, 2) and l_.shape == (1, 0)
        # a start whose rounded pixel is outside the image is rejected and nothing is written
        L = _capi.lib()
        for bad in ([-0.51, 3.0], [3.0, 49.5], [69.6, 3.0], [float("nan"), 3.0]):
            st = np.array([[5.0, 5.0], bad], dtype=np.float64)
            out_e = np.full((2, 3, 2), -7.0, dtype=np.float32)
            out_l = np.full((2, 3), -7.0)
            capped = C.c_int64(-7)
            dp = C.POINTER(C.c_double)
            rc = L.ym_raymap_trace(rm._h, st.ctypes.data_as(dp), 2, cs[:3].ctypes.data_as(dp), 3,
                                   out_e.ctypes.data_as(C.POINTER(C.c_float)), out_l.ctypes.data_as(dp), C.byref(capped))
            assert rc == -1 and ("outside" in _capi.last_error() or "finite" in _capi.last_error())
            assert (out_e == -7).all() and (out_l == -7).all() and capped.value == -7
        with pytest.raises(_capi.YmError):
            rm.trace_dirs([[5.0, 5.0]], [[1.0, 1.0]])  # not a unit direction
        # the start's pixel is the float32 value's, half to even: 69.5 -> 70 is outside, 0.5 -> 0 inside
        rm.trace([[0.5, 0.5]], [0.0])
        with pytest.raises(_capi.YmError):
            rm.trace([[69.5, 3.0]], [0.0])
    # a free-only map: every ray ends at the border
    free = np.full((50, 70), 254, dtype=np.uint8)
    with RayMap(free) as rm:
        ends, _ = rm.trace_dirs([[10.0, 40.0], [35.5, 24.5], [1.0, 1.0]], cs)
        rx, ry = np.rint(ends[..., 0]), np.rint(ends[..., 1])
        assert ((rx < 1) | (ry < 1) | (rx >= 69) | (ry >= 49)).all() and rm.capped == 0
    with pytest.raises(_capi.YmError):
        RayMap(np.zeros((2, 65537), dtype=np.uint8))
    # reference layout: a centroid on an unknown pixel reads 100 everywhere, one in a free-only map never does
    assert (virtual_scans(im, 0.05, (0.0, 0.0), [(40.0, 25.0)], layout="reference")[0].ranges == 100).all()
    assert (virtual_scans(free, 0.05, (0.0, 0.0), [(10.0, 40.0)], layout="reference")[0].ranges < 20).all()


def test_world_layout_cell_centres_exact():
    """the frame of layout="world" (cell (c, r) centred at (ox + c res, oy + r res)) pinned on tests/test_raytrace_host.py's
    hand-made grid: readings exactly (wall - cell + 1) cells, the reference's extra step included"""
    from tests.test_raytrace_host import cell_centre_grid
    from yag_slam_amd.splicing import virtual_scans
    im, res, origin, view, want = cell_centre_grid()
    sensor = (0.0, math.pi, math.pi / 2, 0.0, 30.0, 20.0)
    s = virtual_scans(im, res, origin, [(view[0], view[1], 0.0)], layout="world", sensor=sensor, n_beams=3)[0]
    assert np.array_equal(s.ranges, want), (s.ranges, want)
    # heading pi / 2 turns the beams: 90, 180 and 270 degrees
    s = virtual_scans(im, res, origin, [(view[0], view[1], math.pi / 2)], layout="world", sensor=sensor, n_beams=2)[0]
    assert np.array_equal(s.ranges, want[1:]), (s.ranges, want[1:])


def test_per_viewpoint_directions_are_one_launch_of_the_same_walk():
    """trace_each (a direction table per viewpoint) = trace_dirs viewpoint by viewpoint, bit for bit; world layout uses it"""
    from yag_slam_amd.splicing import RayMap
    im = _random_map(4)
    rng = np.random.default_rng(7)
    vp = np.stack([rng.uniform(0, im.shape[1] - 1, 40), rng.uniform(0, im.shape[0] - 1, 40)], axis=1)
    a = rng.uniform(-math.pi, math.pi, 40)[:, None] + np.arange(300)[None, :] * 0.01
    dirs = np.stack([np.cos(a), np.sin(a)], axis=2)
    with RayMap(im) as rm:
        ends, lengths = rm.trace_each(vp, dirs)
        assert rm.capped == 0 and ends.shape == (40, 300, 2)
        for i in range(0, 40, 3):
            e1, l1 = rm.trace_dirs(vp[i:i + 1], dirs[i])
            assert np.array_equal(ends[i], e1[0]) and np.array_equal(lengths[i], l1[0])
        want_e = np.stack([walk(im, vp[i:i + 1], dirs[i])[0][0] for i in range(40)])
        assert np.array_equal(ends, want_e)


def _rendered_room():
    from yag_slam_amd import synth
    from yag_slam_amd.occupancy import create_occupancy_grid
    scene = synth.Scene()
    truth, _ = synth.loop_trajectory(40 * 12)
    poses = truth[::12]
    scans = [synth.resident_scan(scene.scan_ranges(p, index=700 + i), p) for i, p in enumerate(poses)]
    return scene, create_occupancy_grid(scans, 0.05, 20.0)


def test_world_layout_ranges_follow_the_rendered_map():
    from yag_slam_amd.splicing import REFERENCE_SENSOR, virtual_scan_block, virtual_scans
    scene, g = _rendered_room()
    res, origin = g.resolution, (g.offset.x, g.offset.y)
    poses = [(2.0, 2.0, 0.0), (4.0, 3.0, 0.7), (5.5, 3.5, -2.0), (3.2, 4.4, 3.0), (6.0, 1.8, 1.2)]
    scans = virtual_scans(g.image, res, origin, poses, layout="world")
    block = virtual_scan_block(g.image, res, origin, poses, layout="world")
    assert len(block) == len(poses) and np.array_equal(block.ranges, np.array([s.ranges for s in scans]))
    n = 1439
    for s, p in zip(scans, poses):
        assert s.ranges.shape == (n,) and (s.corrected_pose.x, s.corrected_pose.y, s.corrected_pose.euler[-1]) == p
        exact = scene.cast(p[0], p[1], p[2], n_beams=n, min_angle=REFERENCE_SENSOR[0], inc=REFERENCE_SENSOR[2])
        wall = exact < 20
        ok = np.abs(s.ranges - exact) <= 2 * res
        assert ok[wall].mean() >= 0.95, ok[wall].mean()


def test_start_in_a_prior_map_matches_against_virtual_scans():
    """slam_node_ros1:242-248: the first live scan, at a prior 0.15 m / 0.05 rad off, matched against the nearby virtual scans"""
    from yag_slam_amd import synth
    from yag_slam_amd.scan_matching import ScanMatcher
    from yag_slam_amd.splicing import virtual_scans
    from yag_slam_amd.transform import Transform
    scene, g = _rendered_room()
    res, origin = g.resolution, (g.offset.x, g.offset.y)
    grid = [(x, y, 0.0) for x in np.arange(1.5, 7.0, 0.5) for y in np.arange(1.5, 5.0, 0.5)]
    vscans = virtual_scans(g.image, res, origin, grid, layout="world")
    m = ScanMatcher(None, device=0)
    for k, truth in enumerate([(3.3, 2.7, 0.4), (5.1, 3.6, -1.1), (2.2, 4.2, 2.5)]):
        live = synth.resident_scan(scene.scan_ranges(truth, index=900 + k), truth)
        prior = (truth[0] + 0.15 * math.cos(0.3 + k), truth[1] + 0.15 * math.sin(0.3 + k), truth[2] + (0.05 if k % 2 else -0.05))
        live.corrected_pose = Transform(prior[0], prior[1], 0.0, prior[2])
        near = sorted(vscans, key=lambda s: math.hypot(s.corrected_pose.x - prior[0], s.corrected_pose.y - prior[1]))[:3]
        r = m.match_scan(live, near, True, True)
        bp = r.best_pose
        assert math.hypot(bp.x - truth[0], bp.y - truth[1]) <= 2 * res, (k, bp.x, bp.y, truth)
        assert abs(math.remainder(bp.euler[-1] - truth[2], 2 * math.pi)) <= math.radians(1.0), (k, bp.euler[-1], truth)
