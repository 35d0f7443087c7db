"""Occupancy-grid rendering on the device (karto_scanmatcher.create_occupancy_grid as
/root/reference/yag_slam/graph_slam.py:341-342 and /root/reference/ros1/slam_node_ros1:187-202 use it) against the CPU
oracle's sequential restatement of open_karto's OccupancyGrid.  Counts are integers: the image must be identical.
Parity unpinned at the Karto boundary (no source, no vector in the reference tree); the codes 0 / 200 / 255 are the ones
the reference's ROS node reads.

The image hides almost every miscount (a cell reads 200 up to two passes, and 0 or 255 by a ratio), and the oracle is the
kernel's twin.  So the pass and hit counts themselves are read through the test hook (create_occupancy_grid(counts=True),
ym_occupancy_create_counted) and compared exactly with the independent restatement tests/occupancy_ref.py, on the fixtures
tests/test_occupancy_host.py builds, checks for rounding ties and cross-checks with the oracle."""
import ctypes as C

import numpy as np
import pytest

from tests.test_occupancy_host import EXACT_ON_DEVICE, LITERALS, expected, fixture, make_scan

pytestmark = pytest.mark.gpu


def _scans(n, dirty=False):
    from yag_slam_amd import synth
    scene = synth.Scene()
    truth, _ = synth.loop_trajectory(n * 12)
    poses = truth[::12]
    return scene, [synth.resident_scan(scene.scan_ranges(p, index=700 + i, dirty=dirty), p) for i, p in enumerate(poses)]


@pytest.mark.parametrize("res,rt,dirty", [(0.05, 12.0, False), (0.05, 3.0, True), (0.02, 20.0, True), (0.1, 2.5, False)])
def test_occupancy_grid_matches_oracle(res, rt, dirty):
    from oracle import oracle as orc
    from yag_slam_amd.occupancy import create_occupancy_grid
    scene, scans = _scans(40, dirty)
    g = create_occupancy_grid(scans, res, rt)
    want, (ox, oy) = orc.occupancy_grid(scans, res, rt)
    assert (g.height, g.width) == want.shape and g.image.shape == want.shape
    assert abs(g.offset.x - ox) <= 1e-12 and abs(g.offset.y - oy) <= 1e-12
    assert np.array_equal(g.image, want), int((g.image != want).sum())
    assert set(np.unique(g.image)) <= {0, 200, 255}
    if rt >= 12.0:
        # the room: walls occupied, interior free, and the grid spans what the scans saw (about 8 m x 6 m)
        assert abs(g.width * res - scene.width) < 0.3 and abs(g.height * res - scene.height) < 0.3
        free = (g.image == 255).mean()
        assert free > 0.5 and (g.image == 0).sum() > 2 * (scene.width + scene.height) / res * 0.5


def test_mapper_makes_the_occupancy_grid_like_graphslam():
    """graph_slam.py:341-342 `make_occupancy_grid(resolution, range_threshold)` on the driver, and the cleanup arithmetic of
    slam_node_ros1:190-202 applied to it (0 -> 100, 200 -> -1, 255 -> 0)"""
    from yag_slam_amd import synth
    from yag_slam_amd.mapping import LoopClosingMapper
    from yag_slam_amd.scan_matching import ScanMatcher
    truth, scans = synth.trajectory_scans(30)
    mp = LoopClosingMapper(ScanMatcher(), None)
    for s in scans:
        mp.process_scan(s)
    g = mp.make_occupancy_grid(resolution=0.05, range_threshold=12)
    im = g.image.astype("int16")
    im[im == 0] = 100
    im[im == 200] = -1
    im[im == 255] = 0
    assert set(np.unique(im)) <= {-1, 0, 100} and (im == 100).sum() > 200 and (im == 0).sum() > (im == 100).sum()
    assert g.image.shape == (g.height, g.width) and g.resolution == 0.05


# ------------------------------------------------------------------------------------------ counts, through the test hook
def _render(scans, res, rt, counts=True):
    from yag_slam_amd.occupancy import create_occupancy_grid
    return create_occupancy_grid(scans, res, rt, counts=counts)


def _assert_is(g, want, what):
    """a counted rendering against (image, passes, hits, (off_x, off_y)): sizes, counts and image exactly, offsets to 1e-12"""
    image, passes, hits, (ox, oy) = want
    assert (g.height, g.width) == image.shape, (what, g.height, g.width, image.shape)
    assert g.passes.dtype == np.uint32 and g.hits.dtype == np.uint32 and g.passes.shape == g.hits.shape == image.shape
    assert abs(g.offset.x - ox) <= 1e-12 and abs(g.offset.y - oy) <= 1e-12, (what, g.offset, ox, oy)
    assert np.array_equal(g.passes, passes), (what, "passes", int((g.passes != passes).sum()), np.argwhere(g.passes != passes)[:5])
    assert np.array_equal(g.hits, hits), (what, "hits", int((g.hits != hits).sum()), np.argwhere(g.hits != hits)[:5])
    assert np.array_equal(g.image, image), (what, "image", int((g.image != image).sum()))


def _same(a, b):
    return (a.image.shape == b.image.shape and a.offset == b.offset and np.array_equal(a.passes, b.passes) and
            np.array_equal(a.hits, b.hits) and np.array_equal(a.image, b.image))


@pytest.mark.parametrize("name", EXACT_ON_DEVICE)
def test_counts_match_the_restatement(name):
    """Block edges (scans of 1, 17, 255, 256, 257, 513 beams in one launch; 1081, 33, 600 in another: the grid is sized by the
    longest, the short ones return early), one scan alone, every edge reading in every scan of 16 beams or more, rays clipped
    at the threshold that leave the grid: pass and hit counts, image and size identical to the restatement's."""
    scans, res, rt = fixture(name)
    _assert_is(_render(scans, res, rt), expected(name), name)


@pytest.mark.parametrize("name", sorted(LITERALS))
def test_hand_made_and_tie_cases_give_the_counts_written_out(name):
    """one beam per octant, and exact ties of Round half away from zero along each axis (tests/test_occupancy_host.py)"""
    scans, res, rt = fixture(name)
    g = _render(scans, res, rt)
    want_p, want_h = LITERALS[name]
    assert g.passes.shape == want_p.shape and np.array_equal(g.passes, want_p), g.passes
    assert np.array_equal(g.hits, want_h), g.hits
    _assert_is(g, expected(name), name)


def test_the_product_call_renders_the_same_image_without_counts():
    scans, res, rt = fixture("ragged_b_0.1")
    g = _render(scans, res, rt, counts=False)
    assert not hasattr(g, "passes") and not hasattr(g, "hits")
    image, _, _, (ox, oy) = expected("ragged_b_0.1")
    assert np.array_equal(g.image, image) and abs(g.offset.x - ox) <= 1e-12 and abs(g.offset.y - oy) <= 1e-12


def test_contended_cells_lose_no_count():
    """64 copies of one scan at one pose in one call: every cell is hit by 64 threads of 64 blocks.  Exactly 64 times the
    counts of the scan alone, on the same grid -- whatever the restatement says."""
    scans, res, rt = fixture("ragged_a_0.25")
    one = scans[-1]
    assert len(one.ranges) == 513
    alone = _render([one], res, rt)
    many = _render([one.copy() for _ in range(64)], res, rt)
    assert many.image.shape == alone.image.shape and many.offset == alone.offset
    assert int(alone.passes.max()) > 100 and int(alone.hits.sum()) > 50
    assert np.array_equal(many.passes, 64 * alone.passes) and np.array_equal(many.hits, 64 * alone.hits)


def test_more_scans_than_one_launch_has_rows_of_blocks():
    """65 537 times one scan of 17 beams in one call (the call only reads its scans, so one object serves): a launch has at most
    65 535 rows of blocks, so the trace goes out in several.  Exactly 65 537 times the counts of the scan alone, on the same grid;
    the largest count, 17 * 65 537, is far below 2^32.  The image is the rule (tests/occupancy_ref.py) on those counts: the single
    rendering's wherever that one had its more than two passes -- hits / passes is the same quotient -- and decided by the same
    quotient where one or two passes left the single rendering unknown."""
    from tests import occupancy_ref as ref
    scans, res, rt = fixture("ragged_a_0.25")
    one = scans[1]
    assert len(one.ranges) == 17
    n = 65537
    alone = _render([one], res, rt)
    many = _render([one] * n, res, rt)
    assert many.image.shape == alone.image.shape and many.offset == alone.offset
    assert int(alone.passes.max()) > 1 and int(alone.hits.sum()) > 0 and int(alone.passes.max()) * n < 2 ** 32
    assert np.array_equal(many.passes, n * alone.passes) and np.array_equal(many.hits, n * alone.hits)
    decided = alone.passes > ref.MIN_PASS
    assert decided.any() and np.array_equal(many.image[decided], alone.image[decided])
    with np.errstate(invalid="ignore", divide="ignore"):
        occupied = alone.hits.astype(np.float64) / alone.passes.astype(np.float64) > ref.OCC_RATIO
    want = np.where(alone.passes == 0, ref.UNKNOWN, np.where(occupied, ref.OCCUPIED, ref.FREE)).astype(np.uint8)
    assert np.array_equal(many.image, want), int((many.image != want).sum())


def test_rendering_is_repeatable():
    scans, res, rt = fixture("ragged_b_0.05")
    a, b = _render(scans, res, rt), _render(scans, res, rt)
    assert a.passes.tobytes() == b.passes.tobytes() and a.hits.tobytes() == b.hits.tobytes()
    assert a.image.tobytes() == b.image.tobytes() and a.offset == b.offset


def test_fresh_scans_render_like_scans_created_one_by_one():
    """right after bulk creation (models.ScanBlock, models.native_many) the readings may still be on their way into the pool:
    the rendering must wait for them.  The entry takes a ScanBlock, its handles as numpy integers, and plain ints."""
    from yag_slam_amd.models import ScanBlock, native_many
    scans, res, rt = fixture("block")
    want = expected("block")
    s0 = scans[0]
    sensor = (s0.min_angle, s0.max_angle, s0.angle_increment, s0.min_range, s0.max_range, s0.range_threshold)
    poses = np.array([(s.corrected_pose.x, s.corrected_pose.y, s.corrected_pose.euler[-1]) for s in scans])
    block = ScanBlock(np.stack([s.ranges for s in scans]), poses, sensor)
    _assert_is(_render(block, res, rt), want, "ScanBlock, at once")
    assert block.handles.dtype == np.uint64
    _assert_is(_render(list(block.handles), res, rt), want, "numpy uint64 handles")
    _assert_is(_render(block.handles, res, rt), want, "the handle array")
    _assert_is(_render([int(h) for h in block.handles], res, rt), want, "plain ints")
    block.release()
    twins = [s.copy() for s in scans]
    native_many(twins)
    _assert_is(_render(twins, res, rt), want, "native_many, at once")
    singles = [s.copy() for s in scans]
    for s in singles:
        s.native()
    by_one = _render(singles, res, rt)
    _assert_is(by_one, want, "one by one")
    assert _same(by_one, _render(twins, res, rt))
    _assert_is(_render([s._scan for s in singles], res, rt), want, "handles as the reference passes them")


def test_moved_scans_render_at_their_new_poses():
    """what every loop closure does before the map is redrawn: set_corrected_poses on resident scans, then the rendering"""
    from yag_slam_amd.models import set_corrected_poses
    scans, res, rt = fixture("moved")
    new = np.array([(s.corrected_pose.x, s.corrected_pose.y, s.corrected_pose.euler[-1]) for s in scans])
    old = new + np.array([0.37, -0.21, 0.4])
    mine = [make_scan(s.ranges, p) for s, p in zip(scans, old)]
    before = _render(mine, res, rt)
    set_corrected_poses(mine, new)
    after = _render(mine, res, rt)
    _assert_is(after, expected("moved"), "after set_corrected_poses")
    assert not _same(before, after)
    assert abs(before.offset.x - after.offset.x) > 0.05 and abs(before.offset.y - after.offset.y) > 0.05


def test_error_paths_name_the_cause_and_write_nothing():
    from yag_slam_amd import _capi
    from yag_slam_amd.occupancy import create_occupancy_grid
    L = _capi.lib()
    scans, res, rt = fixture("octants")
    h0 = scans[0].native()
    vp = C.c_void_p
    for create in (L.ym_occupancy_create, L.ym_occupancy_create_counted):
        assert not create((vp * 1)(h0), 0, res, rt) and "no scans" in _capi.last_error()
        assert not create(None, 1, res, rt) and "no scans" in _capi.last_error()
        assert not create((vp * 2)(h0, None), 2, res, rt) and "scan 1 is null" in _capi.last_error()
        for bad_res, bad_rt in ((0.0, rt), (-1.0, rt), (float("nan"), rt), (res, 0.0), (res, -2.0), (res, float("nan"))):
            assert not create((vp * 1)(h0), 1, bad_res, bad_rt)
            assert "resolution and range_threshold must be > 0" in _capi.last_error()
        # a box without height (one beam along x) or without width: YM_ERR_UNSUPPORTED, said with the size
        flat = make_scan([1.5], (0.25, 0.5, 0.0), min_angle=0.0, inc=0.1)
        assert not create((vp * 1)(flat.native()), 1, 0.5, 2.0) and "occupancy grid of 3 x 0 cells" in _capi.last_error()
        thin = make_scan([1.5], (0.25, 0.5, np.pi / 2), min_angle=0.0, inc=0.1)
        assert not create((vp * 1)(thin.native()), 1, 0.5, 2.0) and "occupancy grid of 0 x 3 cells" in _capi.last_error()
    with pytest.raises(_capi.YmError, match="no scans"):
        create_occupancy_grid([], res, rt)
    with pytest.raises(_capi.YmError, match="scan 1 is null"):
        create_occupancy_grid([scans[0], None], res, rt, counts=True)
    with pytest.raises(_capi.YmError, match="3 x 0 cells"):
        create_occupancy_grid([flat], 0.5, 2.0, counts=True)
    # reads: a short buffer, counts of a handle made without them -- -1, the cause, the caller's buffers as they were
    u8, u32 = C.POINTER(C.c_uint8), C.POINTER(C.c_uint32)
    info = _capi.YmOccupancyInfo()
    plain, counted = L.ym_occupancy_create((vp * 1)(h0), 1, res, rt), L.ym_occupancy_create_counted((vp * 1)(h0), 1, res, rt)
    try:
        assert plain and counted
        _capi.check(L.ym_occupancy_get_info(counted, C.byref(info)))
        n = info.width * info.height
        assert n == 48
        img = np.full(n, 9, np.uint8)
        p, h = np.full(n, 0x09090909, np.uint32), np.full(n, 0x09090909, np.uint32)
        for og in (plain, counted):
            assert L.ym_occupancy_read(og, img.ctypes.data_as(u8), n - 1) == -1 and "buffer too small: need 48 bytes" in _capi.last_error()
            assert L.ym_occupancy_read(og, None, n) == -1 and "null argument" in _capi.last_error()
        assert L.ym_occupancy_read_counts(plain, p.ctypes.data_as(u32), h.ctypes.data_as(u32), n) == -1
        assert "made without counts" in _capi.last_error()
        assert L.ym_occupancy_read_counts(counted, p.ctypes.data_as(u32), h.ctypes.data_as(u32), n - 1) == -1
        assert "too small: need 48 cells" in _capi.last_error()
        assert L.ym_occupancy_read_counts(counted, p.ctypes.data_as(u32), None, n) == -1 and "null argument" in _capi.last_error()
        assert L.ym_occupancy_read_counts(None, p.ctypes.data_as(u32), h.ctypes.data_as(u32), n) == -1
        assert np.all(img == 9) and np.all(p == 0x09090909) and np.all(h == 0x09090909)
        # and with room, both handles give the image, the counted one its counts
        assert L.ym_occupancy_read(plain, img.ctypes.data_as(u8), n) == 0
        assert L.ym_occupancy_read_counts(counted, p.ctypes.data_as(u32), h.ctypes.data_as(u32), n) == 0
        want_p, want_h = LITERALS["octants"]
        assert np.array_equal(img.reshape(want_p.shape), expected("octants")[0])
        assert np.array_equal(p.reshape(want_p.shape), want_p) and np.array_equal(h.reshape(want_p.shape), want_h)
    finally:
        L.ym_occupancy_destroy(plain)
        L.ym_occupancy_destroy(counted)
