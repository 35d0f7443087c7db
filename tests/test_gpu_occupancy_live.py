"""The live occupancy grid on the device (occupancy.LiveOccupancyGrid, ym_occmap_*): counts that stay
resident and are changed by the rays of the scans added, moved or dropped.  Two yardsticks, both exact: the full renderer through
its counts hook (create_occupancy_grid(counts=True)) with the anchor at its offset, and the numpy restatement in a given frame
(tests/occupancy_live_ref.py) for every other anchor.  Every case compared with the restatement is shown on the CPU, in
tests/test_occupancy_live_host.py, to be at least 1e-9 cells from every rounding tie in its own frame."""
import ctypes as C
import functools
import gc

import numpy as np
import pytest

from tests import occupancy_live_ref as live_ref
from tests.test_occupancy_host import EXACT_ON_DEVICE, MARGIN, expected, fixture, make_scan
from tests.test_occupancy_live_host import (OWN_ANCHOR_SPLITS, REMOVE_CASES, SHIFTED_CASES, edge_scans, moved_from, own_anchor,
                                            shifted_anchor)

pytestmark = pytest.mark.gpu

ROOM = "room40"
MODES = ("at_once", "one_by_one", "reversed", "first_then_rest")


@functools.lru_cache(maxsize=None)
def _case(name):
    """-> (scans, resolution, range_threshold); the 40-scan room next to the fixtures of test_occupancy_host"""
    if name != ROOM:
        return fixture(name)
    from yag_slam_amd import synth
    scene = synth.Scene()
    truth, _ = synth.loop_trajectory(40 * 12)
    return [synth.resident_scan(scene.scan_ranges(p, index=700 + i), p) for i, p in enumerate(truth[::12])], 0.05, 12.0


@functools.lru_cache(maxsize=None)
def _full(name):
    """the full renderer's counted grid of a case, rendered once"""
    from yag_slam_amd.occupancy import create_occupancy_grid
    scans, res, rt = _case(name)
    g = create_occupancy_grid(scans, res, rt, counts=True)
    for a in (g.image, g.passes, g.hits):
        a.setflags(write=False)
    return g


def _batches(scans, mode):
    scans = list(scans)
    if mode == "at_once":
        return [scans]
    if mode == "one_by_one":
        return [[s] for s in scans]
    if mode == "reversed":
        return [[s] for s in reversed(scans)]
    return [scans[:1], scans[1:]] if len(scans) > 1 else [scans]


def _live(res, rt, **kw):
    from yag_slam_amd.occupancy import LiveOccupancyGrid
    return LiveOccupancyGrid(res, rt, **kw)


def _counted(live):
    """the window with its counts; no count may have wrapped: hits <= passes everywhere and nothing at or beyond 2^31"""
    g = live.grid(counts=True)
    assert g.passes.dtype == np.uint32 and g.hits.dtype == np.uint32 and g.passes.shape == g.hits.shape == g.image.shape
    assert np.all(g.hits <= g.passes) and int(g.passes.max(initial=0)) < 2 ** 31
    return g


def _assert_same_grid(g, want, what):
    assert g.image.shape == want.image.shape, (what, g.image.shape, want.image.shape)
    assert (g.offset.x, g.offset.y) == (want.offset.x, want.offset.y) and g.resolution == want.resolution, (what, g.offset, want.offset)
    assert np.array_equal(g.passes, want.passes), (what, "passes", int((g.passes != want.passes).sum()), np.argwhere(g.passes != want.passes)[:5])
    assert np.array_equal(g.hits, want.hits), (what, "hits", int((g.hits != want.hits).sum()))
    assert np.array_equal(g.image, want.image), (what, "image", int((g.image != want.image).sum()))


def _fill_anchored(name, mode, slack=64):
    scans, res, rt = _case(name)
    full = _full(name)
    live = _live(res, rt, anchor=(full.offset.x, full.offset.y), slack_cells=slack)
    for batch in _batches(scans, mode):
        live.add(batch)
    return live, full


# ------------------------------------------------------------------------------------------ 1. against the full renderer
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("name", EXACT_ON_DEVICE + (ROOM,))
def test_anchored_at_the_full_rendering_it_is_the_full_rendering(name, mode):
    """anchor = the full rendering's offset; the scans added at once, one by one, one by one reversed (the origin moves towards
    smaller cells with every add) and first-then-rest: info, counts and image identical, bit for bit"""
    live, full = _fill_anchored(name, mode)
    info = live.info
    assert (info["origin_x"], info["origin_y"]) == (0, 0) and (info["width"], info["height"]) == (full.width, full.height)
    assert (info["offset_x"], info["offset_y"]) == (full.offset.x, full.offset.y) == (info["anchor_x"], info["anchor_y"])
    assert info["added"] == 1 and info["has_anchor"] == 1 and info["resolution"] == full.resolution
    assert info["alloc_width"] >= info["width"] and info["alloc_height"] >= info["height"]
    assert info["alloc_origin_x"] <= 0 and info["alloc_origin_y"] <= 0
    _assert_same_grid(_counted(live), full, (name, mode))
    plain = live.grid()
    assert not hasattr(plain, "passes") and np.array_equal(plain.image, full.image)
    assert len(live) == len(_case(name)[0])


def test_a_scan_block_is_added_at_its_scans_own_poses():
    """models.ScanBlock (scans without Python objects): right after bulk creation the readings may still be on their way"""
    from yag_slam_amd.models import ScanBlock
    scans, res, rt = fixture("block")
    full = _full("block")
    s0 = scans[0]
    sensor = (s0.min_angle, s0.max_angle, s0.angle_increment, s0.min_range, s0.max_range, s0.range_threshold)
    poses = np.array([(s.corrected_pose.x, s.corrected_pose.y, s.corrected_pose.euler[-1]) for s in scans])
    block = ScanBlock(np.stack([s.ranges for s in scans]), poses, sensor)
    live = _live(res, rt, anchor=(full.offset.x, full.offset.y))
    live.add(block)
    assert len(live) == 3
    _assert_same_grid(_counted(live), full, "ScanBlock")
    with pytest.raises(ValueError, match="already held"):
        live.add(block)
    live.clear()
    assert len(live) == 0 and live.info["added"] == 0 and (live.info["anchor_x"], live.info["anchor_y"]) == (full.offset.x, full.offset.y)
    live.add(scans)
    _assert_same_grid(_counted(live), full, "after clear")
    live.close()
    block.release()


# ------------------------------------------------------------------------------------------ 2. against the restatement
@functools.lru_cache(maxsize=None)
def _want_in_frame(name, anchor, held=None, box=None):
    """the restatement of scans `held` (indices; default all) of a case in `anchor`'s lattice, in the window of scans `box`"""
    scans, res, rt = _case(name)
    held_scans = list(scans) if held is None else [scans[i] for i in held]
    origin, w, h = live_ref.frame_of(list(scans) if box is None else [scans[i] for i in box], res, rt, anchor)
    out = live_ref.render_in_frame(held_scans, res, rt, anchor, origin, w, h)
    for a in out:
        a.setflags(write=False)
    return (origin, w, h), out


def _assert_is_restatement(live, frame, want, what):
    (origin, w, h), (image, passes, hits) = frame, want
    info = live.info
    assert (info["origin_x"], info["origin_y"]) == origin and (info["width"], info["height"]) == (w, h), (what, info, origin, w, h)
    assert info["offset_x"] == info["anchor_x"] + origin[0] * info["resolution"]
    assert info["offset_y"] == info["anchor_y"] + origin[1] * info["resolution"]
    g = _counted(live)
    assert (g.offset.x, g.offset.y) == (info["offset_x"], info["offset_y"])
    assert np.array_equal(g.passes, passes), (what, "passes", int((g.passes != passes).sum()), np.argwhere(g.passes != passes)[:5])
    assert np.array_equal(g.hits, hits), (what, "hits", int((g.hits != hits).sum()), np.argwhere(g.hits != hits)[:5])
    assert np.array_equal(g.image, image), (what, "image", int((g.image != image).sum()))
    return g


def _fill_own(name, slack):
    scans, res, rt = _case(name)
    live = _live(res, rt, slack_cells=slack)
    for batch in OWN_ANCHOR_SPLITS[name]:
        live.add([scans[i] for i in batch])
    return live


@pytest.mark.parametrize("slack", (0, 64, 4096))
@pytest.mark.parametrize("name", sorted(OWN_ANCHOR_SPLITS))
def test_own_anchor_in_batches_is_the_restatement(name, slack):
    """no anchor given: the first batch's bounding-box minimum becomes it, and the later batches grow the window past that box
    towards smaller and larger cells.  slack_cells 0 (every growing add reallocates), 64 and 4096 (none does after the first)."""
    live = _fill_own(name, slack)
    info = live.info
    anchor = (info["anchor_x"], info["anchor_y"])   # the device's bounding-box minimum: libm's to a few ulp
    assert max(abs(a - b) for a, b in zip(anchor, own_anchor(name))) <= 1e-12
    frame, want = _want_in_frame(name, anchor)
    assert frame[0][0] < 0 or frame[0][1] < 0
    _assert_is_restatement(live, frame, want, (name, slack))
    if slack == 0:
        assert info["reallocations"] > 0
    if slack == 4096:
        assert info["reallocations"] == 0


@pytest.mark.parametrize("slack", (0, 4096))
@pytest.mark.parametrize("name", SHIFTED_CASES)
def test_an_anchor_off_every_box_gives_origins_of_both_signs(name, slack):
    scans, res, rt = _case(name)
    anchor = shifted_anchor(name)
    live = _live(res, rt, anchor=anchor, slack_cells=slack)
    for s in scans:
        live.add([s])
    frame, want = _want_in_frame(name, anchor)
    assert frame[0][0] > 0 and frame[0][1] < 0
    _assert_is_restatement(live, frame, want, (name, slack))
    if slack == 4096:
        assert live.info["reallocations"] == 0


# ------------------------------------------------------------------------------------------ 3. ray lengths around the wave's width
@functools.lru_cache(maxsize=None)
def _edge_want():
    scans, res, rt, anchor = edge_scans()
    origin, w, h = live_ref.frame_of(list(scans), res, rt, anchor)
    return (origin, w, h), live_ref.render_in_frame(list(scans), res, rt, anchor, origin, w, h)


@pytest.mark.parametrize("form", (0, 1))
def test_ray_lengths_around_the_wave_width(form):
    """rays of 0, 1, 62 .. 65 and 127 .. 129 cells along the major axis in every octant, with dx = dy and one-off-the-diagonal
    cases, and rays clipped at the threshold that leave the window: the wave-per-ray trace (form 0) and the thread-per-ray
    development form (1) both give the restatement's counts, so identical ones"""
    scans, res, rt, anchor = edge_scans()
    live = _live(res, rt, anchor=anchor, slack_cells=8)
    live._set_trace_form(form)
    live.add(list(scans))
    frame, want = _edge_want()
    g = _assert_is_restatement(live, frame, want, ("edges", form))
    assert int(g.hits.sum()) > 100 and int(g.passes.max()) >= 100   # (every ray starts in the sensor's cell)
    # taken out again under the OTHER form: the two forms visit the same cells, so nothing is left
    live._set_trace_form(1 - form)
    live.remove(list(scans))
    g = _counted(live)
    assert not g.passes.any() and not g.hits.any()


@functools.lru_cache(maxsize=None)
def _many_copies():
    """-> (the full renderer's counted grid of one scan of 17 beams, 32 769 copies of that scan created in bulk, res, rt)"""
    from yag_slam_amd.models import native_many
    from yag_slam_amd.occupancy import create_occupancy_grid
    scans, res, rt = fixture("ragged_a_0.25")
    one = scans[1]
    assert len(one.ranges) == 17
    alone = create_occupancy_grid([one], res, rt, counts=True)
    copies = [one.copy() for _ in range(32769)]   # (the grid refuses a scan that is in a list twice)
    native_many(copies)
    return alone, copies, res, rt


@pytest.mark.parametrize("form", (0, 1))
def test_more_scans_than_one_launch_takes(form):
    """32 769 times one scan of 17 beams in one add, one more than a launch of the trace takes: exactly 32 769 times the full
    rendering's counts of the scan alone (the largest, 17 * 32 769, is far below 2^31), and after one remove of them all every
    count is zero"""
    alone, copies, res, rt = _many_copies()
    n = len(copies)
    live = _live(res, rt, anchor=(alone.offset.x, alone.offset.y))
    live._set_trace_form(form)
    live.add(copies)
    g = _counted(live)
    assert g.image.shape == alone.image.shape and (g.offset.x, g.offset.y) == (alone.offset.x, alone.offset.y)
    assert int(alone.passes.max()) > 1 and int(alone.hits.sum()) > 0
    assert np.array_equal(g.passes, n * alone.passes) and np.array_equal(g.hits, n * alone.hits)
    live.remove(copies)
    g = _counted(live)
    assert g.image.shape == alone.image.shape and not g.passes.any() and not g.hits.any()
    live.close()


# ------------------------------------------------------------------------------------------ 4. remove and move
@pytest.mark.parametrize("name", sorted(REMOVE_CASES))
def test_remove_leaves_the_rest_in_the_unshrunk_window(name):
    scans, res, rt = _case(name)
    anchor = shifted_anchor(name)
    gone = REMOVE_CASES[name]
    rest = tuple(i for i in range(len(scans)) if i not in gone)
    live = _live(res, rt, anchor=anchor)
    live.add(scans)
    frame, want_all = _want_in_frame(name, anchor)
    first = _assert_is_restatement(live, frame, want_all, (name, "all"))
    before = live.info
    live.remove([scans[i] for i in gone])
    assert len(live) == len(rest)
    after = live.info
    assert {k: after[k] for k in after} == {k: before[k] for k in before}  # the window does not shrink, nothing moved
    _, want_rest = _want_in_frame(name, anchor, held=rest, box=tuple(range(len(scans))))
    _assert_is_restatement(live, frame, want_rest, (name, "rest"))
    # remove everything: every count 0, every cell unknown
    live.remove([scans[i] for i in rest])
    g = _counted(live)
    assert len(live) == 0 and not g.passes.any() and not g.hits.any() and np.all(g.image == 200) and g.image.shape == first.image.shape
    # and add again, in another order: the first state exactly
    live.add(list(reversed(scans)))
    again = _counted(live)
    assert np.array_equal(again.passes, first.passes) and np.array_equal(again.hits, first.hits) and np.array_equal(again.image, first.image)
    assert live.info == before


def _cut(info, g, rect):
    """a grid's counts in the lattice rectangle rect = (x0, y0, x1, y1), which its window holds"""
    x, y = rect[0] - info["origin_x"], rect[1] - info["origin_y"]
    w, h = rect[2] - rect[0], rect[3] - rect[1]
    assert 0 <= x and x + w <= g.width and 0 <= y and y + h <= g.height
    return np.stack([g.passes[y:y + h, x:x + w], g.hits[y:y + h, x:x + w]])


def test_sync_after_moves_takes_both_routes_to_the_same_counts():
    from yag_slam_amd.models import set_corrected_poses
    scans, res, rt = fixture("moved")
    anchor = shifted_anchor("moved")
    mine, new = moved_from()
    live = _live(res, rt, anchor=anchor)
    at_first = [s.copy() for s in mine]
    assert live.sync(mine) == "rebuild" and len(live) == 3
    origin, w, h = live_ref.frame_of(mine, res, rt, anchor)
    _assert_is_restatement(live, (origin, w, h), live_ref.render_in_frame(mine, res, rt, anchor, origin, w, h), "first poses")
    assert live.sync(mine) == "none"
    # one of three moved: an update; the window is that of everything ever added
    mine[2].corrected_pose = scans[2].corrected_pose
    assert live.sync(mine) == "update"
    ever = at_first + [scans[2]]
    origin, w, h = live_ref.frame_of(ever, res, rt, anchor)
    updated = _assert_is_restatement(live, (origin, w, h), live_ref.render_in_frame(mine, res, rt, anchor, origin, w, h), "one moved")
    updated_info = live.info
    # the same state reached by the other route on a second grid: the same counts wherever either has a cell
    other = _live(res, rt, anchor=anchor)
    assert other.sync(mine) == "rebuild"
    rebuilt, rebuilt_info = _counted(other), other.info
    # (the windows differ -- one is that of everything ever added, the other starts over -- and outside its window a grid reads
    # nothing, though rays clipped at the threshold leave counts there: compare where both can be read)
    x0, y0 = max(updated_info["origin_x"], rebuilt_info["origin_x"]), max(updated_info["origin_y"], rebuilt_info["origin_y"])
    x1 = min(updated_info["origin_x"] + updated.width, rebuilt_info["origin_x"] + rebuilt.width)
    y1 = min(updated_info["origin_y"] + updated.height, rebuilt_info["origin_y"] + rebuilt.height)
    assert x1 - x0 >= min(updated.width, rebuilt.width) - 1 and y1 - y0 >= min(updated.height, rebuilt.height) - 1
    rect = (x0, y0, x1, y1)
    assert np.array_equal(_cut(updated_info, updated, rect), _cut(rebuilt_info, rebuilt, rect))
    # the other two moved as well, as a loop closure does it: more than half -> rebuild, and the fixture's own rendering
    set_corrected_poses(mine[:2], new[:2])
    assert live.sync(mine) == "rebuild"
    frame, want = _want_in_frame("moved", anchor)
    _assert_is_restatement(live, frame, want, "all moved")
    # a scan dropped from the list goes out at the pose it was traced at
    assert live.sync(mine[1:]) == "update" and len(live) == 2
    _, want_rest = _want_in_frame("moved", anchor, held=(1, 2), box=(0, 1, 2))
    _assert_is_restatement(live, frame, want_rest, "one dropped")


# ------------------------------------------------------------------------------------------ 5. growth
@pytest.mark.parametrize("mode", ("one_by_one", "reversed"))
@pytest.mark.parametrize("name", ("ragged_a_0.05", "ragged_b_0.125", "moved", ROOM))
def test_slack_changes_the_reallocations_and_nothing_else(name, mode):
    tight, full = _fill_anchored(name, mode, slack=0)
    roomy, _ = _fill_anchored(name, mode, slack=4096)
    _assert_same_grid(_counted(tight), full, (name, mode, 0))
    _assert_same_grid(_counted(roomy), full, (name, mode, 4096))
    a, b = tight.info, roomy.info
    assert b["reallocations"] == 0
    if name != ROOM:   # (the room's first scan sees all four walls: no later add grows anything, whatever the slack)
        assert a["reallocations"] > 0
    assert a["alloc_width"] < b["alloc_width"] and a["alloc_height"] < b["alloc_height"]
    for k in ("width", "height", "offset_x", "offset_y", "origin_x", "origin_y", "anchor_x", "anchor_y"):
        assert a[k] == b[k], k


# ------------------------------------------------------------------------------------------ 6. the publish path
@pytest.mark.parametrize("name", ("ragged_b_0.05", ROOM))
def test_ros_map_is_the_full_path_when_anchored_there(name):
    from yag_slam_amd import occupancy
    scans, res, rt = _case(name)
    live, full = _fill_anchored(name, "first_then_rest")
    want = occupancy.ros_map(scans, res, rt)
    got = live.ros_map()
    assert got.data.dtype == np.int8 and np.array_equal(got.data, want.data) and got.stats == want.stats
    assert (got.width, got.height, got.resolution) == (want.width, want.height, want.resolution)
    assert (got.origin.x, got.origin.y) == (want.origin.x, want.origin.y)
    clean = live.clean_grid(min_area=3, connectivity=4)
    ref_clean = occupancy.create_clean_occupancy_grid(scans, res, rt, min_area=3, connectivity=4)
    assert np.array_equal(clean.image, ref_clean.image) and clean.stats == ref_clean.stats
    if name == ROOM:
        assert want.stats["removed_components"] > 0  # the filter has something to do here


def test_ros_map_with_its_own_anchor_is_the_filter_of_its_own_grid():
    from yag_slam_amd import occupancy
    live = _fill_own("ragged_a_0.05", 64)
    image = live.grid().image
    want, stats = occupancy.despeckle(image, stats=True)
    got = live.ros_map()
    assert np.array_equal(got.data, occupancy.ros_codes(want)) and got.stats == stats
    assert np.array_equal(live.grid().image, image)  # a read changes nothing


# ------------------------------------------------------------------------------------------ 7. the mapper
def _poses(scans):
    return np.array([(s.corrected_pose.x, s.corrected_pose.y, s.corrected_pose.euler[-1]) for s in scans])


def _mapper_check(mp, res, rt, ever, what):
    from yag_slam_amd import occupancy
    live = mp.live_grid
    info = live.info
    anchor = (info["anchor_x"], info["anchor_y"])
    margin = live_ref.tie_margin_in_frame(mp.scans, res, rt, anchor, box_scans=ever)
    print("%s: tie margin %.3g cells" % (what, margin))
    assert margin >= MARGIN
    origin, w, h = live_ref.frame_of(ever, res, rt, anchor)
    want = live_ref.render_in_frame(mp.scans, res, rt, anchor, origin, w, h)
    _assert_is_restatement(live, (origin, w, h), want, what)
    return occupancy.ros_codes(occupancy.despeckle(want[0]))


def test_mapper_publishes_from_the_live_grid():
    from yag_slam_amd import synth
    from yag_slam_amd.mapping import LoopClosingMapper
    from yag_slam_amd.models import set_corrected_poses
    from yag_slam_amd.scan_matching import ScanMatcher
    res, rt = 0.05, 12
    truth, scans = synth.trajectory_scans(30)
    mp = LoopClosingMapper(ScanMatcher(), None)
    maps = []
    for i, s in enumerate(scans):
        mp.process_scan(s)
        if (i + 1) % 5 == 0:
            maps.append(mp.live_ros_map(res, rt))
            assert len(mp.live_grid) == i + 1
    assert len(maps) == 6 and maps[-1].width >= maps[0].width and maps[-1].resolution == res
    live = mp.live_grid
    assert mp.live_ros_map(res, rt).data.tobytes() == maps[-1].data.tobytes() and mp.live_grid is live
    at_added = [s.copy() for s in mp.scans]
    codes = _mapper_check(mp, res, rt, at_added, "30 scans")
    assert np.array_equal(maps[-1].data, codes) and set(np.unique(codes)) <= {-1, 0, 100} and (codes == 100).sum() > 200
    # the optimiser moves a third of the poses (run_opt's call): the next publish retraces those ten and nothing else
    poses = _poses(mp.scans)
    poses[10:20] += np.array([0.04, -0.03, 0.01])
    set_corrected_poses(mp.scans[10:20], poses[10:20])
    moved = mp.live_ros_map(res, rt)
    assert mp.live_grid is live and len(live) == 30
    codes = _mapper_check(mp, res, rt, at_added + [s.copy() for s in mp.scans[10:20]], "ten moved")
    assert np.array_equal(moved.data, codes) and moved.data.shape != () and not np.array_equal(moved.data, maps[-1].data)
    # every pose moved: the grid starts over in the same lattice
    poses[:] += np.array([-0.02, 0.05, -0.004])
    set_corrected_poses(mp.scans, poses)
    anchor_before = (live.info["anchor_x"], live.info["anchor_y"])
    all_moved = mp.live_ros_map(res, rt)
    assert (live.info["anchor_x"], live.info["anchor_y"]) == anchor_before
    codes = _mapper_check(mp, res, rt, list(mp.scans), "all moved")
    assert np.array_equal(all_moved.data, codes)
    # another resolution: another grid
    coarse = mp.live_ros_map(0.1, rt)
    assert mp.live_grid is not live and coarse.resolution == 0.1 and coarse.width < all_moved.width


# ------------------------------------------------------------------------------------------ 8. lifetime
def test_the_grid_keeps_what_it_holds_alive_and_leaves_scans_alone_when_it_goes():
    from yag_slam_amd.scan_matching import ScanMatcher
    scans, res, rt = fixture("block")
    anchor = shifted_anchor("block")
    mine = [make_scan(s.ranges, (s.corrected_pose.x, s.corrected_pose.y, s.corrected_pose.euler[-1])) for s in scans]
    live = _live(res, rt, anchor=anchor)
    live.add(mine)
    keep = mine[1]
    del mine
    gc.collect()
    assert live.sync([keep]) == "update" and len(live) == 1   # the other two go out through the references the grid kept
    frame, want = _want_in_frame("block", anchor, held=(1,), box=(0, 1, 2))
    _assert_is_restatement(live, frame, want, "after the caller let go")
    # the grid goes with scans still held: they stay usable
    others = [make_scan(s.ranges, (s.corrected_pose.x, s.corrected_pose.y, s.corrected_pose.euler[-1])) for s in scans[:1]]
    live.add(others)
    live.close()
    del live
    gc.collect()
    r = ScanMatcher().match_scan(keep, others, True, True)
    assert np.isfinite(r.response) and 0.0 <= r.response <= 1.0


# ------------------------------------------------------------------------------------------ the ABI's refusals
def test_error_paths_name_the_cause_and_write_nothing():
    from yag_slam_amd import _capi
    L = _capi.lib()
    scans, res, rt = fixture("octants")
    h0 = scans[0].native()
    vp, dp = C.c_void_p, C.POINTER(C.c_double)
    u8, u32 = C.POINTER(C.c_uint8), C.POINTER(C.c_uint32)
    om = L.ym_occmap_create(0, res, rt, None, 4)
    assert om
    try:
        one = (vp * 1)(h0)
        img, p, h = np.full(64, 9, np.uint8), np.full(64, 0x09090909, np.uint32), np.full(64, 0x09090909, np.uint32)
        info = _capi.YmOccmapInfo()
        assert L.ym_occmap_get_info(om, C.byref(info)) == 0 and info.added == 0 and info.has_anchor == 0 and info.width == 0
        # before any add: no read, no subtraction
        assert L.ym_occmap_read(om, img.ctypes.data_as(u8), 48, None, None) == -1 and "nothing has been added yet" in _capi.last_error()
        assert L.ym_occmap_read_counts(om, p.ctypes.data_as(u32), h.ctypes.data_as(u32), 48) == -1 and "nothing has been added" in _capi.last_error()
        assert L.ym_occmap_accumulate(om, one, None, 1, -1) == -1 and "nothing to subtract" in _capi.last_error()
        assert L.ym_occmap_accumulate(om, one, None, 0, 1) == -1 and "no scans" in _capi.last_error()
        assert L.ym_occmap_accumulate(om, None, None, 1, 1) == -1 and "no scans" in _capi.last_error()
        assert L.ym_occmap_accumulate(om, (vp * 2)(h0, None), None, 2, 1) == -1 and "scan 1 is null" in _capi.last_error()
        for sign in (0, 2, -2):
            assert L.ym_occmap_accumulate(om, one, None, 1, sign) == -1 and "sign %d: +1 or -1" % sign in _capi.last_error()
        bad = np.array([0.0, float("nan"), 0.0])
        assert L.ym_occmap_accumulate(om, one, bad.ctypes.data_as(dp), 1, 1) == -1 and "pose 0: not finite" in _capi.last_error()
        assert L.ym_occmap_debug_option(om, 2, 0) == -1 and L.ym_occmap_debug_option(om, 1, 5) == -1
        assert L.ym_occmap_get_info(om, C.byref(info)) == 0 and info.added == 0 and info.has_anchor == 0  # nothing stuck
        # the scan's own pose (poses = null), then sizes that are not the window's
        assert L.ym_occmap_accumulate(om, one, None, 1, 1) == 0
        assert L.ym_occmap_get_info(om, C.byref(info)) == 0 and (info.width, info.height, info.added) == (8, 6, 1)
        off = expected("octants")[3]
        assert (info.anchor_x, info.anchor_y) == (info.offset_x, info.offset_y) and (info.origin_x, info.origin_y) == (0, 0)
        assert abs(info.anchor_x - off[0]) <= 1e-12 and abs(info.anchor_y - off[1]) <= 1e-12
        off = (info.anchor_x, info.anchor_y)
        for n in (47, 49, 0, -1):
            assert L.ym_occmap_read(om, img.ctypes.data_as(u8), n, None, None) == -1 and "the window has 48" in _capi.last_error()
            assert L.ym_occmap_read_counts(om, p.ctypes.data_as(u32), h.ctypes.data_as(u32), n) == -1 and "the window has 48" in _capi.last_error()
        assert L.ym_occmap_read(om, None, 48, None, None) == -1 and "null argument" in _capi.last_error()
        assert L.ym_occmap_read_counts(om, p.ctypes.data_as(u32), None, 48) == -1 and "null argument" in _capi.last_error()
        bad_opts = _capi.YmDespeckleOpts(0, 255, 5, 6)
        assert L.ym_occmap_read(om, img.ctypes.data_as(u8), 48, C.byref(bad_opts), None) == -1 and "connectivity 6" in _capi.last_error()
        assert np.all(img == 9) and np.all(p == 0x09090909) and np.all(h == 0x09090909)
        # with room: the rendering written out by hand in test_occupancy_host
        assert L.ym_occmap_read(om, img.ctypes.data_as(u8), 48, None, None) == 0
        assert L.ym_occmap_read_counts(om, p.ctypes.data_as(u32), h.ctypes.data_as(u32), 48) == 0
        image, passes, hits, _ = expected("octants")
        assert np.array_equal(img[:48].reshape(6, 8), image) and np.array_equal(p[:48].reshape(6, 8), passes) and np.array_equal(h[:48].reshape(6, 8), hits)
        assert np.all(img[48:] == 9) and np.all(p[48:] == 0x09090909)
        # clear: the anchor stays, reads are refused again
        assert L.ym_occmap_clear(om) == 0
        assert L.ym_occmap_get_info(om, C.byref(info)) == 0 and (info.added, info.has_anchor, info.width) == (0, 1, 0)
        assert (info.anchor_x, info.anchor_y) == off
        assert L.ym_occmap_read(om, img.ctypes.data_as(u8), 48, None, None) == -1 and "nothing has been added yet" in _capi.last_error()
        assert L.ym_occmap_accumulate(om, one, None, 1, -1) == -1
        # a box without height can be added to, not read
        flat = make_scan([1.5], (0.25, 0.5, 0.0), min_angle=0.0, inc=0.1)
        om2 = L.ym_occmap_create(0, 0.5, 2.0, None, 0)
        try:
            assert L.ym_occmap_accumulate(om2, (vp * 1)(flat.native()), None, 1, 1) == 0
            assert L.ym_occmap_read(om2, img.ctypes.data_as(u8), 0, None, None) == -4 and "occupancy grid of 3 x 0 cells" in _capi.last_error()
        finally:
            L.ym_occmap_destroy(om2)
    finally:
        L.ym_occmap_destroy(om)
