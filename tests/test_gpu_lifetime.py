"""Every handle gives back exactly the memory it took.  The library counts the bytes its two buffer types hold (device and
pinned, ym_debug_live_bytes: its own counts, not the card's free memory), so each case creates, uses and destroys a handle
on the smallest input that makes it allocate all of its lazily grown buffers, and asserts both numbers are what they were
before -- exactly.  The failure paths are argument errors that return after their first buffers exist."""
import ctypes as C
import gc
import math

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

BEAMS = 64
SPAN = 1.5 * math.pi                  # the synthetic sensor's 270 degrees, over 64 beams
INC = SPAN / (BEAMS - 1)


def live():
    """(device bytes, pinned bytes) the library's handles hold; handles of earlier tests still waiting for the collector go first"""
    from yag_slam_amd import _capi
    gc.collect()
    dev, pin = C.c_int64(-1), C.c_int64(-1)
    _capi.check(_capi.lib().ym_debug_live_bytes(C.byref(dev), C.byref(pin)))
    return int(dev.value), int(pin.value)


@pytest.fixture(scope="module")
def baseline():
    return live()


def _scan(scene, truth, pose, index):
    from yag_slam_amd import synth
    from yag_slam_amd.models import LocalizedRangeScan
    r = scene.scan_ranges(truth, index=index, n_beams=BEAMS, min_angle=-SPAN / 2, inc=INC)
    return LocalizedRangeScan(r, -SPAN / 2, SPAN / 2, INC, synth.MIN_RANGE, synth.MAX_RANGE, synth.RANGE_THRESHOLD,
                              float(pose[0]), float(pose[1]), float(pose[2]))


def _room(n=64, wall=60):
    """an n x n occupancy image: a free square with walls (0) at cells 0 and `wall`, unknown nowhere"""
    im = np.full((n, n), 255, dtype=np.uint8)
    im[[0, wall], :wall + 1] = 0
    im[:wall + 1, [0, wall]] = 0
    im[wall + 1:, :] = 0
    im[:, wall + 1:] = 0
    return im


def test_matcher_sequence_batch_and_single_match(baseline):
    """the chained sequence grows seq_pose, seq_fault and the pinned seq_results, which ym_destroy used to forget"""
    from yag_slam_amd import synth
    from yag_slam_amd.scan_matching import ScanMatcher
    from yag_slam_amd.transform import Transform
    before = live()
    scene = synth.Scene()
    truth, prior = synth.loop_trajectory(4)
    scans = [_scan(scene, truth[i], truth[0], i) for i in range(4)]
    for s, p in zip(scans, prior):
        s.odom_pose = Transform(p[0], p[1], 0.0, p[2])
    scans[0].odom_pose = Transform(truth[0][0], truth[0][1], 0.0, truth[0][2])
    m = ScanMatcher()
    res = m.map_sequence(scans, 1, 10, True, True, device_chain=True)
    assert len(res) == 3
    assert m.sequence_stats()[0] >= 1
    grown = live()
    assert grown[0] > before[0] and grown[1] > before[1]
    chains = [[_scan(scene, (2.0 + 0.1 * i + 0.3 * c, 3.0, 0.0), (2.0 + 0.1 * i + 0.3 * c, 3.0, 0.0), 10 + 2 * c + i) for i in range(2)]
              for c in range(4)]
    query = _scan(scene, (2.07, 3.04, 0.05), (2.0, 3.0, 0.0), 20)
    per, best = m.match_scan_batch(query, chains)
    assert len(per) == 4 and 0 <= best < 4
    m.match_scan(query, chains[0])
    m.close()
    del scans, chains, query
    assert live() == before


def test_raymap_trace_and_trace_each(baseline):
    from yag_slam_amd.splicing import RayMap, direction_table
    before = live()
    starts = [[10.0, 12.0], [20.5, 8.25]]
    dirs = direction_table([0.0, 90.0, 180.0, 270.0])
    rm = RayMap(_room(32, 30))
    ends, lengths = rm.trace(starts, [0.0, 90.0, 180.0, 270.0])
    assert ends.shape == (2, 4, 2) and rm.capped == 0
    each, _ = rm.trace_each(starts, np.stack([dirs, dirs[::-1]]))
    assert np.array_equal(each[0], ends[0])
    assert live()[0] > before[0]
    rm.close()
    assert live() == before


def test_segments_from_labels_and_from_a_map(baseline):
    from yag_slam_amd import synth
    from yag_slam_amd.splicing import SegmentMap
    before = live()
    sm = SegmentMap(synth.seeded_partition(16, 16, 3, seed=5))
    count, _, _ = sm.stats(4)
    assert count.sum() == 256
    assert sm.boundaries().any()
    assert len(sm.pairs()[0]) >= 1
    sm.close()
    assert live() == before
    for stage in ("final", "assigned"):
        sm = SegmentMap.from_map(_room(), n_segments=2, stage=stage)
        assert sm.info["n_free"] > 0 and sm.labels().max() >= 1
        sm.close()
        assert live() == before


def test_pose_graph_optimize(baseline):
    from yag_slam_amd.posegraph import PoseGraphOptimizer
    before = live()
    opt = PoseGraphOptimizer()
    for i in range(3):
        opt.add_node(1.0 * i + 0.05 * i, 0.02 * i, 0.01 * i, i)
    for a in range(2):
        opt.add_constraint(a, a + 1, 1.0, 0.0, 0.0, np.eye(3))
    opt.compute(10)
    assert live()[0] > before[0]
    opt.close()
    assert live() == before


def test_yagpy_matcher_map_and_locator(baseline):
    from yag_slam_amd import synth
    from yag_slam_amd.scan_matching import ScanMatcher
    before = live()
    m = ScanMatcher(dict(resolution=0.05, smear_deviation=0.05), semantics="yagpy")
    cmap = m.correlation_grid_from_occupancy(_room(), occupied_value=0)
    assert cmap.shape == (64, 64)
    scan = _scan(synth.Scene(3.0, 3.0, n_boxes=0), (1.4, 1.6, 0.3), (0.0, 0.0, 0.0), 30)
    held = live()
    loc = m.map_locator(cmap, levels=2, max_nodes=4096)
    assert live()[0] - held[0] == loc.bytes  # (the locator's own figure: its fixed-size buffers are allocated at exactly their sizes)
    cands = loc.locate([scan], 0.0, 0.0, n_angles=4)
    assert len(cands) >= 1
    loc.close()
    cmap.close()
    m.close()
    del scan
    assert live() == before


def test_occupancy_plain_and_counted(baseline):
    from yag_slam_amd import synth
    from yag_slam_amd.occupancy import create_occupancy_grid
    scene = synth.Scene()
    scans = [_scan(scene, p, p, 40 + i) for i, p in enumerate([(2.0, 3.0, 0.0), (2.1, 3.0, 0.1)])]
    for s in scans:
        s.native(0)
    before = live()
    g = create_occupancy_grid(scans, 0.1, 12.0)
    gc_ = create_occupancy_grid(scans, 0.1, 12.0, counts=True)
    assert np.array_equal(g.image, gc_.image) and gc_.passes.any()
    assert live() == before


def test_failure_paths_give_everything_back(baseline):
    """argument errors that return after the call's first buffers were allocated"""
    from yag_slam_amd import _capi
    from yag_slam_amd.scan_matching import ScanMatcher
    from yag_slam_amd.splicing import RayMap, SegmentError, SegmentMap
    before = live()
    with pytest.raises(SegmentError, match="no free pixel"):
        SegmentMap.from_map(np.zeros((64, 64), dtype=np.uint8), n_segments=2)
    assert live() == before
    rm = RayMap(_room(32, 30))
    held = live()
    with pytest.raises(_capi.YmError, match="outside the 32 x 32 image"):
        rm.trace([[40.0, 3.0]], [0.0])
    assert live() == held
    rm.close()
    assert live() == before
    m = ScanMatcher(dict(resolution=0.05, smear_deviation=0.05), semantics="yagpy")
    cmap = m.correlation_grid_from_occupancy(_room(), occupied_value=0)
    held = live()
    with pytest.raises(_capi.YmError, match="max_nodes"):  # one top-level node of 4 x 4 cells
        m.map_locator(cmap, levels=2, max_nodes=15)
    assert live() == held
    cmap.close()
    m.close()
    assert live() == before


def test_the_counts_are_back_where_the_file_found_them(baseline):
    assert live() == baseline
