"""The live occupancy grid without a device (include/yagmatch.h ym_occmap_*): the restatement in a given
frame (tests/occupancy_live_ref.py) against tests/occupancy_ref.py, the cases tests/test_gpu_occupancy_live.py compares with it
(each shown to be far from every rounding tie in ITS frame), LiveOccupancyGrid's bookkeeping against a recording stand-in for the
library, the exports, and the window and growth arithmetic as a program of its own under the sanitizers."""
import ctypes as C
import functools
import math
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

from tests import occupancy_live_ref as live_ref
from tests import occupancy_ref as ref
from tests.test_occupancy_host import ALL_FIXTURES, EXACT_ON_DEVICE, MARGIN, expected, fixture, make_scan
from tests.util import REPO

FUNCS = ("ym_occmap_create", "ym_occmap_accumulate", "ym_occmap_clear", "ym_occmap_get_info", "ym_occmap_read", "ym_occmap_read_counts",
         "ym_occmap_debug_option", "ym_occmap_destroy")

# ---- the cases of the device tests that are compared with the restatement
# no anchor given: the first batch's bounding-box minimum is the anchor; the later batches grow the window past that box towards
# smaller AND larger cells (name -> batches of scan indices; chosen on the CPU, see the test below)
OWN_ANCHOR_SPLITS = {
    "ragged_a_0.25": ((3,), (0, 1, 5), (2, 4)), "ragged_a_0.125": ((3,), (0, 1, 5), (2, 4)), "ragged_a_0.1": ((3,), (0, 1, 5), (2, 4)),
    "ragged_a_0.05": ((3,), (0, 1, 5), (2, 4)), "ragged_b_0.25": ((2,), (0,), (1,)), "ragged_b_0.125": ((2,), (0, 1)),
    "ragged_b_0.1": ((1,), (0,), (2,)), "ragged_b_0.05": ((1,), (2, 0)), "moved": ((1,), (0,), (2,)), "block": ((0,), (1, 2)),
}
ANCHOR_SHIFT = (-3.3, +2.7)  # metres from the full rendering's offset: an anchor on no scan's box, origins of both signs
SHIFTED_CASES = ("ragged_a_0.1", "ragged_b_0.05", "single_scan", "moved", "octants")
# removal: what is taken out of a grid that held the whole fixture (anchored at the shifted anchor)
REMOVE_CASES = {"ragged_a_0.125": (1, 4, 5), "ragged_b_0.1": (0,), "block": (2, 0)}
MOVE_BY = (0.37, -0.21, 0.4)  # the "moved" fixture's scans start this far from the fixture's poses (as test_gpu_occupancy moves them)


def own_anchor(name):
    scans, res, rt = fixture(name)
    off_x, off_y, _, _ = ref._frame([scans[i] for i in OWN_ANCHOR_SPLITS[name][0]], res, rt)
    return (off_x, off_y)


def shifted_anchor(name):
    off = expected(name)[3]
    return (off[0] + ANCHOR_SHIFT[0], off[1] + ANCHOR_SHIFT[1])


def moved_from(name="moved"):
    """the fixture's scans at their FIRST poses (copies: the fixture's own scans are shared and stay put)"""
    scans, res, rt = fixture(name)
    new = np.array([(s.corrected_pose.x, s.corrected_pose.y, s.corrected_pose.euler[-1]) for s in scans])
    return [make_scan(s.ranges, p) for s, p in zip(scans, new + np.array(MOVE_BY))], new


# ---- ray-length edges of the wave-per-ray trace: hand-made scans at ONE pose, one per ray length (a scan's beams are evenly spaced in
# angle, so every scan is a fan of 4096 directions of which a few carry a reading), the sensor a quarter cell off the lattice
EDGE_RES, EDGE_RT, EDGE_BEAMS = 0.1, 18.5, 4096
EDGE_LENGTHS = (0, 1, 62, 63, 64, 65, 127, 128, 129)  # cells along the major axis
EDGE_SENSOR_CELL = (200, 180)
EDGE_ANCHOR = (-1.7, 2.3)


def _edge_targets(length):
    if length == 0:
        return [(0, 0)]
    out = []
    for sx in (1, -1):
        for sy in (1, -1):
            out += [(sx * length, sy * length), (sx * length, sy * (length - 1)), (sx * (length - 1), sy * length),
                    (sx * length, sy * (length // 3)), (sx * (length // 3), sy * length)]
    return sorted(set(out + [(length, 0), (-length, 0), (0, length), (0, -length)]))


@functools.lru_cache(maxsize=None)
def edge_scans():
    """-> (scans, resolution, range_threshold, anchor): per length a fan whose readings end `length` cells from the sensor along the major
    axis in every octant (dx = dy, one less on the minor axis, one less on the major side's other axis, a third, axis-aligned), and a
    last fan of readings beyond the threshold, clipped at 185 cells: they leave the window, which ends at 129"""
    inc = 2 * math.pi / EDGE_BEAMS
    pose = (EDGE_ANCHOR[0] + (EDGE_SENSOR_CELL[0] + 0.25) * EDGE_RES, EDGE_ANCHOR[1] + (EDGE_SENSOR_CELL[1] + 0.25) * EDGE_RES, 0.0)
    scans = []
    for length in EDGE_LENGTHS:
        r = np.zeros(EDGE_BEAMS)
        for dx, dy in _edge_targets(length):
            beam = int(round((math.atan2(dy, dx) + math.pi) / inc)) % EDGE_BEAMS
            assert r[beam] == 0.0, (length, dx, dy)
            r[beam] = math.hypot(dx, dy) * EDGE_RES if (dx, dy) != (0, 0) else 0.02
        scans.append(make_scan(r, pose, min_angle=-math.pi, inc=inc, min_range=0.005, max_range=40.0))
    r = np.zeros(EDGE_BEAMS)
    r[5::256] = 20.0
    r[133::512] = 39.0
    scans.append(make_scan(r, pose, min_angle=-math.pi, inc=inc, min_range=0.005, max_range=40.0))
    return tuple(scans), EDGE_RES, EDGE_RT, EDGE_ANCHOR


# ---------------------------------------------------------------------------------------------------------------- tests
@pytest.mark.parametrize("name", ALL_FIXTURES)
def test_restatement_in_render_frame_is_the_restatement(name):
    scans, res, rt = fixture(name)
    image, passes, hits, off = expected(name)
    assert live_ref.frame_of(scans, res, rt, off) == ((0, 0), image.shape[1], image.shape[0])
    got = live_ref.render_in_frame(scans, res, rt, off, (0, 0), image.shape[1], image.shape[0])
    assert np.array_equal(got[0], image) and np.array_equal(got[1], passes) and np.array_equal(got[2], hits)
    assert got[1].dtype == np.uint32 and got[2].dtype == np.uint32 and got[0].dtype == np.uint8


def test_a_shifted_frame_shifts_the_counts_when_the_anchor_moves_by_whole_cells():
    """an anchor k cells away and an origin of k: the same lattice up to fp64 rounding of the subtraction, on a fixture whose
    margin dwarfs it; a window cut out of it holds the matching part"""
    scans, res, rt = fixture("ragged_b_0.25")
    image, passes, hits, off = expected("ragged_b_0.25")
    anchor = (off[0] - 7 * res, off[1] - 3 * res)
    assert live_ref.tie_margin_in_frame(scans, res, rt, anchor) >= 1e-7
    origin, w, h = live_ref.frame_of(scans, res, rt, anchor)
    assert (origin, w, h) == ((7, 3), image.shape[1], image.shape[0])
    got = live_ref.render_in_frame(scans, res, rt, anchor, origin, w, h)
    assert np.array_equal(got[1], passes) and np.array_equal(got[2], hits) and np.array_equal(got[0], image)
    part = live_ref.render_in_frame(scans, res, rt, anchor, (12, 1), 9, 11)
    full = live_ref.render_in_frame(scans, res, rt, anchor, (0, 0), w + 8, h + 4)
    assert np.array_equal(part[1], full[1][1:12, 12:21]) and np.array_equal(part[2], full[2][1:12, 12:21])
    assert full[1][:3].sum() >= 0 and np.array_equal(full[1][3:3 + h, 7:7 + w] >= passes, np.ones_like(passes, bool))


def _margin(scans, res, rt, anchor, box_scans=None):
    m = live_ref.tie_margin_in_frame(scans, res, rt, anchor, box_scans)
    assert m >= MARGIN, m
    return m


@pytest.mark.parametrize("name", sorted(OWN_ANCHOR_SPLITS))
def test_own_anchor_cases_are_far_from_ties_and_grow_both_ways(name):
    scans, res, rt = fixture(name)
    split = OWN_ANCHOR_SPLITS[name]
    assert sorted(i for b in split for i in b) == list(range(len(scans)))
    anchor = own_anchor(name)
    print("margin(%s, own anchor) = %.3g" % (name, _margin(scans, res, rt, anchor)))
    first = [scans[i] for i in split[0]]
    (ox, oy), w, h = live_ref.frame_of(scans, res, rt, anchor)
    o1, w1, h1 = live_ref.frame_of(first, res, rt, anchor)
    assert o1 == (0, 0)
    # along at least one axis the window outgrows the first batch's box towards smaller AND towards larger cells
    assert (ox < 0 and ox + w > w1) or (oy < 0 and oy + h > h1), ((ox, oy), (w, h), (w1, h1))


@pytest.mark.parametrize("name", SHIFTED_CASES)
def test_shifted_anchor_cases_are_far_from_ties(name):
    scans, res, rt = fixture(name)
    anchor = shifted_anchor(name)
    print("margin(%s, shifted anchor) = %.3g" % (name, _margin(scans, res, rt, anchor)))
    (ox, oy), w, h = live_ref.frame_of(scans, res, rt, anchor)
    assert ox > 0 and oy < 0 and (h, w) == expected(name)[0].shape


@pytest.mark.parametrize("name", sorted(REMOVE_CASES))
def test_removal_cases_are_far_from_ties(name):
    scans, res, rt = fixture(name)
    anchor = shifted_anchor(name)
    rest = [s for i, s in enumerate(scans) if i not in REMOVE_CASES[name]]
    assert rest and len(rest) < len(scans)
    _margin(scans, res, rt, anchor)
    _margin(rest, res, rt, anchor, box_scans=scans)  # what is left, in the window of everything that was ever added


def test_move_cases_are_far_from_ties():
    scans, res, rt = fixture("moved")
    first, new = moved_from()
    anchor = shifted_anchor("moved")
    _margin(first, res, rt, anchor)
    _margin(scans, res, rt, anchor, box_scans=list(scans) + first)   # after the move, in the window of both
    # one scan of three moved (sync updates): scans 0 and 1 at their first poses, scan 2 at its second, in the window of all four
    nudged = [first[0], first[1], scans[2]]
    _margin(nudged, res, rt, anchor, box_scans=first + [scans[2]])
    assert not np.allclose(new, new + np.array(MOVE_BY))


def test_edge_scans_hold_every_ray_length_in_every_octant():
    scans, res, rt, anchor = edge_scans()
    print("margin(edge scans) = %.3g" % _margin(list(scans), res, rt, anchor))
    assert len(scans) == len(EDGE_LENGTHS) + 1
    for scan, length in zip(scans, EDGE_LENGTHS):
        (start, ends, valid), = ref._rays([scan], res, rt, anchor[0], anchor[1])
        assert np.allclose(start - np.floor(start), 0.25, atol=1e-9)  # a quarter cell off the lattice
        s = ref.round_half_away(start)
        assert tuple(s.astype(int)) == EDGE_SENSOR_CELL
        d = (ref.round_half_away(ends) - s).astype(int)
        assert sorted(map(tuple, d.tolist())) == _edge_targets(length), length   # every reading ends in the cell it was made for
        assert np.all(np.abs(d).max(axis=1) == length) and valid.all()
        if length >= 2:
            kinds = {(abs(dy) > abs(dx), dx > 0, dy > 0) for dx, dy in d.tolist() if dx and dy and abs(dx) != abs(dy)}
            assert len(kinds) == 8, (length, kinds)                              # all eight octants
            assert sum(abs(dx) == abs(dy) for dx, dy in d.tolist()) == 4          # dx = dy, every quadrant
            assert sum(abs(dy) == abs(dx) + 1 for dx, dy in d.tolist()) == 4      # steep by one
            assert sum(abs(dx) == abs(dy) + 1 for dx, dy in d.tolist()) == 4      # shallow by one
    (start, ends, valid), = ref._rays([scans[-1]], res, rt, anchor[0], anchor[1])
    reach = np.abs(ref.round_half_away(ends) - ref.round_half_away(start)).max(axis=1)
    assert len(ends) == 24 and not valid.any() and reach.max() == 185 and reach.min() >= 99
    (ox, oy), w, h = live_ref.frame_of(list(scans), res, rt, anchor)
    assert (ox, oy) == (EDGE_SENSOR_CELL[0] - 129, EDGE_SENSOR_CELL[1] - 129) and (w, h) == (258, 258)
    cells = ref.round_half_away(ends) - np.array([ox, oy])
    outside = (cells[:, 0] < 0) | (cells[:, 0] >= w) | (cells[:, 1] < 0) | (cells[:, 1] >= h)
    assert outside.sum() >= 16   # the clipped rays leave the window


def test_closed_form_of_the_walk_in_32_bits():
    """the kernel evaluates m(k) = (2 k dm + dM) / (2 dM) in unsigned 32-bit integers below dM = 2^15: the largest numerator fits"""
    d = 32767
    assert 2 * d * d + d < 2 ** 31
    xs, ys = ref.line_cells(3, -2, 3 + d, -2 - d + 1)
    assert xs[-1] == 3 + d and ys[-1] == -2 - d + 1 and len(xs) == d + 1
    k = np.arange(d + 1, dtype=np.uint32)
    m32 = (k * np.uint32(2 * (d - 1)) + np.uint32(d)) // np.uint32(2 * d)
    assert np.array_equal(-2 - m32.astype(np.int64), ys)


# ---- exports and layout
def test_exports_argtypes_and_info_layout_match_the_header(tmp_path):
    from yag_slam_amd import _capi, occupancy
    L = _capi.lib()
    hdr = open(os.path.join(REPO, "include", "yagmatch.h")).read()
    code = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    for f in FUNCS:
        assert re.search(r"\b%s\s*\(" % f, code), f
        assert f in _capi.EXPORTS and hasattr(L, f), f
    assert hasattr(occupancy, "LiveOccupancyGrid")
    from yag_slam_amd.mapping import LoopClosingMapper
    assert callable(LoopClosingMapper.live_ros_map)
    vp, dp = C.c_void_p, C.POINTER(C.c_double)
    assert list(L.ym_occmap_create.argtypes) == [C.c_int, C.c_double, C.c_double, dp, C.c_int] and L.ym_occmap_create.restype is vp
    assert list(L.ym_occmap_accumulate.argtypes) == [vp, C.POINTER(vp), dp, C.c_int, C.c_int]
    assert list(L.ym_occmap_read.argtypes) == [vp, C.POINTER(C.c_uint8), C.c_int64, C.POINTER(_capi.YmDespeckleOpts),
                                               C.POINTER(_capi.YmDespeckleStats)]
    assert list(L.ym_occmap_read_counts.argtypes) == [vp, C.POINTER(C.c_uint32), C.POINTER(C.c_uint32), C.c_int64]
    cc = shutil.which("cc") or shutil.which("gcc") or shutil.which("clang")
    assert cc, "no C compiler to read the header with"
    protos = """
ym_occmap *(*p_create)(int, double, double, const double *, int) = ym_occmap_create;
int (*p_acc)(ym_occmap *, const ym_scan *const *, const double *, int, int) = ym_occmap_accumulate;
int (*p_clear)(ym_occmap *) = ym_occmap_clear;
int (*p_info)(const ym_occmap *, ym_occmap_info *) = ym_occmap_get_info;
int (*p_read)(ym_occmap *, uint8_t *, int64_t, const ym_despeckle_opts *, ym_despeckle_stats *) = ym_occmap_read;
int (*p_counts)(ym_occmap *, uint32_t *, uint32_t *, int64_t) = ym_occmap_read_counts;
int (*p_opt)(ym_occmap *, int, int) = ym_occmap_debug_option;
void (*p_destroy)(ym_occmap *) = ym_occmap_destroy;
"""
    lines = ['printf("ym_occmap_info %zu\\n", sizeof(ym_occmap_info));']
    for fname, _ in _capi.YmOccmapInfo._fields_:
        lines.append('printf("%s %%zu\\n", offsetof(ym_occmap_info, %s));' % (fname, fname))
    src = tmp_path / "layout.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "yagmatch.h"\n%s\nint main(void) {\n%s\nreturn 0; }\n'
                   % (protos, "\n".join(lines)))
    stub = tmp_path / "stubs.c"  # (the entries are only named, never called)
    stub.write_text("".join("int %s(void) { return 0; }\n" % f for f in FUNCS))
    obj, exe = str(tmp_path / "layout.o"), str(tmp_path / "layout")
    subprocess.run([cc, "-Wall", "-Werror", "-I", os.path.join(REPO, "include"), "-c", "-o", obj, str(src)], check=True, capture_output=True)
    subprocess.run([cc, "-o", exe, obj, str(stub)], check=True, capture_output=True)
    seen = dict(l.split() for l in subprocess.run([exe], check=True, capture_output=True, text=True).stdout.splitlines())
    assert int(seen["ym_occmap_info"]) == C.sizeof(_capi.YmOccmapInfo)
    for fname, _ in _capi.YmOccmapInfo._fields_:
        assert int(seen[fname]) == getattr(_capi.YmOccmapInfo, fname).offset, fname


def test_no_device_fails_loudly():
    from yag_slam_amd import _capi
    from yag_slam_amd.occupancy import LiveOccupancyGrid
    L = _capi.lib()
    assert not L.ym_occmap_create(0, 0.0, 12.0, None, 64) and "resolution and range_threshold must be > 0" in _capi.last_error()
    assert not L.ym_occmap_create(0, 0.05, float("nan"), None, 64) and "must be > 0" in _capi.last_error()
    assert not L.ym_occmap_create(0, 1e-6, 100.0, None, 64) and "below 2^24 cells" in _capi.last_error()
    assert not L.ym_occmap_create(0, 0.05, 12.0, None, -1) and "slack_cells -1" in _capi.last_error()
    assert not L.ym_occmap_create(0, 0.05, 12.0, (C.c_double * 2)(0.0, float("inf")), 0) and "anchor: not finite" in _capi.last_error()
    assert L.ym_occmap_accumulate(None, None, None, 0, 1) == -1 and "null occupancy map" in _capi.last_error()
    assert L.ym_occmap_read(None, None, 0, None, None) == -1 and L.ym_occmap_get_info(None, None) == -1
    L.ym_occmap_destroy(None)
    if L.ym_device_count() > 0:
        return
    g = LiveOccupancyGrid(0.05, 12.0)   # (making the object touches nothing)
    with pytest.raises(_capi.YmError, match="no HIP device"):
        g.info


# ---- LiveOccupancyGrid's bookkeeping against a stand-in for the library
class _Scan(object):
    serial = 1000

    def __init__(self, x, y, t):
        from yag_slam_amd.transform import Transform
        self.corrected_pose = Transform(x, y, 0.0, t)
        _Scan.serial += 1
        self.handle = _Scan.serial

    def native(self, device=0):
        return self.handle

    def move(self, x, y, t):
        from yag_slam_amd.transform import Transform
        self.corrected_pose = Transform(x, y, 0.0, t)


def _bare_grid(**kw):
    """a LiveOccupancyGrid whose library calls are recorded instead of made"""
    from yag_slam_amd.occupancy import LiveOccupancyGrid
    g = LiveOccupancyGrid(0.05, 12.0, **kw)
    g.calls = []

    def native():
        raise AssertionError("the library was touched")

    g._native = native
    g._accumulate = lambda entries, sign: g.calls.append((sign, [tuple(e) for e in entries])) if entries else None
    g.clear = lambda: (g.calls.append(("clear",)), g._held.clear())[0]
    return g


def test_constructor_refuses_bad_arguments_before_the_library():
    from yag_slam_amd.occupancy import LiveOccupancyGrid
    for bad in ((0.0, 12.0), (-0.05, 12.0), (0.05, 0.0), (float("nan"), 12.0), (0.05, float("inf"))):
        with pytest.raises(ValueError, match="must be > 0"):
            LiveOccupancyGrid(*bad)
    for bad in (-1, 1.5, True, "64"):
        with pytest.raises(ValueError, match="slack_cells"):
            LiveOccupancyGrid(0.05, 12.0, slack_cells=bad)
    for bad in ((1.0,), (1.0, float("nan")), (0.0, 1.0, 2.0)):
        with pytest.raises(ValueError, match="anchor"):
            LiveOccupancyGrid(0.05, 12.0, anchor=bad)
    g = LiveOccupancyGrid(0.05, 12, anchor=[1, 2], slack_cells=np.int64(0))
    assert g.anchor == (1.0, 2.0) and g.slack_cells == 0 and g._h is None and len(g) == 0
    with pytest.raises(ValueError, match="trace form"):
        g._set_trace_form(2)


def test_membership_errors_come_before_the_library_and_change_nothing():
    g = _bare_grid()
    a, b, c = _Scan(0, 0, 0), _Scan(1, 0, 0), _Scan(2, 0, 0)
    g.add([]), g.remove([]), g.add(())
    assert g.calls == [] and g.sync([]) == "none"
    g.add([a, b])
    assert len(g) == 2 and a in g and b in g and c not in g
    before = list(g.calls)
    with pytest.raises(ValueError, match="scan 1 is already held"):
        g.add([c, a])
    with pytest.raises(ValueError, match="scan 1 is in the list twice"):
        g.add([c, c])
    with pytest.raises(ValueError, match="scan 0 is not held"):
        g.remove([c])
    with pytest.raises(ValueError, match="scan 1 is in the list twice"):
        g.remove([a, a])
    with pytest.raises(ValueError, match="element 1 is not a LocalizedRangeScan"):
        g.add([c, None])
    with pytest.raises(ValueError, match="element 0 is not a LocalizedRangeScan"):
        g.sync([17])
    assert g.calls == before and len(g) == 2 and c not in g


def test_removal_subtracts_the_pose_the_scan_was_added_at():
    g = _bare_grid()
    a, b = _Scan(0.5, 1.5, 0.25), _Scan(1.0, 0.0, -0.5)
    g.add([a, b])
    assert g.calls == [(+1, [(a.handle, (0.5, 1.5, 0.25)), (b.handle, (1.0, 0.0, -0.5))])]
    a.move(9.0, 9.0, 1.0)           # whatever happens to the scan's pose afterwards
    g.remove([a])
    assert g.calls[-1] == (-1, [(a.handle, (0.5, 1.5, 0.25))]) and a not in g and b in g
    g.add([a])
    assert g.calls[-1] == (+1, [(a.handle, (9.0, 9.0, 1.0))])


def test_sync_picks_its_route_and_touches_only_what_changed():
    g = _bare_grid()
    scans = [_Scan(float(i), 0.0, 0.0) for i in range(10)]
    assert g.sync(scans) == "rebuild" and g.calls[0] == ("clear",) and g.calls[1][0] == +1 and len(g.calls[1][1]) == 10
    assert g.sync(scans) == "none" and len(g.calls) == 2
    # five new of fifteen, one gone, one moved: 6 to trace of 14 -> update; the rest untouched
    more = [_Scan(float(i), 1.0, 0.0) for i in range(5)]
    scans[3].move(3.0, 0.5, 0.1)
    target = [s for s in scans if s is not scans[7]] + more
    assert g.sync(target) == "update"
    out, into = g.calls[-2], g.calls[-1]
    assert out == (-1, [(scans[7].handle, (7.0, 0.0, 0.0)), (scans[3].handle, (3.0, 0.0, 0.0))])
    assert into[0] == +1 and into[1][0] == (scans[3].handle, (3.0, 0.5, 0.1)) and [e[0] for e in into[1][1:]] == [s.handle for s in more]
    assert len(g) == 14 and scans[7] not in g and g.sync(target) == "none"
    # exactly half re-traced stays an update; one more than half rebuilds
    for s in target[:7]:
        s.move(s.corrected_pose.x, 2.0, 0.0)
    n = len(g.calls)
    assert g.sync(target) == "update" and len(g.calls) == n + 2 and len(g.calls[-1][1]) == 7
    for s in target[:8]:
        s.move(s.corrected_pose.x, 3.0, 0.0)
    assert g.sync(target) == "rebuild" and g.calls[-2] == ("clear",) and len(g.calls[-1][1]) == 14
    # only removals: an update that adds nothing
    assert g.sync(target[:10]) == "update" and g.calls[-1][0] == -1 and len(g.calls[-1][1]) == 4 and len(g) == 10
    assert g.sync([]) == "rebuild" and len(g) == 0


def test_mapper_makes_one_grid_per_resolution_and_threshold():
    from yag_slam_amd import occupancy
    from yag_slam_amd.mapping import LoopClosingMapper

    made = []

    class _Grid(object):
        def __init__(self, resolution, range_threshold, device=0):
            self.resolution, self.range_threshold, self.device = float(resolution), float(range_threshold), device
            self.synced, self.closed = [], False
            made.append(self)

        def sync(self, scans):
            self.synced.append(list(scans))

        def ros_map(self, **kw):
            return ("map", self, kw)

        def close(self):
            self.closed = True

    class _Matcher(object):
        device = 3

    real = occupancy.LiveOccupancyGrid
    occupancy.LiveOccupancyGrid = _Grid
    try:
        mp = LoopClosingMapper(_Matcher(), None)
        mp.scans = ["s0", "s1"]
        assert mp.live_ros_map() == ("map", made[0], {}) and made[0].device == 3 and (made[0].resolution, made[0].range_threshold) == (0.05, 12.0)
        mp.scans.append("s2")
        assert mp.live_ros_map(min_area=3)[2] == {"min_area": 3} and len(made) == 1 and made[0].synced == [["s0", "s1"], ["s0", "s1", "s2"]]
        mp.live_ros_map(resolution=0.1)
        assert len(made) == 2 and made[0].closed and made[1].resolution == 0.1 and mp.live_grid is made[1]
        mp.live_ros_map(resolution=0.1, range_threshold=8)
        assert len(made) == 3 and made[1].closed and not made[2].closed
    finally:
        occupancy.LiveOccupancyGrid = real


# ---- the window and growth arithmetic under the sanitizers, as a program of its own
def test_window_arithmetic_under_the_sanitizers(tmp_path):
    cxx = shutil.which("c++") or shutil.which("g++") or shutil.which("clang++")
    assert cxx, "no C++ compiler"
    exe = str(tmp_path / "occlive_window_check")
    cmd = [cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-Wall", "-Wextra", "-Werror",
           "-I", os.path.join(REPO, "yag_slam_amd", "csrc"), "-o", exe, os.path.join(REPO, "tests", "native", "occlive_window_check.cpp")]
    # the sanitizers' runtimes inside the program (gcc's spelling, then clang's): it runs whatever else the process environment loads
    for static in (["-static-libasan", "-static-libubsan"], ["-static-libsan"]):
        built = subprocess.run(cmd + static, capture_output=True, text=True)
        if built.returncode == 0:
            break
    assert built.returncode == 0, built.stderr[-2000:]
    run = subprocess.run([exe, "3000"], capture_output=True, text=True)
    assert run.returncode == 0, (run.stdout[-2000:], run.stderr[-2000:])
    words = run.stdout.split()
    assert words[0] == "ok" and int(words[1]) == 3000 and int(words[2]) > 3000
