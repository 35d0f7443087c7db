"""Maps whose window moves, without a device (include/yagmatch.h ym_map_reframe / ym_map_window / ym_map_create_counted_window,
DESIGN.md section 17): the ABI against the header read through a C compiler, the refusals that need no device, the numpy
restatement (tests/mapreframe_ref.py) against itself -- reframing equals restating in the new window, a scroll and its inverse is
the identity, a copied cell stands exactly where its neighbourhood meets both windows alike --, CorrelationMap.reframe's
bookkeeping with a stub library, and MapBuilder's extent policy with stubs."""
import ctypes as C
import os
import re
import shutil
import subprocess
import types

import numpy as np
import pytest

from tests import mapforget_ref as F
from tests import mapgrow_ref as R
from tests import mapreframe_ref as W
from tests.test_map_forget_host import (_CountedStubMap, _FixtureScan, _KeyScan, _PlainStubMap, _Pose, _Scan, _StubLib, _StubMatcher,
                                        _StubScanMatcher, _bare_map, _tf)
from tests.util import GOLDEN, REPO

FUNCS = ("ym_map_reframe", "ym_map_window", "ym_map_create_counted_window")

# what yag_slam_amd/_capi.py declares, spelled as C prototypes (see tests/test_map_grow_host.py)
PROTOS = """
int (*p_reframe)(ym_matcher *, ym_map *, int, int, int, int, const ym_scan *const *, const double *, int,
                 ym_map_reframe_stats *) = ym_map_reframe;
int (*p_window)(const ym_map *, int *, int *, int *, int *) = ym_map_window;
ym_map *(*p_create)(ym_matcher *, int, int, double, double, int, int) = ym_map_create_counted_window;
"""


def test_exports_argtypes_and_stats_layout_match_the_header(tmp_path):
    from yag_slam_amd import _capi
    L = _capi.lib()
    hdr = open(os.path.join(REPO, "include", "yagmatch.h")).read()
    code = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    for f in FUNCS:
        assert re.search(r"\b%s\s*\(" % f, code), f
        assert f in _capi.EXPORTS and hasattr(L, f), f
    vp, ip = C.c_void_p, C.POINTER(C.c_int32)
    assert list(L.ym_map_reframe.argtypes) == [vp, vp, C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(vp), C.POINTER(C.c_double), C.c_int,
                                               C.POINTER(_capi.YmMapReframeStats)]
    assert list(L.ym_map_window.argtypes) == [vp, ip, ip, ip, ip]
    assert L.ym_map_create_counted_window.restype is vp
    assert list(L.ym_map_create_counted_window.argtypes) == [vp, C.c_int, C.c_int, C.c_double, C.c_double, C.c_int, C.c_int]
    assert L.ym_version() == 1
    cc = shutil.which("cc") or shutil.which("gcc") or shutil.which("clang")
    assert cc, "no C compiler to read the header with"
    lines = ['printf("ym_map_reframe_stats %zu\\n", sizeof(ym_map_reframe_stats));',
             'printf("ym_map_update_stats %zu\\n", sizeof(ym_map_update_stats));']
    for fname, _ in _capi.YmMapReframeStats._fields_:
        lines.append('printf("%s %%zu\\n", offsetof(ym_map_reframe_stats, %s));' % (fname, fname))
    src = tmp_path / "layout.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "yagmatch.h"\n%s\nint main(void) {\n%s\nreturn 0; }\n'
                   % (PROTOS, "\n".join(lines)))
    obj = str(tmp_path / "layout.o")
    subprocess.run([cc, "-Wall", "-Werror", "-I", os.path.join(REPO, "include"), "-c", "-o", obj, str(src)], check=True, capture_output=True)
    exe = str(tmp_path / "layout")
    stub = tmp_path / "stubs.c"  # (the entries are only named, never called: the program links against empty stand-ins)
    stub.write_text("".join("int %s(void) { return 0; }\n" % f for f in FUNCS))
    subprocess.run([cc, "-o", exe, obj, str(stub)], check=True, capture_output=True)
    seen = dict(l.split() for l in subprocess.run([exe], check=True, capture_output=True, text=True).stdout.splitlines())
    assert int(seen["ym_map_reframe_stats"]) == C.sizeof(_capi.YmMapReframeStats) == 5 * 8 + 4 * 4
    assert int(seen["ym_map_update_stats"]) == 6 * 8 + 4 * 4  # (the existing struct keeps its pinned size)
    assert [f for f, _ in _capi.YmMapReframeStats._fields_] == ["kept", "restamped", "dropped", "recomputed", "mismatch", "x0", "y0",
                                                                "width", "height"]
    for fname, _ in _capi.YmMapReframeStats._fields_:
        assert int(seen[fname]) == getattr(_capi.YmMapReframeStats, fname).offset, fname


def test_null_negative_and_oversize_arguments_are_refused_before_any_device_is_touched():
    from yag_slam_amd import _capi
    L = _capi.lib()
    st = _capi.YmMapReframeStats()
    one = (C.c_void_p * 1)()
    poses = (C.c_double * 3)()
    fake = C.c_void_p(16)  # never dereferenced: the argument beside it is refused first
    assert L.ym_map_reframe(None, None, 1, 1, 8, 8, one, poses, 1, C.byref(st)) == -1 and "null" in _capi.last_error()
    assert L.ym_map_reframe(fake, None, 1, 1, 8, 8, None, None, 0, None) == -1 and "null" in _capi.last_error()
    assert L.ym_map_reframe(None, fake, 1, 1, 8, 8, None, None, 0, None) == -1 and "null" in _capi.last_error()
    # a held list that is said to hold something and is null, its poses among them
    assert L.ym_map_reframe(fake, fake, 1, 1, 8, 8, None, poses, 1, None) == -1 and "null" in _capi.last_error()
    assert L.ym_map_reframe(fake, fake, 1, 1, 8, 8, one, None, 1, None) == -1 and "null" in _capi.last_error()
    assert L.ym_map_reframe(fake, fake, 1, 1, 8, 8, one, poses, -1, None) == -1 and "negative" in _capi.last_error()
    for w, h in ((0, 8), (8, 0), (-3, 8), (8, -3), (40000, 40000)):
        assert L.ym_map_reframe(fake, fake, 1, 1, w, h, None, None, 0, C.byref(st)) == -1 and "size" in _capi.last_error(), (w, h)
    assert L.ym_map_window(None, None, None, None, None) == -1 and "null" in _capi.last_error()
    assert not L.ym_map_create_counted_window(None, 8, 8, 0.0, 0.0, 3, -4) and "null matcher" in _capi.last_error()
    for x0, y0 in ((2 ** 30 + 1, 0), (0, -2 ** 30 - 1)):
        assert not L.ym_map_create_counted_window(fake, 8, 8, 0.0, 0.0, x0, y0) and "offset" in _capi.last_error()


# ---- the restatement against itself --------------------------------------------------------------------------------------------
def _fixture():
    z = np.load(os.path.join(GOLDEN, "map_grow.npz"))
    res, anchor = float(z["res"]), (float(z["ox"]), float(z["oy"]))
    a, b = (_FixtureScan(z, r, p) for r, p in zip(z["ranges"], z["poses"]))
    c = _FixtureScan(z, z["ranges"][0], (z["poses"][0][0] + 0.131, z["poses"][0][1] - 0.087, z["poses"][0][2] + 0.05))
    for s in (a, b, c):
        assert R.distance_to_half(*s.points(), anchor[0], anchor[1], res) > R.HALF_GUARD
    return z, res, anchor, [a, b, c]


def test_the_window_at_offset_zero_is_the_map_of_before_and_cells_are_lattice_cells_minus_the_offset():
    z, res, anchor, scans = _fixture()
    w, h = int(z["width"]), int(z["height"])
    cells, dropped = W.window_cells(scans, anchor, res, (0, 0, w, h))
    assert cells == F.cells_of(scans, (h, w), anchor[0], anchor[1], res) and len(cells) > 60
    assert dropped == sum(len(s.points()[0]) for s in scans) - len(cells)
    grid, counts = W.build(z["kernel"], scans, anchor, res, (0, 0, w, h))
    assert np.array_equal(grid, R.build((h, w), z["kernel"], scans, anchor[0], anchor[1], res)[0])
    win = (-7, 5, w + 3, h - 2)
    lat = W.lattice_cells(scans, anchor, res)
    inside = [(x + 7, y - 5) for x, y in lat if -7 <= x < -7 + w + 3 and 5 <= y < 5 + h - 2]
    assert W.window_cells(scans, anchor, res, win)[0] == inside and 0 < len(inside) < len(lat)
    assert W.origin(anchor, win, res) == (anchor[0] + -7 * res, anchor[1] + 5 * res)
    # the trap of a map re-created at a shifted ORIGIN: its own quotient rounds a reading near a tie into another cell than the
    # lattice cell minus the offset.  Found by search near the tie, so that the restatement's rule is shown to differ from it
    k, hit = 13, None
    for i in range(1, 4000):
        x = anchor[0] + (i + 0.5) * res
        for x in (np.nextafter(x, -np.inf), x, np.nextafter(x, np.inf)):
            if np.round((x - (anchor[0] + k * res)) / res) != np.round((x - anchor[0]) / res) - k:
                hit = x
        if hit is not None:
            break
    assert hit is not None, "no reading near a tie tells the two roundings apart"


def test_reframing_the_restatement_equals_restating_in_the_new_window():
    z, res, anchor, scans = _fixture()
    kernel = z["kernel"]
    half = kernel.shape[0] // 2
    w, h = int(z["width"]), int(z["height"])
    # the fixture's map is larger than its scans reach: start from a window some of their readings lie outside of
    lat = np.array(W.lattice_cells(scans, anchor, res))
    lo, hi = lat.min(axis=0), lat.max(axis=0)
    start = (int(lo[0]) + 6, int(lo[1]) + 4, int(hi[0] - lo[0]) - 9, int(hi[1] - lo[1]) - 7)
    grid0, counts0 = W.build(kernel, scans, anchor, res, start)
    assert W.window_cells(scans, anchor, res, start)[1] > 0
    moves = [(13, -7, None, None), (-13, 7, None, None), (-9, -6, start[2] + 20, start[3] + 15), (5, 4, start[2] - 11, start[3] - 9),
             (10 * w, 0, None, None), (0, 0, None, None)]
    for dx, dy, nw, nh in moves:
        new = W.moved(start, dx, dy, nw, nh)
        got, st = W.reframe_counted(counts0, scans, anchor, res, start, dx, dy, nw, nh)
        want_grid, want = W.build(kernel, scans, anchor, res, new)
        assert np.array_equal(got, want) and st["mismatch"] == 0, (dx, dy)
        assert st["dropped"] == W.window_cells(scans, anchor, res, new)[1]
        assert int(got.sum()) == int(W.shifted(counts0, dx, dy, new[2], new[3]).sum()) + st["restamped"]
        # a copied value stands exactly where the neighbourhood meets both windows alike; elsewhere some cell differs in some case
        copied = W.shifted(grid0, dx, dy, new[2], new[3])
        touched = W.touches_difference(start, new, half)
        assert np.array_equal(copied[~touched], want_grid[~touched]), (dx, dy)
        if (dx, dy, nw, nh) == (0, 0, None, None):
            assert not touched.any() and st["kept"] == start[2] * start[3] and st["restamped"] == 0
        if dx == 10 * w:
            assert st["kept"] == 0 and not got.any() and touched.all()
    # the grow is not vacuous, and the crop loses taps at a border: an overlap cell differs from the plain crop of the old grid
    assert W.reframe_counted(counts0, scans, anchor, res, start, -9, -6, start[2] + 20, start[3] + 15)[1]["restamped"] > 0
    crop = W.moved(start, 5, 4, start[2] - 11, start[3] - 9)
    assert (W.shifted(grid0, 5, 4, crop[2], crop[3]) != W.build(kernel, scans, anchor, res, crop)[0]).any()
    # wrong poses: what the kept cells count is not what the held scans put there
    far = [_FixtureScan(z, s.ranges, (s.pose[0] + 40 * w * res, s.pose[1], s.pose[2])) for s in scans]
    assert W.reframe_counted(counts0, far, anchor, res, start, 13, -7, None, None)[1]["mismatch"] == int(
        W.shifted(counts0, 13, -7, start[2], start[3]).sum()) > 0


def test_a_scroll_and_its_inverse_is_the_identity():
    z, res, anchor, scans = _fixture()
    lat = np.array(W.lattice_cells(scans, anchor, res))
    lo, hi = lat.min(axis=0), lat.max(axis=0)
    start = (int(lo[0]) + 6, int(lo[1]) + 4, int(hi[0] - lo[0]) - 9, int(hi[1] - lo[1]) - 7)
    counts0 = W.counts(scans, anchor, res, start)
    away, st = W.reframe_counted(counts0, scans, anchor, res, start, 13, -7, None, None)
    assert st["dropped"] != W.window_cells(scans, anchor, res, start)[1] or not np.array_equal(away, counts0)
    back, st = W.reframe_counted(away, scans, anchor, res, W.moved(start, 13, -7), -13, 7, None, None)
    assert np.array_equal(back, counts0) and st["mismatch"] == 0
    assert np.array_equal(F.from_counts(back, z["kernel"]), F.from_counts(counts0, z["kernel"]))
    # an array without counts only loses: away and back keeps the overlap of the two and nothing else
    g = F.from_counts(counts0, z["kernel"])
    there_and_back = W.shifted(W.shifted(g, 13, -7, start[2], start[3]), -13, 7, start[2], start[3])
    keep = np.zeros_like(g, dtype=bool)
    keep[:start[3] - 7, 13:] = True
    assert np.array_equal(there_and_back, np.where(keep, g, 0.0)) and (g[~keep] != 0).any()
    # the origin after many moves is the anchor plus the whole offset, not a running sum
    win, run = start, W.origin(anchor, start, res)[0]
    for _ in range(500):
        win = W.moved(win, 13, -7)
        run = run + 13 * res
    assert W.origin(anchor, win, res)[0] == anchor[0] + (start[0] + 500 * 13) * res
    assert run != W.origin(anchor, win, res)[0], "this fixture's resolution does not show the drift of a running sum"


# ---- CorrelationMap.reframe's bookkeeping with a stub library ------------------------------------------------------------------
class _ReframeLib(_StubLib):
    def __init__(self):
        _StubLib.__init__(self)
        self.mismatch = 0

    def ym_map_reframe(self, m, h, dx, dy, width, height, hs, poses, n, st):
        self.calls.append(("reframe", dx, dy, width, height, [hs[i] for i in range(n)],
                           [tuple(poses[3 * i + k] for k in range(3)) for i in range(n)]))
        st._obj.mismatch = self.mismatch
        st._obj.kept, st._obj.width, st._obj.height = 5, width, height
        return -1 if self.mismatch else 0


def _reframe_matcher(res=0.05):
    m = _StubScanMatcher()
    m._lib, m._cfg = _ReframeLib(), types.SimpleNamespace(resolution=res)
    return m


def test_reframe_passes_the_held_scans_with_their_stored_poses_and_keeps_the_books():
    m = _reframe_matcher(0.05)
    cm = _bare_map(m, (0.5, 1.5))
    assert cm.window == (0, 0, 4, 4) and cm.anchor == (0.5, 1.5)
    a, b = _Scan(1.0, 2.0, 0.1), _Scan(3.0, 4.0, 0.2)
    ha, hb = m._require_native(a), m._require_native(b)
    cm.add_scans(0.5, 1.5, [a, b])
    a.corrected_pose = _Pose(9.0, 9.0, 0.9)  # moved since: the reframe names the pose of the add
    st = cm.reframe(3, -2)
    assert m._lib.calls[-1] == ("reframe", 3, -2, 4, 4, [ha, hb], [(1.0, 2.0, 0.1), (3.0, 4.0, 0.2)])
    assert st.kept == 5 and cm.revision == 2 and cm.shape == (4, 4) and cm.window == (3, -2, 4, 4)
    assert cm.origin == (0.5 + 3 * 0.05, 1.5 + -2 * 0.05) and cm.anchor == (0.5, 1.5) and len(cm) == 2 and a in cm
    cm.reframe(-1, 0, width=9, height=7)
    assert m._lib.calls[-1][:5] == ("reframe", -1, 0, 9, 7) and cm.shape == (7, 9) and cm.window == (2, -2, 9, 7) and cm.revision == 3
    assert cm.origin == (0.5 + 2 * 0.05, 1.5 + -2 * 0.05)  # from the anchor and the whole offset
    # the map takes scans at its new origin, and at no other
    c = _Scan(5.0, 6.0, 0.3)
    with pytest.raises(ValueError, match="origin"):
        cm.add_scans(0.5, 1.5, [c])
    cm.add_scans(cm.origin[0], cm.origin[1], [c])
    # the identity goes to the library and leaves the revision alone
    rev = cm.revision
    cm.reframe(0, 0)
    cm.reframe(0, 0, 9, 7)
    assert m._lib.calls[-1][:5] == ("reframe", 0, 0, 9, 7) and cm.revision == rev and cm.window == (2, -2, 9, 7)
    # many moves do not drift: 300 scrolls of 7 cells give the origin of one move of 2100
    for _ in range(300):
        cm.reframe(7, 0)
    assert cm.window[:2] == (2102, -2) and cm.origin[0] == 0.5 + 2102 * 0.05
    # counts and bookkeeping that disagree must not pass silently, and the books stay as they were
    m._lib.mismatch = 4
    before = (cm.window, cm.origin, cm.revision, cm.shape, len(cm))
    with pytest.raises(RuntimeError, match="disagree"):
        cm.reframe(1, 1)
    assert (cm.window, cm.origin, cm.revision, cm.shape, len(cm)) == before


def test_reframe_on_a_map_without_counts_and_on_a_map_made_before_the_window_existed():
    from yag_slam_amd.scan_matching import CorrelationMap
    m = _reframe_matcher()
    cm = _bare_map(m, None)
    assert cm.window == (0, 0, 4, 4) and cm.anchor is None
    cm.reframe(2, 1, 6, 5)
    assert m._lib.calls[-1] == ("reframe", 2, 1, 6, 5, [], []) and cm.origin is None and cm.anchor is None
    assert cm.window == (2, 1, 6, 5) and cm.shape == (5, 6) and cm.revision == 1
    old = CorrelationMap.__new__(CorrelationMap)  # only what the constructor of before set
    old.m, old._h, old.shape, old.revision = m, None, (4, 4), 0
    assert old.window == (0, 0, 4, 4) and old.anchor is None
    old.reframe(-1, -1)
    assert old.window == (-1, -1, 4, 4) and old.revision == 1
    old.add_scans(0.0, 0.0, [_Scan(1.0, 2.0, 0.1)])  # (still any origin: the caller keeps it)


def test_empty_correlation_map_window_arguments():
    from yag_slam_amd.scan_matching import ScanMatcher
    m = ScanMatcher.__new__(ScanMatcher)  # (no device: the argument errors come first)
    m._m = None
    with pytest.raises(ValueError, match="only a counted map"):
        m.empty_correlation_map(8, 8, window=(1, 2))
    with pytest.raises(ValueError, match="needs its origin"):
        m.empty_correlation_map(8, 8, counted=True, window=(1, 2))


# ---- MapBuilder's extent policy ------------------------------------------------------------------------------------------------
class _ConfigMatcher(_StubMatcher):
    """_StubMatcher with the three numbers the default margin is made of: range 1.0 + search 0.25 + reach 2 cells of 0.05"""
    config = types.SimpleNamespace(resolution=0.05, smear_deviation=0.05, range_threshold=1.0)


class _WindowStubMap(_CountedStubMap):
    """a counted stub with a window: `reframe` moves it as CorrelationMap does and logs the call"""

    def __init__(self, anchor, window, res=0.05):
        _CountedStubMap.__init__(self)
        self.anchor, self.window, self.res = anchor, window, res
        self.shape = (window[3], window[2])
        self.origin = W.origin(anchor, window, res)

    def add_scans(self, ox, oy, scans):
        assert (ox, oy) == self.origin, ((ox, oy), self.origin)  # bit for bit, as the library asks
        return _CountedStubMap.add_scans(self, ox, oy, scans)

    def reframe(self, dx, dy, width=None, height=None):
        from yag_slam_amd.scan_matching import MapReframeStats
        self.window = W.moved(self.window, dx, dy, width, height)
        self.shape = (self.window[3], self.window[2])
        self.origin = W.origin(self.anchor, self.window, self.res)
        self.log.append(("reframe", dx, dy, self.window[2], self.window[3]))
        self.revision += 1
        return MapReframeStats(0, 0, 0, 0, 0, *self.window)


def _walk_east(n, x0=2.0, y=2.0, pace=0.25):
    return [_KeyScan((x0 + pace * i, y, 0.0)) for i in range(n)]


def test_map_builder_fixed_never_reframes_and_is_the_default():
    from yag_slam_amd.mapping import MapBuilder
    cmap = _WindowStubMap((0.0, 0.0), (0, 0, 80, 80))
    b = MapBuilder(_ConfigMatcher(), cmap, 0.0, 0.0)
    assert b.extent == "fixed"
    b.process_scans(_walk_east(40))  # far out of the map
    assert [e[0] for e in cmap.log] == ["add"] * 40 and b.reframes == [] and (b.ox, b.oy) == (0.0, 0.0)
    for bad in ("follow", None, 1):
        with pytest.raises(ValueError, match="extent"):
            MapBuilder(_ConfigMatcher(), cmap, 0.0, 0.0, extent=bad)
    for bad in (0, -8, 2.5, True):
        with pytest.raises(ValueError, match="step"):
            MapBuilder(_ConfigMatcher(), cmap, 0.0, 0.0, extent="scroll", step=bad)
    with pytest.raises(ValueError, match="margin"):
        MapBuilder(_ConfigMatcher(), cmap, 0.0, 0.0, extent="grow", margin=0.0)


def test_map_builder_scroll_reframes_at_the_margin_by_multiples_of_the_step_and_keeps_the_size():
    from yag_slam_amd.mapping import MapBuilder
    res, anchor = 0.05, (0.013, -0.021)
    cmap = _WindowStubMap(anchor, (0, 0, 80, 80), res)  # 4 m x 4 m; the robot starts at its centre
    b = MapBuilder(_ConfigMatcher(), cmap, anchor[0], anchor[1], extent="scroll", step=8, window=3)
    assert b.margin == 1.0 + 0.25 + 2 * 0.05
    scans = _walk_east(60)
    for s in scans:
        before = (cmap.window, len(cmap.log))
        b.process_scan(s)
        new = [e for e in cmap.log[before[1]:] if e[0] == "reframe"]
        p = s.corrected_pose
        near = min(p.x - W.origin(anchor, before[0], res)[0], W.origin(anchor, before[0], res)[0] + 80 * res - p.x) < b.margin
        assert len(new) == (1 if near else 0), (p.x, before[0])
        # the reframe comes before the add of the same step
        kinds = [e[0] for e in cmap.log[before[1]:]]
        assert kinds in (["add"], ["update"], ["reframe", "add"], ["reframe", "update"])
        # after the step the pose is at least a margin from every side again
        assert p.x - b.ox >= b.margin and b.ox + 80 * res - p.x >= b.margin
    moves = [e for e in cmap.log if e[0] == "reframe"]
    assert len(moves) >= 3 and len(moves) == len(b.reframes)
    assert all(e[1] % 8 == 0 and e[2] % 8 == 0 and e[1] > 0 and e[3:] == (80, 80) for e in moves)
    assert cmap.window[0] == sum(e[1] for e in moves) and cmap.window[1] == sum(e[2] for e in moves) == 0
    # the origin comes from the first origin and the whole offset, bit for bit what the map itself computes
    assert (b.ox, b.oy) == cmap.origin == (anchor[0] + cmap.window[0] * res, anchor[1] + cmap.window[1] * res)
    # the window of keyframes worked as before
    assert len(b.added) == 3 and b.dropped == scans[:57]


def test_map_builder_grow_enlarges_to_the_union_and_a_started_window_keeps_the_maps_origin():
    from yag_slam_amd.mapping import MapBuilder
    res, anchor = 0.05, (0.013, -0.021)
    cmap = _WindowStubMap(anchor, (-16, 24, 80, 80), res)  # a map restored with a window offset
    ox, oy = cmap.origin
    b = MapBuilder(_ConfigMatcher(), cmap, ox, oy, extent="grow", step=16, margin=1.0)
    scans = [_KeyScan((ox + 2.0, oy + 2.0, 0.0))] + [_KeyScan((ox + 2.0 - 0.3 * i, oy + 2.0 + 0.3 * i, 0.0)) for i in range(1, 12)]
    b.process_scans(scans)
    moves = [e for e in cmap.log if e[0] == "reframe"]
    assert len(moves) >= 2
    x0, y0, w, h = -16, 24, 80, 80
    for _, dx, dy, nw, nh in moves:
        assert dx % 16 == 0 and dy % 16 == 0 and nw % 16 == 0 and nh % 16 == 0
        assert dx <= 0 and dy == 0 and nw >= w and nh >= h and (nw, nh) != (w, h)  # west and north only: the union with the old extent
        assert x0 + dx + nw == x0 + w and y0 + dy == y0  # the east and south sides stay
        x0, y0, w, h = x0 + dx, y0 + dy, nw, nh
    assert cmap.window == (x0, y0, w, h) and (b.ox, b.oy) == cmap.origin
    p = scans[-1].corrected_pose
    assert p.x - b.ox >= 1.0 and b.oy + h * res - p.y >= 1.0
    # a map that keeps no counts: the builder moves the origin the caller gave
    plain = _PlainWindowStub(80, 80)
    u = MapBuilder(_ConfigMatcher(), plain, 0.5, 0.25, extent="scroll", step=4, margin=1.0)
    u.process_scans(_walk_east(30, x0=2.5, y=2.25))
    total = sum(e[1] for e in plain.log if e[0] == "reframe")
    assert total > 0 and total % 4 == 0 and (u.ox, u.oy) == (0.5 + total * 0.05, 0.25 + 0 * 0.05)


class _PlainWindowStub(_PlainStubMap):
    def __init__(self, w, h):
        _PlainStubMap.__init__(self)
        self.shape = (h, w)

    def reframe(self, dx, dy, width=None, height=None):
        self.shape = (self.shape[0] if height is None else height, self.shape[1] if width is None else width)
        self.log.append(("reframe", dx, dy) + self.shape[::-1])
        self.revision += 1


# ---- the window's integer arithmetic under the sanitizers, as a program of its own
def test_map_window_arithmetic_under_the_sanitizers(tmp_path):
    cxx = shutil.which("c++") or shutil.which("g++") or shutil.which("clang++")
    assert cxx, "no C++ compiler"
    exe = str(tmp_path / "map_window_check")
    cmd = [cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-Wall", "-Wextra", "-Werror",
           "-I", os.path.join(REPO, "yag_slam_amd", "csrc"), "-o", exe, os.path.join(REPO, "tests", "native", "map_window_check.cpp")]
    # the sanitizers' runtimes inside the program (gcc's spelling, then clang's): it runs whatever else the process environment loads
    for static in (["-static-libasan", "-static-libubsan"], ["-static-libsan"]):
        built = subprocess.run(cmd + static, capture_output=True, text=True)
        if built.returncode == 0:
            break
    assert built.returncode == 0, built.stderr[-2000:]
    run = subprocess.run([exe], capture_output=True, text=True)
    assert run.returncode == 0, (run.stdout[-2000:], run.stderr[-2000:])
    words = run.stdout.split()
    assert words[0] == "ok" and int(words[1]) > 100000
