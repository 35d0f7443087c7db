"""Maps that forget, without a device (include/yagmatch.h ym_map_create_counted / ym_map_update_scans / ym_map_counted /
ym_map_read_stamps): the ABI against the header read through a C compiler, the refusals that need no
device, CorrelationMap's bookkeeping of held scans with a stub library, MapBuilder's window policy with stubs, and the numpy
restatement of a removal (decrement, then the map of the counts -- tests/mapforget_ref.py) against tests/mapgrow_ref.py's build of
the scans that remain, on the scans of the fixture the reference made."""
import ctypes as C
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

from tests import mapforget_ref as F
from tests import mapgrow_ref as R
from tests.util import GOLDEN, REPO

FUNCS = ("ym_map_create_counted", "ym_map_update_scans", "ym_map_counted", "ym_map_read_stamps")

# what yag_slam_amd/_capi.py declares, spelled as C prototypes (see tests/test_map_grow_host.py)
PROTOS = """
ym_map *(*p_counted)(ym_matcher *, int, int, double, double) = ym_map_create_counted;
int (*p_update)(ym_matcher *, ym_map *, const ym_scan *const *, const double *, int, const ym_scan *const *, int,
                ym_map_update_stats *) = ym_map_update_scans;
int (*p_is)(const ym_map *) = ym_map_counted;
int (*p_stamps)(const ym_map *, uint32_t *, int64_t) = ym_map_read_stamps;
"""


def test_exports_argtypes_and_stats_layout_match_the_header(tmp_path):
    from yag_slam_amd import _capi
    L = _capi.lib()
    hdr = open(os.path.join(REPO, "include", "yagmatch.h")).read()
    code = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    for f in FUNCS:
        assert re.search(r"\b%s\s*\(" % f, code), f
        assert f in _capi.EXPORTS and hasattr(L, f), f
    vp = C.c_void_p
    assert L.ym_map_create_counted.restype is vp
    assert list(L.ym_map_create_counted.argtypes) == [vp, C.c_int, C.c_int, C.c_double, C.c_double]
    assert list(L.ym_map_update_scans.argtypes) == [vp, vp, C.POINTER(vp), C.POINTER(C.c_double), C.c_int, C.POINTER(vp), C.c_int,
                                                    C.POINTER(_capi.YmMapUpdateStats)]
    assert list(L.ym_map_counted.argtypes) == [vp] and list(L.ym_map_read_stamps.argtypes) == [vp, C.POINTER(C.c_uint32), C.c_int64]
    assert L.ym_version() == 1
    cc = shutil.which("cc") or shutil.which("gcc") or shutil.which("clang")
    assert cc, "no C compiler to read the header with"
    lines = ['printf("ym_map_update_stats %zu\\n", sizeof(ym_map_update_stats));',
             'printf("ym_map_add_stats %zu\\n", sizeof(ym_map_add_stats));']
    for fname, _ in _capi.YmMapUpdateStats._fields_:
        lines.append('printf("%s %%zu\\n", offsetof(ym_map_update_stats, %s));' % (fname, fname))
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
    assert int(seen["ym_map_update_stats"]) == C.sizeof(_capi.YmMapUpdateStats) == 6 * 8 + 4 * 4
    assert int(seen["ym_map_add_stats"]) == 3 * 8 + 4 * 4  # (the existing struct keeps its pinned size)
    for fname, _ in _capi.YmMapUpdateStats._fields_:
        assert int(seen[fname]) == getattr(_capi.YmMapUpdateStats, fname).offset, fname


def test_null_and_negative_arguments_are_refused_before_any_device_is_touched():
    from yag_slam_amd import _capi
    L = _capi.lib()
    st = _capi.YmMapUpdateStats()
    one = (C.c_void_p * 1)()
    poses = (C.c_double * 3)()
    fake = C.c_void_p(16)  # never dereferenced: the argument beside it is refused first
    assert L.ym_map_update_scans(None, None, one, poses, 1, one, 1, C.byref(st)) == -1 and "null" in _capi.last_error()
    assert L.ym_map_update_scans(fake, None, one, poses, 1, one, 1, C.byref(st)) == -1 and "null" in _capi.last_error()
    assert L.ym_map_update_scans(None, fake, one, poses, 1, one, 1, None) == -1 and "null" in _capi.last_error()
    # a list that is said to hold something and is null, the removed scans' poses among them
    assert L.ym_map_update_scans(fake, fake, None, poses, 1, one, 0, None) == -1 and "null" in _capi.last_error()
    assert L.ym_map_update_scans(fake, fake, one, None, 1, one, 0, None) == -1 and "null" in _capi.last_error()
    assert L.ym_map_update_scans(fake, fake, one, poses, 0, None, 1, None) == -1 and "null" in _capi.last_error()
    assert L.ym_map_update_scans(fake, fake, one, poses, -1, one, 0, None) == -1 and "negative" in _capi.last_error()
    assert L.ym_map_update_scans(fake, fake, one, poses, 0, one, -1, None) == -1 and "negative" in _capi.last_error()
    assert not L.ym_map_create_counted(None, 8, 8, 0.0, 0.0) and "null matcher" in _capi.last_error()
    assert L.ym_map_counted(None) == 0
    buf = (C.c_uint32 * 4)()
    assert L.ym_map_read_stamps(None, buf, 4) == -1 and "null" in _capi.last_error()
    assert L.ym_map_read_stamps(fake, None, 4) == -1 and "null" in _capi.last_error()


# ---- the restatement of a removal against the restatement of the scans that remain -------------------------------------------
class _FixtureScan(object):
    """what mapgrow_ref.add_scans needs of a scan: `points()` at the current pose, by the package's own `point_readings`"""

    def __init__(self, z, ranges, pose):
        self.z, self.ranges, self.pose = z, ranges, tuple(float(v) for v in pose)

    def points(self):
        from yag_slam_amd.models import point_readings
        z = self.z
        return point_readings(self.ranges, self.pose[0], self.pose[1], self.pose[2], float(z["sensor_min_angle"]),
                              float(z["sensor_angle_increment"]), float(z["sensor_range_threshold"]))


def test_restated_removal_equals_the_restatement_of_the_scans_that_remain():
    z = np.load(os.path.join(GOLDEN, "map_grow.npz"))
    w, h, res, ox, oy = int(z["width"]), int(z["height"]), float(z["res"]), float(z["ox"]), float(z["oy"])
    kernel = z["kernel"]
    a, b = (_FixtureScan(z, r, p) for r, p in zip(z["ranges"], z["poses"]))
    # a third scan: the first one's readings from a pose a few cells on, so that the three share cells and reach
    c = _FixtureScan(z, z["ranges"][0], (z["poses"][0][0] + 0.131, z["poses"][0][1] - 0.087, z["poses"][0][2] + 0.05))
    for s in (a, b, c):
        assert R.distance_to_half(*s.points(), ox, oy, res) > R.HALF_GUARD  # no quotient within 1e-6 of a rounding tie
    cells = {id(s): F.cells_of([s], (h, w), ox, oy, res) for s in (a, b, c)}
    assert all(len(v) > 20 for v in cells.values())
    both, _ = R.build((h, w), kernel, [a, b], ox, oy, res)
    want = np.zeros((h, w))
    want[z["cgrid_nz_y"], z["cgrid_nz_x"]] = z["cgrid_nz_val"]
    assert np.array_equal(both, want)  # (the fixture's own map: the reference made it)
    counts = F.counts_of((h, w), cells[id(a)] + cells[id(b)] + cells[id(c)])
    assert counts.sum() == sum(len(v) for v in cells.values()) and counts.max() >= 2  # cells shared between readings
    # the map is a function of the counts: gather (from_counts) and scatter (build) meet bit for bit, the table being the same
    assert np.array_equal(F.from_counts(counts, kernel), R.build((h, w), kernel, [a, b, c], ox, oy, res)[0])
    for gone, rest in ((c, [a, b]), (a, [b]), (b, [])):
        before = counts.copy()
        F.remove(counts, cells[id(gone)])
        assert np.array_equal(F.from_counts(counts, kernel), R.build((h, w), kernel, rest, ox, oy, res)[0]), len(rest)
        assert np.array_equal(counts, F.counts_of((h, w), [x for s in rest for x in cells[id(s)]]))
        # what a removal has to recompute: only cells within the taps' reach of a cell whose count fell to zero differ
        released = (before > 0) & (counts == 0)
        changed = F.from_counts(before, kernel) != F.from_counts(counts, kernel)
        half = kernel.shape[0] // 2
        reach = np.zeros((h, w), dtype=bool)
        for y, x in np.argwhere(released):
            reach[max(0, y - half):y + half + 1, max(0, x - half):x + half + 1] = True
        assert released.any() and not (changed & ~reach).any()
    assert not counts.any()
    with pytest.raises(AssertionError):
        F.remove(counts, cells[id(a)])  # a count below zero is the caller's error


# ---- CorrelationMap's bookkeeping with a stub library ------------------------------------------------------------------------
class _Pose(object):
    def __init__(self, x, y, th):
        self.x, self.y, self.euler = x, y, (0.0, 0.0, th)


class _Scan(object):
    def __init__(self, x, y, th):
        self.corrected_pose = _Pose(x, y, th)


class _StubLib(object):
    """the library entries a counted CorrelationMap uses; records every call with the poses it was given"""

    def __init__(self):
        self.calls, self.unmatched, self.removed, self.added = [], 0, None, None

    def ym_map_add_scans(self, m, h, ox, oy, hs, n, st):
        self.calls.append(("add", ox, oy, [hs[i] for i in range(n)]))
        st._obj.points, st._obj.stamped, st._obj.dropped = 3 * n, 2 * n, n
        return 0

    def ym_map_update_scans(self, m, h, rs, poses, n_remove, ads, n_add, st):
        self.calls.append(("update", [rs[i] for i in range(n_remove)], [tuple(poses[3 * i + k] for k in range(3)) for i in range(n_remove)],
                           [ads[i] for i in range(n_add)]))
        st._obj.removed = 2 * n_remove if self.removed is None else self.removed
        st._obj.added = 2 * n_add if self.added is None else self.added
        st._obj.unmatched = self.unmatched
        return 0

    def ym_map_clear(self, m, h):
        self.calls.append(("clear",))
        return 0


class _StubScanMatcher(object):
    def __init__(self):
        self._lib, self._m, self.handles = _StubLib(), 111, {}

    def _require_native(self, s):
        return self.handles.setdefault(id(s), 1000 + len(self.handles))


def _bare_map(matcher, origin):
    from yag_slam_amd.scan_matching import CorrelationMap
    cm = CorrelationMap.__new__(CorrelationMap)
    cm.m, cm._h, cm.shape, cm.revision = matcher, None, (4, 4), 0  # (no handle: nothing to destroy)
    cm.counted, cm.origin, cm._held = origin is not None, origin, {}
    return cm


def test_a_counted_map_remembers_the_pose_of_the_add_and_refuses_before_the_library():
    m = _StubScanMatcher()
    cm = _bare_map(m, (0.5, 1.5))
    a, b, c = _Scan(1.0, 2.0, 0.1), _Scan(3.0, 4.0, 0.2), _Scan(5.0, 6.0, 0.3)
    ha, hb, hc = (m._require_native(s) for s in (a, b, c))
    with pytest.raises(ValueError, match="origin"):
        cm.add_scans(0.5, 1.25, [a])
    with pytest.raises(ValueError, match="twice"):
        cm.add_scans(0.5, 1.5, [a, a])
    assert m._lib.calls == [] and len(cm) == 0 and a not in cm and cm.revision == 0
    cm.add_scans(0.5, 1.5, [a, b])
    assert m._lib.calls == [("add", 0.5, 1.5, [ha, hb])] and len(cm) == 2 and a in cm and b in cm and c not in cm and cm.revision == 1
    with pytest.raises(ValueError, match="already held"):
        cm.add_scans(0.5, 1.5, [c, a])
    with pytest.raises(ValueError, match="not held"):
        cm.remove_scans([a, c])
    with pytest.raises(ValueError, match="twice"):
        cm.remove_scans([a, a])
    with pytest.raises(ValueError, match="twice"):
        cm.sync([a, a])
    assert len(m._lib.calls) == 1 and len(cm) == 2 and cm.revision == 1  # refused before the library, nothing changed
    # nothing moved: no call, no revision
    assert cm.sync().removed == 0 and cm.moved_scans() == [] and len(m._lib.calls) == 1 and cm.revision == 1
    # a moves: the removal names the pose of the add, not the current one
    a.corrected_pose = _Pose(1.25, 2.0, 0.1)
    assert cm.moved_scans() == [a] and cm.moved_scans([b, c]) == []
    assert cm.sync([b, c]).removed == 0 and len(m._lib.calls) == 1  # (a is not in the list; c is not held and is passed over)
    st = cm.sync()
    assert m._lib.calls[-1] == ("update", [ha], [(1.0, 2.0, 0.1)], [ha]) and (st.removed, st.added) == (2, 2) and cm.revision == 2
    assert cm.moved_scans() == [] and len(cm) == 2
    a.corrected_pose = _Pose(9.0, 9.0, 0.9)  # moved again, then removed: out at the pose of the last add
    cm.remove_scans([a])
    assert m._lib.calls[-1] == ("update", [ha], [(1.25, 2.0, 0.1)], []) and a not in cm and len(cm) == 1 and cm.revision == 3
    # one call that takes b out and puts a and c in
    cm.update_scans([b], [a, c])
    assert m._lib.calls[-1] == ("update", [hb], [(3.0, 4.0, 0.2)], [ha, hc]) and [s in cm for s in (a, b, c)] == [True, False, True]
    with pytest.raises(ValueError, match="already held"):
        cm.update_scans([a], [c])
    cm.update_scans([a], [a])  # in both lists: a move
    assert m._lib.calls[-1] == ("update", [ha], [(9.0, 9.0, 0.9)], [ha]) and cm.revision == 5
    # a call that changed no reading leaves the revision alone
    m._lib.removed = m._lib.added = 0
    cm.remove_scans([c])
    assert cm.revision == 5 and c not in cm
    m._lib.removed = m._lib.added = None
    # counts and bookkeeping that disagree must not pass silently
    m._lib.unmatched = 3
    with pytest.raises(RuntimeError, match="count of zero"):
        cm.remove_scans([a])
    m._lib.unmatched = 0
    # clear forgets the held scans too
    cm.add_scans(0.5, 1.5, [b])
    cm.clear()
    assert len(cm) == 0 and b not in cm and m._lib.calls[-1] == ("clear",)
    cm.add_scans(0.5, 1.5, [b])  # (not "already held")
    assert bool(cm) and len(cm) == 1


def test_an_uncounted_map_refuses_what_forgets_and_adds_as_before():
    m = _StubScanMatcher()
    cm = _bare_map(m, None)
    a = _Scan(1.0, 2.0, 0.1)
    for call in (lambda: cm.remove_scans([a]), lambda: cm.sync(), lambda: cm.sync([a]), lambda: cm.stamps(), lambda: len(cm),
                 lambda: a in cm, lambda: cm.update_scans([], [a]), lambda: cm.moved_scans()):
        with pytest.raises(ValueError, match="keeps no counts"):
            call()
    assert m._lib.calls == [] and bool(cm)
    cm.add_scans(7.0, 8.0, [a])
    cm.add_scans(-7.0, 8.5, [a, a])  # any origin, any scan again: exactly today's add_scans
    assert [c[:3] for c in m._lib.calls] == [("add", 7.0, 8.0), ("add", -7.0, 8.5)] and cm.revision == 2
    # a map made before the attributes existed (only what the old constructor set) still adds and clears
    from yag_slam_amd.scan_matching import CorrelationMap
    old = CorrelationMap.__new__(CorrelationMap)
    old.m, old._h, old.shape, old.revision = m, None, (4, 4), 0
    old.add_scans(0.0, 0.0, [a])
    old.clear()
    assert old.revision == 2
    with pytest.raises(ValueError, match="keeps no counts"):
        old.remove_scans([a])


def test_empty_correlation_map_arguments():
    from yag_slam_amd.scan_matching import ScanMatcher
    m = ScanMatcher.__new__(ScanMatcher)  # (no device: the argument errors come first)
    m._m = None
    with pytest.raises(ValueError, match="needs its origin"):
        m.empty_correlation_map(8, 8, counted=True)
    with pytest.raises(ValueError, match="needs its origin"):
        m.empty_correlation_map(8, 8, counted=True, ox=1.0)
    with pytest.raises(ValueError, match="only a counted map"):
        m.empty_correlation_map(8, 8, ox=1.0, oy=2.0)


# ---- MapBuilder's window policy ----------------------------------------------------------------------------------------------
class _KeyScan(object):
    def __init__(self, odom):
        from yag_slam_amd.transform import Transform
        self.odom_pose = Transform(odom[0], odom[1], 0.0, odom[2])
        self.corrected_pose = Transform(odom[0], odom[1], 0.0, odom[2])


def _tf(p):
    return (p.x, p.y, p.euler[-1])


class _PlainStubMap(object):
    """a map of before: add_scans, clear and a revision, nothing else"""

    def __init__(self):
        self.log, self.revision = [], 0

    def add_scans(self, ox, oy, scans):
        from yag_slam_amd.scan_matching import MapAddStats
        self.log.append(("add", [(s, _tf(s.corrected_pose)) for s in scans]))
        self.revision += 1
        return MapAddStats(len(scans), len(scans), 0, 0, 0, 1, 1)

    def clear(self):
        self.log.append(("clear",))
        self.revision += 1


class _CountedStubMap(_PlainStubMap):
    """what MapBuilder may use of a counted map, with CorrelationMap's bookkeeping: held scans and the poses of their adds"""
    counted = True

    def __init__(self):
        _PlainStubMap.__init__(self)
        self.held = {}

    def add_scans(self, ox, oy, scans):
        assert not any(id(s) in self.held for s in scans)
        for s in scans:
            self.held[id(s)] = (s, _tf(s.corrected_pose))
        return _PlainStubMap.add_scans(self, ox, oy, scans)

    def clear(self):
        self.held = {}
        _PlainStubMap.clear(self)

    def moved_scans(self, scans=None):
        scans = [e[0] for e in self.held.values()] if scans is None else scans
        return [s for s in scans if id(s) in self.held and self.held[id(s)][1] != _tf(s.corrected_pose)]

    def update_scans(self, remove, add):
        from yag_slam_amd.scan_matching import MapUpdateStats
        assert all(id(s) in self.held for s in remove)
        self.log.append(("update", [(s, self.held[id(s)][1]) for s in remove], [(s, _tf(s.corrected_pose)) for s in add]))
        for s in remove:
            del self.held[id(s)]
        for s in add:
            self.held[id(s)] = (s, _tf(s.corrected_pose))
        self.revision += 1
        return MapUpdateStats(len(remove), len(add), 0, 0, len(remove), len(add), 0, 0, 1, 1)

    def sync(self, scans=None):
        moved = self.moved_scans(scans)
        return self.update_scans(moved, moved)


class _StubMatcher(object):
    """track_in_map on the host: the prior is the odometry composition and every step is accepted at it"""

    def track_in_map(self, cmap, ox, oy, tracks, start, penalty, do_fine, coarse, min_response):
        from yag_slam_amd.scan_matching import ScanMatcherResult
        prior = tracks[0].corrected_pose + (tracks[1].odom_pose - tracks[0].odom_pose)
        tracks[1].corrected_pose = prior
        return [None, ScanMatcherResult(0.9, None, prior, {"accepted": True})], 2


def test_map_builder_window_at_n_and_n_plus_one():
    from yag_slam_amd.mapping import MapBuilder
    N = 3
    scans = [_KeyScan((1.0 + 0.5 * i, 2.0, 0.0)) for i in range(6)]
    cmap = _CountedStubMap()
    b = MapBuilder(_StubMatcher(), cmap, 0.5, 0.25, window=N)
    b.process_scans(scans[:N])
    # at N: every keyframe went in by a plain add, nothing was dropped
    assert b.added == scans[:N] and b.dropped == [] and [e[0] for e in cmap.log] == ["add"] * N and b.window == N
    # the (N + 1)th takes the oldest out in the same call, at the pose it was added at
    first_pose = _tf(scans[0].corrected_pose)
    r = b.process_scan(scans[N])
    assert r.meta["added"] and b.added == scans[1:N + 1] and b.dropped == [scans[0]] and b.last_added is scans[N]
    assert cmap.log[-1] == ("update", [(scans[0], first_pose)], [(scans[N], _tf(scans[N].corrected_pose))]) and len(cmap.log) == N + 1
    b.process_scans(scans[N + 1:])
    assert b.added == scans[3:] and b.dropped == scans[:3] and len(b.added) == N
    assert [e[0] for e in cmap.log] == ["add"] * N + ["update"] * 3 and sorted(cmap.held) == sorted(id(s) for s in scans[3:])
    # window=1: the map holds the last keyframe alone
    cmap1 = _CountedStubMap()
    b1 = MapBuilder(_StubMatcher(), cmap1, 0.0, 0.0, window=1)
    b1.process_scans(scans[:3])
    assert b1.added == [scans[2]] and b1.dropped == scans[:2]


def test_map_builder_window_needs_a_counted_map_and_a_plain_map_still_works_unwindowed():
    from yag_slam_amd.mapping import MapBuilder
    from yag_slam_amd.transform import Transform
    with pytest.raises(ValueError, match="can forget"):
        MapBuilder(_StubMatcher(), _PlainStubMap(), 0.0, 0.0, window=4)
    for bad in (0, -1, 2.5, True):
        with pytest.raises(ValueError, match="window"):
            MapBuilder(_StubMatcher(), _CountedStubMap(), 0.0, 0.0, window=bad)
    scans = [_KeyScan((1.0 + 0.5 * i, 2.0, 0.0)) for i in range(5)]
    plain = _PlainStubMap()
    b = MapBuilder(_StubMatcher(), plain, 0.0, 0.0)
    b.process_scans(scans)
    assert b.added == scans and b.dropped == [] and b.window is None and [e[0] for e in plain.log] == ["add"] * 5
    # rebuild on a map that keeps no counts: exactly clear and add, whatever moved
    scans[1].corrected_pose = Transform(7.0, 7.0, 0.0, 0.5)
    b.rebuild()
    assert [e[0] for e in plain.log[5:]] == ["clear", "add"] and [s for s, _ in plain.log[-1][1]] == scans


def test_map_builder_rebuild_routes_by_counted_and_by_the_share_that_moved():
    from yag_slam_amd.mapping import MapBuilder
    from yag_slam_amd.transform import Transform
    scans = [_KeyScan((1.0 + 0.5 * i, 2.0, 0.0)) for i in range(8)]
    cmap = _CountedStubMap()
    b = MapBuilder(_StubMatcher(), cmap, 0.0, 0.0)  # a counted map without a window: nothing is dropped
    b.process_scans(scans)
    assert b.added == scans and b.dropped == [] and len(cmap.log) == 8
    old = _tf(scans[2].corrected_pose)
    scans[2].corrected_pose = Transform(7.0, 7.0, 0.0, 0.5)
    b.rebuild()  # one of eight moved: only that one is touched
    assert cmap.log[8:] == [("update", [(scans[2], old)], [(scans[2], (7.0, 7.0, 0.5))])]
    b.rebuild()  # nothing moved: an update of nothing
    assert cmap.log[9:] == [("update", [], [])]
    n_share = int(MapBuilder.REBUILD_SHARE * len(scans))
    assert 0 < n_share < len(scans)
    for s in scans[:n_share]:  # exactly the share: still moved one by one
        s.corrected_pose = Transform(s.corrected_pose.x, 9.0, 0.0, 0.0)
    b.rebuild()
    assert cmap.log[-1][0] == "update" and len(cmap.log[-1][1]) == n_share
    for s in scans[:n_share + 1]:  # above it: clear and add everything, at the current poses
        s.corrected_pose = Transform(s.corrected_pose.x, 11.0, 0.0, 0.0)
    b.rebuild()
    assert [e[0] for e in cmap.log[-2:]] == ["clear", "add"] and [s for s, _ in cmap.log[-1][1]] == scans
    assert cmap.moved_scans() == []
