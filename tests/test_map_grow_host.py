"""Maps that take scans, without a device (include/yagmatch.h ym_map_create_empty / ym_map_add_scans / ym_map_clear, DESIGN.md
section 15): the ABI against the header read through a C compiler, the refusals that need no device, MapBuilder's policy with a
stub matcher and a stub map, the restatement (tests/mapgrow_ref.py) against the fixture the reference's own add_scan_to_grid
made, and the revision / stale-locator rule with stubs."""
import ctypes as C
import math
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

from tests import mapgrow_ref as R
from tests.util import GOLDEN, REPO

FUNCS = ("ym_map_create_empty", "ym_map_add_scans", "ym_map_clear")

# what yag_slam_amd/_capi.py declares, spelled as C prototypes: assigning the header's functions to these pointers compiles
# without a diagnostic only when the header declares exactly these parameter lists
PROTOS = """
ym_map *(*p_empty)(ym_matcher *, int, int) = ym_map_create_empty;
int (*p_add)(ym_matcher *, ym_map *, double, double, const ym_scan *const *, int, ym_map_add_stats *) = ym_map_add_scans;
int (*p_clear)(ym_matcher *, ym_map *) = ym_map_clear;
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
    assert L.ym_map_create_empty.restype is vp and list(L.ym_map_create_empty.argtypes) == [vp, C.c_int, C.c_int]
    assert list(L.ym_map_add_scans.argtypes) == [vp, vp, C.c_double, C.c_double, C.POINTER(vp), C.c_int, C.POINTER(_capi.YmMapAddStats)]
    assert list(L.ym_map_clear.argtypes) == [vp, vp]
    assert L.ym_version() == 1
    cc = shutil.which("cc") or shutil.which("gcc") or shutil.which("clang")
    assert cc, "no C compiler to read the header with"
    lines = ['printf("ym_map_add_stats %zu\\n", sizeof(ym_map_add_stats));']
    for fname, _ in _capi.YmMapAddStats._fields_:
        lines.append('printf("%s %%zu\\n", offsetof(ym_map_add_stats, %s));' % (fname, fname))
    src = tmp_path / "layout.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "yagmatch.h"\n%s\nint main(void) {\n%s\nreturn 0; }\n'
                   % (PROTOS, "\n".join(lines)))
    obj = str(tmp_path / "layout.o")
    subprocess.run([cc, "-Wall", "-Werror", "-I", os.path.join(REPO, "include"), "-c", "-o", obj, str(src)], check=True, capture_output=True)
    exe = str(tmp_path / "layout")
    stub = tmp_path / "stubs.c"  # (the three entries are only named, never called: the program links against empty stand-ins)
    stub.write_text("".join("int %s(void) { return 0; }\n" % f for f in FUNCS))
    subprocess.run([cc, "-o", exe, obj, str(stub)], check=True, capture_output=True)
    seen = dict(l.split() for l in subprocess.run([exe], check=True, capture_output=True, text=True).stdout.splitlines())
    assert int(seen["ym_map_add_stats"]) == C.sizeof(_capi.YmMapAddStats) == 3 * 8 + 4 * 4
    for fname, _ in _capi.YmMapAddStats._fields_:
        assert int(seen[fname]) == getattr(_capi.YmMapAddStats, fname).offset, fname


def test_null_arguments_are_refused_before_any_device_is_touched():
    from yag_slam_amd import _capi
    L = _capi.lib()
    st = _capi.YmMapAddStats()
    one = (C.c_void_p * 1)()
    fake = C.c_void_p(16)  # never dereferenced: the null argument beside it is found first
    assert L.ym_map_add_scans(None, None, 0.0, 0.0, one, 1, C.byref(st)) == -1 and "null" in _capi.last_error()
    assert L.ym_map_add_scans(fake, None, 0.0, 0.0, one, 1, C.byref(st)) == -1 and "null" in _capi.last_error()
    assert L.ym_map_add_scans(None, fake, 0.0, 0.0, one, 0, None) == -1 and "null" in _capi.last_error()
    assert L.ym_map_clear(None, None) == -1 and "null" in _capi.last_error()
    assert L.ym_map_clear(fake, None) == -1 and L.ym_map_clear(None, fake) == -1
    assert not L.ym_map_create_empty(None, 8, 8) and "null matcher" in _capi.last_error()


# ---- the restatement against the reference's own add_scan_to_grid ------------------------------------------------------------
def test_restatement_equals_the_reference_made_fixture():
    z = np.load(os.path.join(GOLDEN, "map_grow.npz"))
    w, h, res = int(z["width"]), int(z["height"]), float(z["res"])
    assert w <= 130 and h <= 67
    ox, oy = float(z["ox"]), float(z["oy"])
    kernel = R.calculate_kernel(res, float(z["smear"]))
    assert kernel.shape == z["kernel"].shape == (5, 5) and np.abs(kernel - z["kernel"]).max() <= 1e-15
    want = np.zeros((h, w))
    want[z["cgrid_nz_y"], z["cgrid_nz_x"]] = z["cgrid_nz_val"]
    # from the fixture's world points (the reference's own scan model made them) with the fixture's taps: every bit
    g = np.zeros((h, w))
    stamped, dropped, cells = R.add_points(g, z["kernel"], z["points_x"], z["points_y"], ox, oy, res)
    assert (stamped, dropped) == (int(z["stamped"]), int(z["dropped"])) and stamped > 50 and dropped > 50
    assert np.array_equal(g, want)
    gx, gy = R.world_to_grid(z["points_x"], z["points_y"], ox, oy, res)
    assert np.array_equal(gx.astype(np.int32), z["gx"]) and np.array_equal(gy.astype(np.int32), z["gy"])
    assert (z["gy"] < 0).any() and (z["gx"] >= w).any()  # readings beyond two sides, negative cells among them
    inside = [(int(a), int(b)) for a, b in zip(z["gx"], z["gy"]) if 0 <= a < w and 0 <= b < h]
    assert cells == inside
    # from the package's own scans: the same points (its points() against the reference's), the same cells, the same grid
    from yag_slam_amd.models import point_readings
    xs, ys = [], []
    for r, p in zip(z["ranges"], z["poses"]):
        x, y = point_readings(r, p[0], p[1], p[2], float(z["sensor_min_angle"]), float(z["sensor_angle_increment"]),
                              float(z["sensor_range_threshold"]))
        xs.append(x); ys.append(y)
    xs, ys = np.concatenate(xs), np.concatenate(ys)
    assert len(xs) == len(z["points_x"]) and np.abs(xs - z["points_x"]).max() <= 1e-12 and np.abs(ys - z["points_y"]).max() <= 1e-12
    assert R.distance_to_half(xs, ys, ox, oy, res) > R.HALF_GUARD
    g2 = np.zeros((h, w))
    assert R.add_points(g2, z["kernel"], xs, ys, ox, oy, res)[:2] == (stamped, dropped)
    assert np.array_equal(g2, want)
    # the order of the points does not matter
    g3 = np.zeros((h, w))
    R.add_points(g3, z["kernel"], xs[::-1], ys[::-1], ox, oy, res)
    assert np.array_equal(g3, want)
    # quotients that are not finite or do not fit an int32 are dropped
    g4 = np.zeros((4, 4))
    assert R.add_points(g4, z["kernel"], [np.nan, np.inf, 1e300, -1e300, 0.1], [0.1, 0.1, 0.1, 0.1, 0.1], 0.0, 0.0, res)[:2] == (1, 4)


# ---- MapBuilder's policy -----------------------------------------------------------------------------------------------------
class _Scan(object):
    def __init__(self, odom):
        from yag_slam_amd.transform import Transform
        self.odom_pose = Transform(odom[0], odom[1], 0.0, odom[2])
        self.corrected_pose = Transform(odom[0], odom[1], 0.0, odom[2])


class _StubMap(object):
    """records what it is asked to do, with the poses the scans had at that moment"""

    def __init__(self):
        self.log, self.revision = [], 0

    def add_scans(self, ox, oy, scans):
        from yag_slam_amd.scan_matching import MapAddStats
        self.log.append(("add", ox, oy, [(s, _tf(s.corrected_pose)) for s in scans]))
        self.revision += 1
        return MapAddStats(len(scans), len(scans), 0, 0, 0, 1, 1)

    def clear(self):
        self.log.append(("clear",))
        self.revision += 1


class _StubMatcher(object):
    """track_in_map as the library defines it, on the host: the prior is the odometry composition, the 'match' leaves it
    where it is (a zero correction) and answers with the response the test queued; None: the scan cannot be served.
    exact: the 'match' puts an accepted scan at its odometry pose instead -- the composition's roundings aside that is the
    same pose, and the keyframe test can then sit exactly on a threshold"""

    def __init__(self, responses, exact=False):
        self.responses, self.calls, self.map_revisions, self.exact = list(responses), [], [], exact

    def track_in_map(self, cmap, ox, oy, tracks, start, penalty, do_fine, coarse, min_response):
        from yag_slam_amd.scan_matching import ScanMatcherResult
        self.calls.append((cmap, ox, oy, len(tracks), start, penalty, do_fine, coarse, min_response))
        self.map_revisions.append(cmap.revision)
        assert len(tracks) == 2 and start == 1
        prior = tracks[0].corrected_pose + (tracks[1].odom_pose - tracks[0].odom_pose)
        tracks[1].corrected_pose = prior
        resp = self.responses.pop(0)
        if resp is None:
            return [None, None], 1
        ok = not resp < min_response
        if ok and self.exact:
            tracks[1].corrected_pose = tracks[1].odom_pose
        return [None, ScanMatcherResult(resp, None, prior, {"accepted": ok})], 2


def _tf(p):
    return (p.x, p.y, p.euler[-1])


def test_map_builder_keyframe_rule_at_below_and_above_both_thresholds():
    from yag_slam_amd.mapping import MapBuilder
    D, A = 0.25, 0.125  # (both exact in binary, and so are the poses below: "at the threshold" means equal)
    # (dx, dyaw) of each scan against the LAST ADDED scan, and whether the rule adds it: near in both -> not added
    steps = [((0.125, 0.0625), False),    # below both
             ((0.25, 0.0), True),         # distance at its threshold (the node's test is a strict <)
             ((0.0, 0.125), True),        # rotation at its threshold
             ((0.125, -0.125), True),     # rotation at its threshold, the other way round
             ((0.5, 0.0), True),          # distance above
             ((0.0, 0.25), True),         # rotation above
             ((0.2499, 0.1249), False),   # just below both
             ((-0.125, 0.0), False)]      # a step backwards is measured by its length
    stub, cmap = _StubMatcher([0.9] * len(steps), exact=True), _StubMap()
    b = MapBuilder(stub, cmap, -1.0, -2.0, coarse={"xy_step": 0.02}, min_response=0.3, min_distance=D, min_rotation=A)
    first = _Scan((1.0, 2.0, 0.0))
    assert b.process_scan(first) is None
    assert b.last is first and b.last_added is first and b.added == [first] and stub.calls == []
    assert cmap.log == [("add", -1.0, -2.0, [(first, (1.0, 2.0, 0.0))])]
    for (dx, da), want in steps:
        l = b.last_added.corrected_pose
        s = _Scan((l.x + dx, l.y, l.euler[-1] + da))
        n_added = len(b.added)
        r = b.process_scan(s)
        assert r.meta["accepted"] and r.meta["added"] == want, (dx, da)
        assert b.last is s and (b.last_added is s) == want and len(b.added) == n_added + int(want)
        if want:  # added AFTER the match, at the pose the match left
            assert cmap.log[-1] == ("add", -1.0, -2.0, [(s, _tf(s.corrected_pose))])
            assert stub.map_revisions[-1] == cmap.revision - 1
    assert stub.calls[0] == (cmap, -1.0, -2.0, 2, 1, True, True, {"xy_step": 0.02}, 0.3)
    assert len(stub.calls) == len(steps) == len(b.results) and b.lost == 0
    assert [e[0] for e in cmap.log] == ["add"] * (1 + sum(w for _, w in steps))
    # the defaults (0, 0): nothing is "nearer than 0", every accepted scan is added
    stub2, cmap2 = _StubMatcher([0.9, 0.9], exact=True), _StubMap()
    b2 = MapBuilder(stub2, cmap2, 0.0, 0.0)
    b2.start(first)
    assert [r.meta["added"] for r in b2.process_scans([_Scan((1.0, 2.0, 0.0)), _Scan((1.0, 2.0, 0.0))])] == [True, True]


def test_map_builder_never_adds_a_rejected_step_counts_lost_and_rebuilds_once():
    from yag_slam_amd.mapping import MapBuilder
    from yag_slam_amd.transform import Transform
    scans = [_Scan((1.0 + 0.5 * i, 2.0, 0.25 * i)) for i in range(7)]
    stub, cmap = _StubMatcher([0.9, 0.1, 0.2, 0.8, None, 0.7]), _StubMap()
    b = MapBuilder(stub, cmap, 0.5, 0.25, min_response=0.3, min_distance=0.25, min_rotation=0.125)
    stats = b.start(scans[0])
    assert stats.stamped == 1 and b.lost == 0
    lost, added = [], []
    for s in scans[1:4]:
        r = b.process_scan(s)
        lost.append(b.lost); added.append(r.meta["added"])
    # steps 2 and 3 moved half a metre each and were rejected: far beyond both thresholds, and still not added
    assert lost == [0, 1, 2] and added == [True, False, False] and b.added == scans[:2] and b.last is scans[3]
    got = b.process_scans([scans[4]])
    assert len(got) == 1 and got[0].meta["added"] and b.lost == 0 and b.added == [scans[0], scans[1], scans[4]]
    # a scan the matcher cannot serve keeps its prior, is not added, and the track goes on from it
    prior = scans[4].corrected_pose + (scans[5].odom_pose - scans[4].odom_pose)
    with pytest.raises(ValueError, match="could not be matched"):
        b.process_scan(scans[5])
    assert b.last is scans[5] and _tf(scans[5].corrected_pose) == _tf(prior) and len(b.results) == 4 and len(b.added) == 3
    assert b.process_scan(scans[6]).meta["added"] and b.last_added is scans[6] and len(b.results) == 5
    # an optimiser moves the added scans; rebuild clears and passes every one of them once, in one call, at its new pose
    for i, s in enumerate(b.added):
        s.corrected_pose = Transform(10.0 + i, 20.0, 0.0, 0.5)
    before = len(cmap.log)
    b.rebuild()
    assert cmap.log[before:] == [("clear",), ("add", 0.5, 0.25, [(s, (10.0 + i, 20.0, 0.5)) for i, s in enumerate(b.added)])]
    assert [s for s, _ in cmap.log[-1][3]] == [scans[0], scans[1], scans[4], scans[6]]
    assert not hasattr(b, "scans") and not hasattr(b, "constraints")  # no graph, no vertex


# ---- revision and the stale-locator rule -------------------------------------------------------------------------------------
class _StubLib(object):
    """the three library entries CorrelationMap's new calls use; `stamped` is what the next add reports"""

    def __init__(self):
        self.stamped, self.calls = 0, []

    def ym_map_add_scans(self, m, h, ox, oy, hs, n, st):
        self.calls.append(("add", m, h, ox, oy, [hs[i] for i in range(n)], n))
        st._obj.points, st._obj.stamped, st._obj.dropped = 7, self.stamped, 7 - self.stamped
        st._obj.x0, st._obj.y0, st._obj.x1, st._obj.y1 = (1, 2, 3, 4) if self.stamped else (0, 0, 0, 0)
        return 0

    def ym_map_clear(self, m, h):
        self.calls.append(("clear", m, h))
        return 0


class _StubScanMatcher(object):
    def __init__(self):
        self._lib, self._m = _StubLib(), 111

    def _require_native(self, s):
        return s


def _bare_map(matcher):
    from yag_slam_amd.scan_matching import CorrelationMap
    cm = CorrelationMap.__new__(CorrelationMap)
    cm.m, cm._h, cm.shape, cm.revision = matcher, None, (4, 4), 0  # (no handle: nothing to destroy)
    return cm


def test_revision_counts_adds_that_stamped_and_clears_and_a_stale_locator_refuses():
    from yag_slam_amd.scan_matching import MapAddStats, MapLocator
    m = _StubScanMatcher()
    cm = _bare_map(m)
    cm._h = 222
    try:
        assert cm.revision == 0
        assert cm.add_scans(0.5, 1.5, []) == MapAddStats(7, 0, 7, 0, 0, 0, 0) and cm.revision == 0  # nothing stamped
        assert m._lib.calls[-1] == ("add", 111, 222, 0.5, 1.5, [], 0)
        m._lib.stamped = 5
        assert cm.add_scans(0.5, 1.5, [31, 32]) == MapAddStats(7, 5, 2, 1, 2, 3, 4) and cm.revision == 1
        assert m._lib.calls[-1] == ("add", 111, 222, 0.5, 1.5, [31, 32], 2)
        cm.clear()
        assert cm.revision == 2 and m._lib.calls[-1] == ("clear", 111, 222)
        # a locator remembers the revision it was built at (its pyramid is a copy of the map of then)
        loc = MapLocator.__new__(MapLocator)
        loc.m, loc._h, loc._cmap, loc._revision = m, None, cm, cm.revision
        loc._check_revision()
        cm.add_scans(0.0, 0.0, [33])
        with pytest.raises(ValueError, match="make a new locator"):
            loc.locate([object()], 0.0, 0.0)  # (before anything of the query or the library is touched)
        fresh = MapLocator.__new__(MapLocator)
        fresh.m, fresh._h, fresh._cmap, fresh._revision = m, None, cm, cm.revision
        fresh._check_revision()
    finally:
        cm._h = None


def test_half_guard_helper_measures_the_distance_to_a_tie():
    assert R.distance_to_half([0.125], [0.1], 0.0, 0.0, 0.05) < 1e-9            # 2.5 is a tie
    assert math.isclose(R.distance_to_half([0.1], [0.05], 0.0, 0.0, 0.05), 0.5, abs_tol=1e-9)  # 2.0 and 1.0: as far as can be
    assert R.distance_to_half([0.1], [-0.1250001], 0.0, 0.0, 0.05) < 1e-5       # just beside -2.5
    assert R.distance_to_half([], [], 0.0, 0.0, 0.05) == np.inf
