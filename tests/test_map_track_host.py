"""Localization mode without a device (include/yagmatch.h ym_match_map_many / ym_map_track / ym_debug_map_sums, DESIGN.md section
13): the ABI against the header read through a C compiler, the Python entries' validation, MapLocalizer's prior and pose
bookkeeping against a stub matcher, and the polish_top selection and tie rule."""
import ctypes as C
import os
import re
import shutil
import subprocess

import pytest

from tests.util import REPO

FUNCS = ("ym_match_map_many", "ym_map_track", "ym_debug_map_sums")

# what yag_slam_amd/_capi.py declares, spelled as C prototypes: assigning the header's functions to these pointers compiles
# without a diagnostic only when the header declares exactly these parameter lists
PROTOS = """
int (*p_many)(ym_matcher *, const ym_map *, double, double, const ym_scan *const *, const int32_t *, int, int, int,
              const ym_map_search *, ym_result *) = ym_match_map_many;
int (*p_track)(ym_matcher *, const ym_map *, double, double, ym_scan *const *, const double *, const int32_t *, int, int, int, int,
               const ym_map_search *, double, ym_result *, int32_t *) = ym_map_track;
int (*p_sums)(ym_matcher *, int, int, uint32_t *, int64_t) = ym_debug_map_sums;
"""


def test_exports_argtypes_and_result_layout_match_the_header(tmp_path):
    from yag_slam_amd import _capi
    L = _capi.lib()
    hdr = open(os.path.join(REPO, "include", "yagmatch.h")).read()
    code = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    for f in FUNCS:
        assert re.search(r"\b%s\s*\(" % f, code), f
        assert f in _capi.EXPORTS and hasattr(L, f), f
    vp, ip, dp = C.c_void_p, C.POINTER(C.c_int32), C.POINTER(C.c_double)
    ms, rs = C.POINTER(_capi.YmMapSearch), C.POINTER(_capi.YmResult)
    assert list(L.ym_match_map_many.argtypes) == [vp, vp, C.c_double, C.c_double, C.POINTER(vp), ip, C.c_int, C.c_int, C.c_int, ms, rs]
    assert list(L.ym_map_track.argtypes) == [vp, vp, C.c_double, C.c_double, C.POINTER(vp), dp, ip, C.c_int, C.c_int, C.c_int, C.c_int,
                                             ms, C.c_double, rs, ip]
    assert list(L.ym_debug_map_sums.argtypes) == [vp, C.c_int, C.c_int, C.POINTER(C.c_uint32), C.c_int64]
    # the header itself, through a C compiler: the prototypes, and the layout of ym_result whose last field ym_map_track uses
    cc = shutil.which("cc") or shutil.which("gcc") or shutil.which("clang")
    assert cc, "no C compiler to read the header with"
    lines = ['printf("ym_result %zu\\n", sizeof(ym_result));']
    for fname, _ in _capi.YmResult._fields_:
        lines.append('printf("%s %%zu\\n", offsetof(ym_result, %s));' % (fname, fname))
    src = tmp_path / "layout.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "yagmatch.h"\n%s\nint main(void) {\n%s\nreturn 0; }\n'
                   % (PROTOS, "\n".join(lines)))
    obj = str(tmp_path / "layout.o")
    subprocess.run([cc, "-Wall", "-Werror", "-I", os.path.join(REPO, "include"), "-c", "-o", obj, str(src)], check=True, capture_output=True)
    exe = str(tmp_path / "layout")
    stub = tmp_path / "stubs.c"  # (the three entries are only named, never called: the program links against empty stand-ins)
    stub.write_text("int ym_match_map_many(void) { return 0; }\nint ym_map_track(void) { return 0; }\nint ym_debug_map_sums(void) { return 0; }\n")
    subprocess.run([cc, "-o", exe, obj, str(stub)], check=True, capture_output=True)
    seen = dict(l.split() for l in subprocess.run([exe], check=True, capture_output=True, text=True).stdout.splitlines())
    assert int(seen["ym_result"]) == C.sizeof(_capi.YmResult)
    for fname, _ in _capi.YmResult._fields_:
        assert int(seen[fname]) == getattr(_capi.YmResult, fname).offset, fname
    assert _capi.YmResult.reserved.offset == C.sizeof(_capi.YmResult) - 4
    # the option that forces the chunk length and the two counters are documented where the tests look them up
    assert re.search(r"^\s*\*\s+47\s", hdr, flags=re.M) and "[6] items of ym_match_map_many" in hdr


class _NoLibrary(object):
    """a ScanMatcher whose library must not be touched"""

    def __getattr__(self, name):
        raise AssertionError("the library was touched: %s" % name)


def _bare_matcher():
    from yag_slam_amd.scan_matching import ScanMatcher
    m = ScanMatcher.__new__(ScanMatcher)
    m._lib, m._m, m.device = _NoLibrary(), None, 0
    return m


def test_batch_and_track_entries_refuse_empty_input_before_the_library():
    m = _bare_matcher()
    cmap = object()
    with pytest.raises(ValueError, match="no query set"):
        m.match_map_batch(cmap, 0.0, 0.0, [])
    with pytest.raises(ValueError, match="set 1 is empty"):
        m.match_map_batch(cmap, 0.0, 0.0, [[object()], []])
    with pytest.raises(ValueError, match="no track"):
        m.track_in_map(cmap, 0.0, 0.0, [])
    with pytest.raises(ValueError, match="track 1 is empty"):
        m.track_in_map(cmap, 0.0, 0.0, [[object()], []])
    with pytest.raises(ValueError, match="start"):
        m.track_in_map(cmap, 0.0, 0.0, [object(), object()], start=0)
    with pytest.raises(TypeError, match="CorrelationMap"):
        m.match_map_batch(cmap, 0.0, 0.0, [[object()]])
    m._m = None


class _Scan(object):
    def __init__(self, odom):
        from yag_slam_amd.transform import Transform
        self.odom_pose = Transform(odom[0], odom[1], 0.0, odom[2])
        self.corrected_pose = Transform(odom[0], odom[1], 0.0, odom[2])


class _StubMatcher(object):
    """track_in_map as the library defines it, on the host: the 'match' moves every prior by a fixed correction and answers
    with the response the test queued for it"""

    def __init__(self, responses, correction=(0.01, -0.02, 0.003)):
        self.responses, self.correction, self.calls, self.priors = list(responses), correction, [], []

    def track_in_map(self, cmap, ox, oy, tracks, start, penalty, do_fine, coarse, min_response):
        from yag_slam_amd.scan_matching import ScanMatcherResult
        from yag_slam_amd.transform import Transform
        self.calls.append((cmap, ox, oy, len(tracks), start, penalty, do_fine, coarse, min_response))
        res = [None] * len(tracks)
        for i in range(start, len(tracks)):
            prior = tracks[i - 1].corrected_pose + (tracks[i].odom_pose - tracks[i - 1].odom_pose)
            self.priors.append(prior)
            resp = self.responses.pop(0)
            if resp is None:  # the matcher cannot serve this scan: it keeps its prior, the track ends
                tracks[i].corrected_pose = prior
                return res, i
            ok = not resp < min_response
            c = self.correction
            centre = Transform(prior.x + c[0], prior.y + c[1], 0.0, c[2])
            tracks[i].corrected_pose = Transform(centre.x, centre.y, 0.0, prior.euler[-1] + c[2]) if ok else prior
            res[i] = ScanMatcherResult(resp, None, centre, {"accepted": ok})
        return res, len(tracks)

    def locate_in_map(self, cmap, ox, oy, scans, **kw):
        from yag_slam_amd.scan_matching import ScanMatcherResult
        from yag_slam_amd.transform import Transform
        self.calls.append(("locate", kw))
        return ScanMatcherResult(0.9, None, [Transform(4.0, 3.0, 0.0, 0.5)], {})


def _tf(p):
    return (p.x, p.y, p.euler[-1])


def test_map_localizer_keeps_priors_poses_and_the_lost_count():
    from yag_slam_amd.mapping import MapLocalizer
    from yag_slam_amd.transform import Transform
    scans = [_Scan((1.0 + 0.1 * i, 2.0 - 0.05 * i, 0.1 * i)) for i in range(6)]
    stub = _StubMatcher([0.9, 0.2, 0.1, 0.8, 0.7])
    loc = MapLocalizer(stub, "the map", -1.0, -2.0, coarse={"xy_step": 0.02}, min_response=0.3)
    assert loc.process_scan(scans[0]) is None and loc.last is scans[0] and stub.calls == []
    want_pose = scans[0].corrected_pose
    lost = []
    for i in range(1, 4):
        odom_diff = scans[i].odom_pose - scans[i - 1].odom_pose
        prior = want_pose + odom_diff
        r = loc.process_scan(scans[i])
        assert _tf(stub.priors[-1]) == _tf(prior)
        want_pose = Transform(prior.x + 0.01, prior.y - 0.02, 0.0, prior.euler[-1] + 0.003) if r.meta["accepted"] else prior
        assert _tf(scans[i].corrected_pose) == _tf(want_pose) and loc.last is scans[i]
        lost.append(loc.lost)
    assert lost == [0, 1, 2] and [r.meta["accepted"] for r in loc.results] == [True, False, False]
    assert stub.calls[0] == ("the map", -1.0, -2.0, 2, 1, True, True, {"xy_step": 0.02}, 0.3)
    # several scans in one call: one library call, the same bookkeeping
    got = loc.process_scans(scans[4:])
    assert len(got) == 2 and len(stub.calls) == 4 and stub.calls[-1][3] == 3
    assert loc.lost == 0 and loc.last is scans[5] and len(loc.results) == 5
    assert not hasattr(loc, "scans") and not hasattr(loc, "constraints")  # no graph, no vertex
    # a scan the matcher cannot serve keeps its prior; the track goes on from it
    more = [_Scan((2.0, 2.0, 0.6)), _Scan((2.1, 2.0, 0.6))]
    stub.responses = [None]
    with pytest.raises(ValueError, match="could not be matched"):
        loc.process_scans(more)
    assert loc.last is more[0] and _tf(more[0].corrected_pose) == _tf(stub.priors[-1]) and len(loc.results) == 5
    # a scan without a pose: located first, both poses set
    lost_scan = _Scan((0.0, 0.0, 0.0))
    res = loc.start(lost_scan, n_angles=36)
    assert stub.calls[-1] == ("locate", {"n_angles": 36}) and res.response == 0.9
    assert _tf(lost_scan.corrected_pose) == _tf(lost_scan.odom_pose) == (4.0, 3.0, 0.5) and loc.last is lost_scan and loc.lost == 0


def test_polish_top_takes_the_best_response_and_the_earlier_of_equals():
    from yag_slam_amd.scan_matching import ScanMatcherResult, _pick_polished
    from yag_slam_amd.transform import Transform

    def polished(resp, x):
        rigid = [Transform(x, 0.0, 0.0, 0.0)]
        return ScanMatcherResult(resp, [[resp]], [Transform(-x, 0.0, 0.0, 0.0)], {"rigid_poses": rigid, "centre": (x, 0.0, 0.0)})

    r = _pick_polished([polished(0.5, 1.0), polished(0.8, 2.0), polished(0.8, 3.0), polished(0.7, 4.0)], {"candidates": "kept"})
    assert r.response == 0.8 and r.meta["polished_index"] == 1 and r.best_pose[0].x == 2.0 and r.covariance == [[0.8]]
    assert r.meta["candidates"] == "kept" and r.meta["centre"] == (2.0, 0.0, 0.0) and r.meta["wrapper_poses"][0].x == -2.0
    assert [p.response for p in r.meta["polished"]] == [0.5, 0.8, 0.8, 0.7]
    assert [p.best_pose[0].x for p in r.meta["polished"]] == [1.0, 2.0, 3.0, 4.0]
    assert _pick_polished([polished(0.3, 1.0), polished(0.3, 2.0)], {}).meta["polished_index"] == 0
