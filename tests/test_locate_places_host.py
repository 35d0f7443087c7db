"""The places search without a device (include/yagmatch.h ym_locator_locate_places): the new export and
its structs against the header, the restated branch and bound with exclusion against the greedy rule on the exhaustive
volume on the cases tests/test_gpu_locate_places.py runs, the finding that motivates the call, and the bookkeeping of a
MapLocalizer that follows alternatives, on a scripted matcher."""
import ctypes as C
import math
import os
import re
import shutil
import subprocess
from collections import namedtuple

import numpy as np
import pytest

from tests import locate_places_ref as P
from tests import locate_ref as R
from tests.util import REPO

STRUCTS = {"ym_locate_places_opts": "YmLocatePlacesOpts", "ym_locate_places_stats": "YmLocatePlacesStats"}


def test_places_export_and_struct_layouts_match_the_header(tmp_path):
    from yag_slam_amd import _capi
    L = _capi.lib()
    hdr = open(os.path.join(REPO, "include", "yagmatch.h")).read()
    code = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    assert re.search(r"\bym_locator_locate_places\s*\(", code)
    assert "ym_locator_locate_places" in _capi.EXPORTS and hasattr(L, "ym_locator_locate_places")
    assert L.ym_locator_locate_places.argtypes is not None and len(L.ym_locator_locate_places.argtypes) == 12
    assert C.sizeof(_capi.YmLocatePlacesOpts) == 2 * 4 + 8 + 8 + 2 * 4
    assert C.sizeof(_capi.YmLocatePlacesStats) == 2 * 4 + 5 * 8 + 16 * 8
    assert _capi.YmLocatePlacesOpts.sep_cells2.offset == 16 and _capi.YmLocatePlacesStats.round_nodes.offset == 48
    cc = shutil.which("cc") or shutil.which("gcc") or shutil.which("clang")
    assert cc, "no C compiler to read the header with"
    lines = []
    for cname, pyname in STRUCTS.items():
        lines.append('printf("%s %%zu\\n", sizeof(%s));' % (cname, cname))
        for fname, _ in getattr(_capi, pyname)._fields_:
            lines.append('printf("%s.%s %%zu\\n", offsetof(%s, %s));' % (cname, fname, cname, fname))
    src = tmp_path / "layout.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "yagmatch.h"\nint main(void) {\n%s\nreturn 0; }\n' % "\n".join(lines))
    exe = str(tmp_path / "layout")
    subprocess.run([cc, "-I", os.path.join(REPO, "include"), "-o", exe, str(src)], check=True, capture_output=True)
    seen = dict(l.split() for l in subprocess.run([exe], check=True, capture_output=True, text=True).stdout.splitlines())
    for cname, pyname in STRUCTS.items():
        st = getattr(_capi, pyname)
        assert int(seen[cname]) == C.sizeof(st), cname
        for fname, _ in st._fields_:
            assert int(seen["%s.%s" % (cname, fname)]) == getattr(st, fname).offset, (cname, fname)


# ---- the cases of tests/test_gpu_locate_places.py on the yardstick alone --------------------------------------------------
class _Scan(object):
    pass


def _room_scan():
    from yag_slam_amd import synth
    from yag_slam_amd.transform import Transform
    q = _Scan()
    q.ranges = synth.Scene().scan_ranges(R.ROOM_TRUTH, index=950)
    q.min_angle, q.angle_increment, q.range_threshold = synth.MIN_ANGLE, synth.ANGLE_INCREMENT, synth.RANGE_THRESHOLD
    q.corrected_pose = Transform(0.0, 0.0, 0.0, 0.0)
    return q


@pytest.fixture(scope="module")
def room():
    from yag_slam_amd import synth
    g8 = R.byte_grid(R.smear_grid(R.room_image(synth.Scene()), R.ROOM_RES, R.ROOM_RES))
    offs = R.offsets(R.set_points([_room_scan()], 6), R.dir_table(R.ROOM_ANGLES), R.ROOM_RES)
    return g8, offs, R.score_volume(g8, offs)


def test_the_best_64_hide_the_places_that_the_whole_volume_holds(room):
    """the finding the call answers, on the room with (100, 3, circular): the volume holds 8 places, and from the fifth on
    they score below the 64th best hypothesis -- thinning the best 64 cannot see them, whatever top_k says"""
    g8, offs, S = room
    got = P.places(S, 8, 100, 3, 1)
    sixty_fourth = R.top_k(S, 64)[-1][0]
    print("places", got, "64th best", sixty_fourth)
    assert len(got) == 8 and got[0] == R.top_k(S, 1)[0]
    assert [s for s, _ in got] == sorted((s for s, _ in got), reverse=True)
    assert got[4][0] < sixty_fourth
    thinned = P.greedy_over_top(S, 64, 8, 100, 3, 1)
    assert len(thinned) < 8 and thinned == got[:len(thinned)]
    H, W = g8.shape
    for i, (_, a) in enumerate(got):  # no place is near an earlier one
        for _, b in got[:i]:
            k, cx, cy = R.decode(a, W, H)
            assert not P.near_mask(S.shape, R.decode(b, W, H), 100, 3, 1)[k, cy, cx]


def test_places_with_zero_separations_is_top_k(room):
    g8, offs, S = room
    assert P.places(S, 16, 0, 0, 1) == R.top_k(S, 16) == P.places(S, 16, 0, 0, 0)
    assert P.places(S, 1, 100, 3, 1) == R.top_k(S, 1)
    distinct = np.unique(S)[::-1]
    assert P.places(S, 16, 0, 0, 1, s_min=int(distinct[2])) == R.top_k(S, 16, int(distinct[2]))
    assert P.places(S, 4, 100, 3, 1, s_min=int(distinct[0]) + 1) == []
    H, W = g8.shape
    assert len(P.places(S, 8, W * W + H * H, 18, 1)) == 1  # every hypothesis is near the first pick
    assert len(P.places(S, 8, W * W + H * H, 18, 0)) > 1   # ... but not when the headings do not wrap


CASES = [("room", None, 8, 100, 3), ("random", 0, 5, 9, 1), ("random", 2, 5, 9, 1), ("random", 5, 5, 9, 1), ("zero", None, 6, 25, 2),
         ("corners", None, 4, 4, 0), ("odd", 4, 5, 49, 2)]


@pytest.mark.parametrize("name, levels, K, sep_cells2, sep_headings", CASES)
def test_restated_branch_and_bound_with_exclusion_equals_the_greedy_rule(room, name, levels, K, sep_cells2, sep_headings):
    offs = room[1][::3]  # (a third of the headings: the plain-Python search is slow, the GPU tests run all 36)
    g = {"room": None, "random": R.random_grid(), "zero": np.zeros((29, 37)), "corners": R.corner_grid(), "odd": R.random_grid(97, 83, 9) ** 4}[name]
    g8 = room[0] if name == "room" else R.byte_grid(g)
    S = R.score_volume(g8, offs)
    for circular in (1, 0):
        want = P.places(S, K, sep_cells2, sep_headings, circular)
        got, stats = P.branch_and_bound(g8, offs, K, sep_cells2, sep_headings, circular, levels=levels,
                                        max_nodes=1 << 12 if name == "zero" else 1 << 25)
        print(name, levels, "circular", circular, got, stats)
        assert got == want
        assert stats["rounds"] == len(got) + (1 if len(got) < K else 0) == len(stats["round_nodes"])
        assert sum(stats["round_nodes"]) == stats["nodes"] + stats["probe_nodes"]
        if len(got) > 1 and sep_cells2 > 0:
            assert stats["excluded_leaves"] + stats["excluded_nodes"] > 0
    if name == "zero":
        # every score ties: index and exclusion alone decide.  Six picks of radius 5 all fit into row 0 of heading 0, so the two
        # lists agree; that a pick at k = 0 reaches the last headings on a circle only shows in what the search excluded ...
        assert want == [(0, 6 * i) for i in range(6)]
        mask = [np.zeros(S.shape, dtype=bool), np.zeros(S.shape, dtype=bool)]
        n_near = [0, 0]
        for _, index in want[:-1]:
            for c in (0, 1):
                mask[c] |= P.near_mask(S.shape, R.decode(index, 37, 29), sep_cells2, sep_headings, c)
                n_near[c] += int(mask[c].sum())  # every later round meets them again
        assert n_near[1] > n_near[0]
        for c in (0, 1):
            _, stats = P.branch_and_bound(g8, offs, K, sep_cells2, sep_headings, c, levels=0, max_nodes=1 << 12)
            assert stats["excluded_leaves"] == n_near[c] and stats["excluded_nodes"] == 0
        # ... and in the lists once a pick covers its whole heading: 0, 5, 10 in a row, 0, 5 on a circle of 12
        far = 37 * 37 + 29 * 29
        for c, ks in ((0, [0, 5, 10]), (1, [0, 5])):
            got, _ = P.branch_and_bound(g8, offs, 8, far, 4, c, max_nodes=1 << 12)
            assert got == P.places(S, 8, far, 4, c) == [(0, k * 29 * 37) for k in ks]


# ---- MapLocalizer's bookkeeping on a scripted matcher --------------------------------------------------------------------
Res = namedtuple("Res", ["response", "best_pose", "meta"])


def _scan(x=0.0, y=0.0, t=0.0):
    from yag_slam_amd.models import LocalizedRangeScan
    return LocalizedRangeScan(np.full(8, 2.0), -1.0, 1.0, 2.0 / 7, 0.1, 10.0, 8.0, x, y, t)


class _Stub(object):
    """locate_in_map returns the scripted places; track_in_map serves step after step of a script
    {place: (response, accepted, pose)} and records how it was called"""

    def __init__(self, places, script):
        self.places, self.script, self.step, self.calls, self.loc = places, script, 0, [], None

    def locate_in_map(self, cmap, ox, oy, scans, places=None, min_separation=None, **kw):
        from yag_slam_amd.transform import Transform
        self.calls.append(("locate", places, min_separation, kw))
        polished = [Res(r, [Transform(x, y, 0.0, t)], {}) for (r, (x, y, t)) in self.places]
        best = max(range(len(polished)), key=lambda i: (polished[i].response, -i))
        return Res(polished[best].response, polished[best].best_pose, {"places": polished})

    def track_in_map(self, cmap, ox, oy, tracks, start, penalty, do_fine, coarse, min_response):
        from yag_slam_amd.transform import Transform
        if not isinstance(tracks[0], (list, tuple)):  # the single-track step
            self.calls.append(("single", tracks))
            tracks[1].corrected_pose = Transform(7.0, 7.0, 0.0, 0.7)
            return [None, Res(0.77, None, {"accepted": True})], 2
        alts = self.loc.alternatives
        assert len(tracks) == len(alts) and all(len(t) == 2 and t[0] is a.last for t, a in zip(tracks, alts))
        assert all(t[1] is not u[1] for i, t in enumerate(tracks) for u in tracks[:i])  # a copy of the scan each
        self.calls.append(("many", [a.place for a in alts]))
        out = []
        for t, a in zip(tracks, alts):
            r, accepted, (x, y, th) = self.script[self.step][a.place]
            t[1].corrected_pose = Transform(x, y, 0.0, th)
            out.append(([None, Res(r, None, {"accepted": accepted})], 2))
        self.step += 1
        return out


def _state(loc):
    return [(a.place, round(a.evidence, 9), a.lost) for a in loc.alternatives]


def test_localizer_follows_alternatives_by_the_five_step_rule():
    from yag_slam_amd.mapping import MapLocalizer
    A, B, C_, D = (1.0, 1.0, 0.0), (5.0, 5.0, 3.0), (1.1, 1.0, 0.05), (9.0, 9.0, 1.0)
    script = [
        {0: (0.5, True, A), 1: (0.5, True, B), 2: (0.3, True, C_), 3: (0.4, True, D)},   # tie 0/1: the lower place leads; 2 merges into 0
        {0: (0.2, True, A), 1: (0.6, True, B), 3: (0.4, True, D)},                       # the leader changes to 1
        {0: (0.0, False, A), 1: (0.7, True, B), 3: (0.1, True, D)},                      # 0 trails by 1.1 >= 1.0: dropped; 3 by 0.9: stays
        {1: (0.05, False, B), 3: (0.3, True, D)},
        {1: (0.0, False, B), 3: (0.1, False, D)},                                        # the leader's lost reaches max_lost: never dropped
        {1: (0.9, True, B), 3: (0.0, False, D)},                                         # 3's lost reaches max_lost: dropped -- collapse
    ]
    stub = _Stub([(0.6, A), (0.8, B), (0.5, C_), (0.4, D)], script)
    loc = MapLocalizer(stub, "map", -1.0, -2.0, evidence_gap=1.0, max_lost=2, merge=(0.2, 0.1))
    stub.loc = loc
    first = _scan()
    res = loc.start(first, places=4, min_separation=(2.0, 0.3), n_angles=36)
    assert stub.calls[0] == ("locate", 4, (2.0, 0.3), {"n_angles": 36}) and res.response == 0.8
    assert loc.ambiguous and _state(loc) == [(0, 0.0, 0), (1, 0.0, 0), (2, 0.0, 0), (3, 0.0, 0)]
    assert loc.leader.place == 0  # (all evidence 0: the lower place)
    p = first.corrected_pose
    assert (p.x, p.y, p.euler[-1]) == B and loc.last is first  # the best polished place's pose
    for a, want in zip(loc.alternatives, (A, B, C_, D)):
        q = a.last.corrected_pose
        assert a.last is not first and (q.x, q.y) == want[:2] and abs(q.euler[-1] - want[2]) < 1e-12 and a.results == []
    with pytest.raises(ValueError, match="one scan at a time"):
        loc.process_scans([_scan(), _scan()])
    want_states = [
        ([(0, 0.5, 0), (1, 0.5, 0), (3, 0.4, 0)], 0, A),
        ([(0, 0.7, 0), (1, 1.1, 0), (3, 0.8, 0)], 1, B),
        ([(1, 1.8, 0), (3, 0.9, 0)], 1, B),
        ([(1, 1.85, 1), (3, 1.2, 0)], 1, B),
        ([(1, 1.85, 2), (3, 1.3, 1)], 1, B),
        ([(1, 2.75, 0)], 1, B),
    ]
    for i, (state, lead, pose) in enumerate(want_states):
        s = _scan(0.1 * i, 0.0, 0.0)
        r = loc.process_scan(s)
        assert _state(loc) == state, i
        assert loc.leader.place == lead and loc.ambiguous == (len(state) > 1)
        q = s.corrected_pose
        assert (q.x, q.y) == pose[:2] and abs(q.euler[-1] - pose[2]) < 1e-12 and loc.last is s
        assert r.response == script[i][lead][0] and loc.lost == loc.leader.lost
        assert loc.results == loc.leader.results and loc.results[-1] is r
    assert [c[1] for c in stub.calls if c[0] == "many"] == [[0, 1, 2, 3], [0, 1, 3], [0, 1, 3], [1, 3], [1, 3], [1, 3]]
    # collapsed: the next step is the single-track call on the caller's own scans
    before = loc.last
    s = _scan(1.0, 0.0, 0.0)
    r = loc.process_scan(s)
    assert stub.calls[-1][0] == "single" and stub.calls[-1][1][0] is before and stub.calls[-1][1][1] is s
    assert r.response == 0.77 and loc.last is s and not loc.ambiguous and len(loc.alternatives) == 1


def test_localizer_drops_by_evidence_and_lost_before_it_merges():
    """an alternative that is dropped shields nothing: 1 (more evidence, not applied, max_lost 1) goes first, so 2, which stands
    within the merge distance of 1, stays"""
    from yag_slam_amd.mapping import MapLocalizer
    A, B, C_ = (1.0, 1.0, 0.0), (5.0, 5.0, 3.0), (5.1, 5.0, 3.05 - 2 * math.pi)
    stub = _Stub([(0.9, A), (0.8, B), (0.7, C_)], [{0: (0.9, True, A), 1: (0.5, False, B), 2: (0.4, True, C_)},
                                                    {0: (0.1, True, A), 2: (0.1, True, (1.0, 1.15, 0.05))}])
    loc = MapLocalizer(stub, "map", 0.0, 0.0, evidence_gap=10.0, max_lost=1, merge=(0.2, 0.1))
    stub.loc = loc
    loc.start(_scan(), places=3)
    loc.process_scan(_scan())
    assert _state(loc) == [(0, 0.9, 0), (2, 0.4, 0)] and loc.ambiguous
    loc.process_scan(_scan())  # 2 has come within the merge distance of 0, which has more evidence
    assert _state(loc) == [(0, 1.0, 0)] and not loc.ambiguous


def test_localizer_started_without_places_keeps_no_alternative():
    from yag_slam_amd.mapping import MapLocalizer
    stub = _Stub([(0.9, (1.0, 1.0, 0.0))], [])
    loc = MapLocalizer(stub, "map", 0.0, 0.0)
    first = _scan(2.0, 3.0, 0.1)
    assert loc.start(first) is None and loc.alternatives == [] and not loc.ambiguous and loc.leader is None
    assert (loc.evidence_gap, loc.max_lost, loc.merge) == (0.5, 3, (0.2, 0.1))
    loc.process_scan(_scan())
    assert stub.calls == [("single", stub.calls[0][1])] and stub.calls[0][1][0] is first
    loc.start(first, places=1, n_angles=36)  # one place: the plain locate, no alternative
    assert stub.calls[-1] == ("locate", None, None, {"n_angles": 36}) and loc.alternatives == []
