"""The map locator without a device (include/yagmatch.h ym_locator_*): the ABI's layout and exports, the
pyramid bound, the yardstick's own branch and bound against its exhaustive evaluation on the cases tests/test_gpu_locate.py
runs, the min_separation filter, and the scene conditions the GPU tests rely on."""
import ctypes as C
import math
import os
import re
import shutil
import subprocess
from collections import namedtuple

import numpy as np
import pytest

from tests import locate_ref as R
from tests.util import REPO

FUNCS = ("ym_locator_create", "ym_locator_get_info", "ym_locator_read_level", "ym_locator_locate", "ym_locator_destroy")
STRUCTS = {"ym_locator_info": "YmLocatorInfo", "ym_locate_opts": "YmLocateOpts", "ym_locate_candidate": "YmLocateCandidate",
           "ym_locate_stats": "YmLocateStats"}


def test_locator_exports_and_struct_layouts_match_the_header(tmp_path):
    from yag_slam_amd import _capi
    L = _capi.lib()
    hdr = open(os.path.join(REPO, "include", "yagmatch.h")).read()
    code = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    for f in FUNCS:
        assert re.search(r"\b%s\s*\(" % f, code), f
        assert f in _capi.EXPORTS and hasattr(L, f), f
    assert C.sizeof(_capi.YmLocatorInfo) == 4 * 4 + 2 * 8
    assert C.sizeof(_capi.YmLocateOpts) == 2 * 4 + 8
    assert C.sizeof(_capi.YmLocateCandidate) == 4 * 4 + 8 + 8 + 3 * 8
    assert C.sizeof(_capi.YmLocateStats) == 2 * 4 + 9 * 8 + 9 * 8 + 8
    assert _capi.YmLocateCandidate.index.offset == 16 and _capi.YmLocateCandidate.pose.offset == 32
    assert _capi.YmLocateStats.nodes.offset == 8 and _capi.YmLocateStats.survivors.offset == 80
    # the same from the header itself, through a C compiler: size of every struct and offset of every field
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


@pytest.mark.parametrize("seed", [0, 1, 2])
def test_every_pyramid_bound_covers_the_scores_below_it(seed):
    """B of a node >= the largest S of the map cells it covers, for nodes anywhere: aligned or not, overhanging the low edges
    (negative X, Y down to -(2^j - 1)) and the high ones; offsets that leave the map on every side"""
    rng = np.random.default_rng(seed)
    H, W = 23, 19
    g8 = rng.integers(0, 101, size=(H, W)) * (rng.random((H, W)) < 0.3)
    offs = rng.integers(-15, 16, size=(1, 40, 2))
    offs[0, :4] = [[-40, 0], [0, 40], [30, -30], [0, 0]]
    S = R.score_volume(g8, offs)[0]
    for j in range(0, 5):
        side, m = 1 << j, (1 << j) - 1
        lvl = R.pyramid_level(g8, j)
        assert lvl.shape == (H + m, W + m)
        xs, ys = np.meshgrid(np.arange(-m, W), np.arange(-m, H))
        B = R.node_bounds(lvl, j, offs[0], xs.reshape(-1), ys.reshape(-1)).reshape(xs.shape)
        for (y, x), b in np.ndenumerate(B):
            Y, X = y - m, x - m
            below = S[max(0, Y):Y + side, max(0, X):X + side]
            assert below.size and b >= below.max(), (j, X, Y, b, below.max())
        if j == 0:
            assert np.array_equal(B, S)
        # level j from level j - 1 by four reads at offsets 0 and 2^(j - 1), as the device builds it
        if j > 0:
            h, prev = side // 2, R.pyramid_level(g8, j - 1)
            pm = h - 1
            big = np.zeros((H + m + h + side, W + m + h + side), dtype=np.int64)
            big[m - pm:m - pm + prev.shape[0], m - pm:m - pm + prev.shape[1]] = prev  # prev's cell (x, y) at [y + m][x + m]
            four = np.maximum(np.maximum(big[:H + m, :W + m], big[:H + m, h:h + W + m]),
                              np.maximum(big[h:h + H + m, :W + m], big[h:h + H + m, h:h + W + m]))
            assert np.array_equal(four, lvl)


Cand = namedtuple("Cand", ["name", "pose"])


def test_min_separation_filter_on_a_hand_made_list():
    from yag_slam_amd.scan_matching import filter_min_separation
    from yag_slam_amd.transform import Transform
    c = [Cand("a", Transform(1.0, 1.0, 0.0, 0.10)),
         Cand("b", Transform(1.1, 1.0, 0.0, 0.15)),                 # near a in both: dropped
         Cand("c", Transform(1.1, 1.0, 0.0, 1.50)),                 # near a in metres only: kept
         Cand("d", Transform(4.0, 1.0, 0.0, 0.10)),                 # near a in radians only: kept
         Cand("e", Transform(4.1, 1.1, 0.0, 0.10 - 2 * math.pi)),   # near d, the heading a full turn away: dropped
         Cand("f", Transform(1.2, 1.0, 0.0, 0.20)),                 # near a (kept) -- b, nearer still, was dropped and shields nothing
         Cand("g", Transform(1.45, 1.0, 0.0, 0.10))]                # within 0.3 of f and b, which are gone; 0.45 from a: kept
    assert [k.name for k in filter_min_separation(c, 0.3, 0.2)] == ["a", "c", "d", "g"]
    assert [k.name for k in filter_min_separation(c, 0.0, 0.0)] == list("abcdefg")
    assert filter_min_separation([], 1.0, 1.0) == []


# ---- the cases of tests/test_gpu_locate.py on the yardstick alone -----------------------------------------------------------
class _Scan(object):
    pass


def _room_scan(pose=(0.0, 0.0, 0.0), truth=R.ROOM_TRUTH, index=950):
    from yag_slam_amd import synth
    from yag_slam_amd.transform import Transform
    q = _Scan()
    q.ranges = synth.Scene().scan_ranges(truth, index=index)
    q.min_angle, q.angle_increment, q.range_threshold = synth.MIN_ANGLE, synth.ANGLE_INCREMENT, synth.RANGE_THRESHOLD
    q.corrected_pose = Transform(pose[0], pose[1], 0.0, pose[2])
    return q


@pytest.fixture(scope="module")
def room():
    from yag_slam_amd import synth
    g8 = R.byte_grid(R.smear_grid(R.room_image(synth.Scene()), R.ROOM_RES, R.ROOM_RES))
    offs = R.offsets(R.set_points([_room_scan()], 6), R.dir_table(R.ROOM_ANGLES), R.ROOM_RES)
    S = R.score_volume(g8, offs)
    return g8, offs, S


def test_the_room_scene_is_what_the_gpu_tests_need(room):
    """asserted on the yardstick first: the exhaustive best lies within one cell and half a heading step of the true pose, and
    the branch and bound scores fewer than half the exhaustive node count"""
    g8, offs, S = room
    H, W = g8.shape
    assert (H, W) == R.ROOM_SHAPE and offs.shape[:2] == (R.ROOM_ANGLES, 181)
    score, index = R.top_k(S, 1)[0]
    k, cx, cy = R.decode(index, W, H)
    step = 2 * math.pi / R.ROOM_ANGLES
    assert abs(R.ROOM_ORIGIN[0] + cx * R.ROOM_RES - R.ROOM_TRUTH[0]) <= R.ROOM_RES + 1e-9
    assert abs(R.ROOM_ORIGIN[1] + cy * R.ROOM_RES - R.ROOM_TRUTH[1]) <= R.ROOM_RES + 1e-9
    assert abs(k * step - R.ROOM_TRUTH[2]) <= step / 2
    best, stats = R.branch_and_bound(g8, offs, 16)
    assert best == R.top_k(S, 16)
    assert sum(stats["nodes"]) + stats["probe_nodes"] < 0.5 * S.size, (stats, S.size)
    assert stats["chunks"] == 1


@pytest.mark.parametrize("levels", [0, 1, 3, 4, 6])
def test_yardstick_branch_and_bound_is_exhaustive_on_the_room_at_every_depth(room, levels):
    g8, offs, S = room
    best, _ = R.branch_and_bound(g8, offs, 16, levels=levels)
    assert best == R.top_k(S, 16)


def test_yardstick_branch_and_bound_in_many_chunks_and_with_a_floor(room):
    g8, offs, S = room
    one, _ = R.branch_and_bound(g8, offs, 16)
    many, stats = R.branch_and_bound(g8, offs, 16, max_nodes=256 * 100)
    assert stats["chunks"] >= 8 and many == one == R.top_k(S, 16)
    distinct = np.unique(S)[::-1]
    s_min = R.s_min_of((distinct[2] + distinct[3]) / 2.0 / (100.0 * offs.shape[1]), offs.shape[1])
    assert distinct[3] < s_min <= distinct[2]
    got, _ = R.branch_and_bound(g8, offs, 64, s_min=s_min)
    assert got == R.top_k(S, 64, s_min) and 3 <= len(got) < 64 and all(s >= distinct[2] for s, _ in got)
    assert R.branch_and_bound(g8, offs, 16, s_min=int(distinct[0]) + 1)[0] == []


@pytest.mark.parametrize("name, levels", [("random", 0), ("random", 2), ("random", 5), ("zero", None), ("corners", None), ("odd", 4)])
def test_yardstick_branch_and_bound_equals_its_exhaustive_top_k(room, name, levels):
    offs = room[1][::3]  # (a third of the headings: the plain-Python search is slow, the GPU tests run all 36)
    g = {"random": R.random_grid(), "zero": np.zeros((29, 37)), "corners": R.corner_grid(), "odd": R.random_grid(97, 83, 9) ** 4}[name]
    g8 = R.byte_grid(g)
    S = R.score_volume(g8, offs)
    best, stats = R.branch_and_bound(g8, offs, 16, levels=levels, max_nodes=1 << 12 if name == "zero" else 1 << 25)
    assert best == R.top_k(S, 16)
    if name == "zero":
        assert best == [(0, i) for i in range(16)] and stats["survivors"] == stats["nodes"] and stats["chunks"] > 1
