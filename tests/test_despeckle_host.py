"""The component area filter without a device (include/yagmatch.h ym_image_despeckle / ym_occupancy_create_clean, DESIGN.md
section 12): the restatement tests/despeckle_ref.py against arrays written out by hand and against a literal transcription
of the node's loop (slam_node_ros1:191-197, scipy's labels in cv2's place), ros_codes against the node's three assignment
lines, the ABI's layout, the argument checks that run before any device work, and the conditions the fixtures of
tests/test_gpu_despeckle.py must meet for its comparisons to mean something."""
import ctypes as C
import os
import re
import shutil
import subprocess

import numpy as np
import pytest
from scipy import ndimage

from tests import despeckle_ref as D
from tests import occupancy_ref
from tests.util import REPO

FUNCS = ("ym_image_despeckle", "ym_occupancy_create_clean", "ym_occupancy_get_despeckle_stats")
STRUCTS = {"ym_despeckle_opts": "YmDespeckleOpts", "ym_despeckle_stats": "YmDespeckleStats"}

def _img(rows):
    """'#' = foreground (0), '.' = free (255), '?' = unknown (200)"""
    return np.array([[{"#": 0, ".": 255, "?": 200}[c] for c in r] for r in rows], dtype=np.uint8)


# a diagonal chain of 4 (rows 0 - 3) and an L of 5 (rows 5 - 7) in one image
BOTH = _img(["#.......",
             ".#......",
             "..#.....",
             "...#....",
             "........",
             ".....#..",
             ".....#..",
             ".....###"])
BOTH_8 = _img(["........",
               "........",
               "........",
               "........",
               "........",
               ".....#..",
               ".....#..",
               ".....###"])


def test_restatement_on_a_chain_and_an_l_written_out_by_hand():
    out, st = D.despeckle(BOTH, connectivity=8)
    assert np.array_equal(out, BOTH_8)
    assert st == {"foreground_cells": 9, "components": 2, "removed_components": 1, "cleared_cells": 4, "background_cells": 55,
                  "background_filled": 0}
    # under 4 the chain is 4 singletons: removed all the same at area 5, and one by one at area 2, which keeps the L
    out, st = D.despeckle(BOTH, connectivity=4)
    assert np.array_equal(out, BOTH_8)
    assert (st["components"], st["removed_components"], st["cleared_cells"]) == (5, 4, 4)
    out8, st8 = D.despeckle(BOTH, min_area=2, connectivity=8)
    out4, st4 = D.despeckle(BOTH, min_area=2, connectivity=4)
    assert np.array_equal(out8, BOTH) and st8["removed_components"] == 0
    assert np.array_equal(out4, BOTH_8) and (st4["components"], st4["removed_components"]) == (5, 4)
    # the chain survives at area 4 under 8 only
    assert np.array_equal(D.despeckle(BOTH, min_area=4, connectivity=8)[0], BOTH)
    assert np.array_equal(D.despeckle(BOTH, min_area=4, connectivity=4)[0], BOTH_8)


def test_restatement_background_rule_on_three_by_three():
    im = _img(["###", "#.#", "##?"])
    out, st = D.despeckle(im)
    assert np.array_equal(out, _img(["###", "#.#", "##."]))  # B = 2 < 5: both become 255, the 200 too
    assert st == {"foreground_cells": 7, "components": 1, "removed_components": 0, "cleared_cells": 0, "background_cells": 2,
                  "background_filled": 1}
    out, st = D.despeckle(im, fill=9)
    assert out[1, 1] == 9 and out[2, 2] == 9 and (out == 0).sum() == 7
    out, st = D.despeckle(im, min_area=2)
    assert np.array_equal(out, im) and st["background_filled"] == 0  # B = 2 is not < 2
    full = np.zeros((3, 3), np.uint8)
    out, st = D.despeckle(full)
    assert np.array_equal(out, full)
    assert st == {"foreground_cells": 9, "components": 1, "removed_components": 0, "cleared_cells": 0, "background_cells": 0,
                  "background_filled": 0}


@pytest.mark.parametrize("min_area", [0, 1])
@pytest.mark.parametrize("connectivity", [4, 8])
def test_restatement_min_area_0_and_1_are_the_identity(min_area, connectivity):
    for im in (BOTH, _img(["###", "#.#", "##?"]), np.zeros((2, 2), np.uint8), np.full((2, 2), 200, np.uint8)):
        out, st = D.despeckle(im, min_area=min_area, connectivity=connectivity)
        assert np.array_equal(out, im) and st["removed_components"] == 0 and st["cleared_cells"] == 0 and st["background_filled"] == 0


def _node_loop(im):
    """slam_node_ros1:191-197 line for line; cv2.connectedComponentsWithStats (8-connected, label 0 = the background, the
    last column of its statistics = the area) stood in for by scipy's labels, which number the same way: 0 = background"""
    im = im.copy()
    static_only = 255 - im.copy()
    static_only[static_only < 200] = 0
    mask, num = ndimage.label(static_only != 0, structure=np.ones((3, 3)))
    stats = [[int((mask == ii).sum())] for ii in range(num + 1)]
    for ii, stat in enumerate(stats):
        if stat[-1] < 5:
            im[mask == ii] = 255
    return im


def _random_image(seed):
    """0 / 200 / 255 at five densities of 0; the last five seeds are small and nearly full, the background rule's ground"""
    r = np.random.RandomState(1000 + seed)
    density = (0.02, 0.1, 0.3, 0.45, 0.6)[seed % 5]
    h, w = (r.randint(3, 40), r.randint(3, 40)) if seed < 15 else (r.randint(3, 8), r.randint(3, 8))
    im = np.where(r.rand(h, w) < density, 0, r.choice([200, 255], size=(h, w))).astype(np.uint8)
    if seed >= 15:
        im[r.rand(h, w) < 0.9] = 0
    return im


@pytest.mark.parametrize("seed", range(20))
def test_restatement_is_the_nodes_loop(seed):
    im = _random_image(seed)
    # the node's threshold: 255 - im >= 200 means im <= 55; on a rendered grid (0 / 200 / 255) that is im == 0
    assert set(np.unique(im)) <= {0, 200, 255}
    out, st = D.despeckle(im)
    assert np.array_equal(out, _node_loop(im)), seed
    assert st["foreground_cells"] == int((im == 0).sum())


def test_the_nodes_loop_cases_reach_every_rule():
    stats = [D.despeckle(_random_image(seed))[1] for seed in range(20)]
    assert sum(st["background_filled"] for st in stats) >= 2
    assert sum(st["removed_components"] > 0 for st in stats) >= 10
    assert sum(st["components"] > st["removed_components"] for st in stats) >= 10


def test_ros_codes_are_the_nodes_three_lines():
    from yag_slam_amd.occupancy import ros_codes
    r = np.random.RandomState(3)
    im = r.choice(np.array([0, 200, 255], np.uint8), size=(17, 23))
    got = ros_codes(im)
    assert got.dtype == np.int8 and got.shape == im.shape
    assert np.array_equal(got, D.ros_codes(im))
    assert set(np.unique(got)) == {-1, 0, 100}
    assert np.array_equal(ros_codes(im[::2, 1::3]), D.ros_codes(im[::2, 1::3]))
    for bad in (1, 100, 199, 201, 254):
        im2 = im.copy()
        im2[5, 7] = bad
        with pytest.raises(ValueError, match="rendered grid"):
            ros_codes(im2)
    with pytest.raises(ValueError):
        ros_codes(im.astype(np.int16))
    with pytest.raises(ValueError):
        ros_codes(im.ravel())


def test_exports_and_struct_layouts_match_the_header(tmp_path):
    from yag_slam_amd import _capi
    L = _capi.lib()
    hdr = open(os.path.join(REPO, "include", "yagmatch.h")).read()
    code = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    for f in FUNCS:
        assert re.search(r"\b%s\s*\(" % f, code), f
        assert f in _capi.EXPORTS and hasattr(L, f), f
    assert C.sizeof(_capi.YmDespeckleOpts) == 16 and C.sizeof(_capi.YmDespeckleStats) == 48
    assert _capi.YmDespeckleStats.background_filled.offset == 40
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


def test_python_refuses_bad_arguments_before_the_library_is_touched(monkeypatch):
    from yag_slam_amd import _capi, occupancy

    def no_library():
        raise AssertionError("the library was touched")
    monkeypatch.setattr(_capi, "lib", no_library)
    im = np.zeros((4, 4), np.uint8)
    for kw in ({"connectivity": 6}, {"connectivity": 0}, {"connectivity": 8.0}, {"foreground": -1}, {"foreground": 256}, {"fill": 256},
               {"fill": -1}, {"min_area": -1}, {"min_area": 2 ** 31}, {"min_area": 2.5}, {"foreground": True}):
        with pytest.raises(ValueError, match=list(kw)[0]):
            occupancy.despeckle(im, **kw)
    for bad in (im.astype(np.int32), im.ravel(), np.zeros((0, 4), np.uint8), np.zeros((2, 2, 2), np.uint8), [[0, 1]]):
        with pytest.raises(ValueError, match="image"):
            occupancy.despeckle(bad)
    for kw in ({"connectivity": 6}, {"min_area": -1}):
        with pytest.raises(ValueError, match=list(kw)[0]):
            occupancy.create_clean_occupancy_grid([], 0.05, 12.0, **kw)
        with pytest.raises(ValueError, match=list(kw)[0]):
            occupancy.ros_map([], 0.05, 12.0, **kw)


def test_library_refuses_bad_arguments_before_any_device_work():
    """on a host without a device these would otherwise end in YM_ERR_NO_DEVICE: the checks come first"""
    from yag_slam_amd import _capi
    L = _capi.lib()
    u8 = C.POINTER(C.c_uint8)
    im = np.zeros((4, 4), np.uint8)
    out = np.full((4, 4), 9, np.uint8)
    st = _capi.YmDespeckleStats()
    st.components = 77

    def call(opts, image=im, w=4, h=4, pitch=4, o=out):
        return L.ym_image_despeckle(0, image.ctypes.data_as(u8) if image is not None else None, w, h, pitch,
                                    C.byref(opts) if opts is not None else None, o.ctypes.data_as(u8) if o is not None else None, C.byref(st))
    for opts, text in ((_capi.YmDespeckleOpts(0, 255, 5, 6), "connectivity 6"), (_capi.YmDespeckleOpts(0, 255, 5, 0), "connectivity 0"),
                       (_capi.YmDespeckleOpts(256, 255, 5, 8), "foreground 256"), (_capi.YmDespeckleOpts(0, -1, 5, 8), "fill -1"),
                       (_capi.YmDespeckleOpts(0, 255, -1, 8), "min_area -1")):
        assert call(opts) == -1 and text in _capi.last_error(), _capi.last_error()
        vp = C.c_void_p
        assert not L.ym_occupancy_create_clean((vp * 1)(None), 1, 0.05, 12.0, C.byref(opts)) and text in _capi.last_error()
    ok = _capi.YmDespeckleOpts(0, 255, 5, 8)
    assert call(ok, image=None) == -1 and "null" in _capi.last_error()
    assert call(ok, o=None) == -1 and "null" in _capi.last_error()
    assert call(ok, w=0) == -1 and "0 x 4" in _capi.last_error()
    assert call(ok, pitch=3) == -1 and "pitch 3" in _capi.last_error()
    assert call(ok, w=65536, h=32768, pitch=65536) == -4 and "2^31 - 1" in _capi.last_error()  # YM_ERR_UNSUPPORTED: one cell too many
    assert L.ym_occupancy_get_despeckle_stats(None, C.byref(st)) == -1 and "null" in _capi.last_error()
    assert np.all(out == 9) and st.components == 77


@pytest.fixture(scope="module")
def rendered():
    return {name: occupancy_ref.render(D.loop_scans(40, dirty), res, rt)[0] for name, (res, rt, dirty) in D.RENDER_SETS.items()}


def test_fixtures_have_what_the_gpu_tests_compare(rendered):
    """the reference alone, with the counts of the issue's table: specks to remove, walls to keep, and one set on which the
    two connectivities part"""
    a = rendered["0.05_clean"]
    assert a.shape == (121, 161)
    for conn in (4, 8):
        st = D.despeckle(a, connectivity=conn)[1]
        assert (st["foreground_cells"], st["components"], st["removed_components"], st["cleared_cells"]) == (880, 42, 24, 37)
    b = rendered["0.02_dirty"]
    assert b.shape == (304, 403)
    out8, st8 = D.despeckle(b, connectivity=8)
    out4, st4 = D.despeckle(b, connectivity=4)
    assert (st8["foreground_cells"], st8["components"], st8["removed_components"], st8["cleared_cells"]) == (3337, 17, 6, 7)
    assert (st4["foreground_cells"], st4["components"], st4["removed_components"], st4["cleared_cells"]) == (3337, 22, 11, 13)
    assert not np.array_equal(out8, out4)
    for st in (st8, st4, D.despeckle(a)[1]):
        assert st["removed_components"] >= 5 and st["components"] - st["removed_components"] >= 5
        assert st["background_filled"] == 0
    # the third row of the table, which no GPU test renders: the counts hold there too
    c = occupancy_ref.render(D.loop_scans(40, True), 0.05, 3.0)[0]
    st = D.despeckle(c)[1]
    assert (st["foreground_cells"], st["components"], st["removed_components"], st["cleared_cells"]) == (839, 46, 32, 64)
