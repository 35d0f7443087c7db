"""`match_scan_sets` without a device (include/yagmatch.h ym_match_sets / ym_match_sets_many): the numpy
restatement (tests/scansets_ref.py) against every fixture the reference made (tests/golden/make_golden_scan_sets.py), the properties
the fixtures were constructed for, the ABI against the header read through a C compiler, the refusals that need no device, and the
Python batch call's refusals before the library is touched."""
import ctypes as C
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

from tests import scansets_ref as S
from tests.util import GOLDEN, REPO

CASES = ["scan_sets_two", "scan_sets_one_coarse", "scan_sets_dirty_three", "scan_sets_far_base", "scan_sets_r02_blank"]
FUNCS = ("ym_match_sets", "ym_match_sets_many")

# what yag_slam_amd/_capi.py declares, spelled as C prototypes
PROTOS = """
int (*p_sets)(ym_matcher *, const ym_scan *const *, int, const ym_scan *const *, int, int, int, ym_result *) = ym_match_sets;
int (*p_many)(ym_matcher *, const ym_scan *const *, const int32_t *, const ym_scan *const *, const int32_t *, int, int, int,
              ym_result *) = ym_match_sets_many;
"""

_CACHE = {}


def load_case(name):
    """the fixture, its configuration and its scans as (ranges, pose, sensor) triples"""
    z = np.load(os.path.join(GOLDEN, name + ".npz"))
    cfg = {str(k): float(v) for k, v in zip(z["cfg_keys"], z["cfg_vals"])}

    def sensor(t):
        return dict(min_angle=float(z["sensor_min_angle"]), angle_increment=float(z["sensor_angle_increment"]),
                    min_range=float(z["sensor_min_range"]), range_threshold=float(t))
    queries = [(r, tuple(p), sensor(t)) for r, p, t in zip(z["q_ranges"], z["q_poses"], z["q_thresholds"])]
    base = [(r, tuple(p), sensor(t)) for r, p, t in zip(z["base_ranges"], z["base_poses"], z["base_thresholds"])]
    return z, cfg, queries, base


def restated(name):
    """the restatement's result on a fixture's inputs, computed once for all tests of the session"""
    if name not in _CACHE:
        z, cfg, queries, base = load_case(name)
        _CACHE[name] = S.match_scan_sets(cfg, queries, base, bool(z["penalty"]), bool(z["do_fine"]))
    return _CACHE[name]


@pytest.mark.parametrize("name", CASES)
def test_the_restatement_reproduces_the_reference(name):
    z = load_case(name)[0]
    r = restated(name)
    assert r["status"] == 0 and r["G"] == int(z["grid_size"])
    assert r["centre"] == (float(z["centre"][0]), float(z["centre"][1]))
    assert r["kept"] == z["valid_counts"].tolist()
    nzy, nzx = np.nonzero(r["grid"])
    assert np.array_equal(nzy, z["grid_nz_y"]) and np.array_equal(nzx, z["grid_nz_x"])
    assert np.array_equal(r["g8"][nzy, nzx], (100 * z["grid_nz_val"]).astype(np.int64))
    np.testing.assert_allclose(r["grid"][nzy, nzx], z["grid_nz_val"], rtol=0, atol=1e-15)
    assert r["n_points"] == len(z["pts_local_x"])
    np.testing.assert_allclose(r["pts"][0], z["pts_local_x"], rtol=0, atol=1e-12)
    np.testing.assert_allclose(r["pts"][1], z["pts_local_y"], rtol=0, atol=1e-12)
    assert np.array_equal(r["coarse_sums"], z["coarse_sums"])
    assert abs(r["coarse"][0] - z["coarse"][0]) <= 1e-12
    if bool(z["do_fine"]):
        assert np.array_equal(r["fine_sums"], z["fine_sums"])
    else:
        assert "fine_sums" not in r and "fine_sums" not in z.files
    assert abs(r["response"] - float(z["response"])) <= 1e-12
    np.testing.assert_allclose(r["coarse"][1:4], z["coarse"][1:4], rtol=0, atol=1e-9)
    np.testing.assert_allclose(r["corrected_centre"], z["final"][1:4], rtol=0, atol=1e-9)
    np.testing.assert_allclose(r["covariance"], z["covariance"], rtol=1e-9, atol=1e-15)
    np.testing.assert_allclose(np.array(r["poses"]), z["poses"], rtol=0, atol=1e-9)
    # every decision the fixture turns on lies clear of its boundary, by the restatement's own count and by the generator's
    assert min(r["tie"], r["near_d"], r["near_s"]) >= 1e-9
    assert min(float(z["margin_tie"]), float(z["margin_d2"]), float(z["margin_ss"])) >= 1e-9


def test_the_fixtures_hold_what_they_were_constructed_for():
    z = load_case("scan_sets_dirty_three")[0]
    assert np.isnan(z["q_ranges"]).any() and (z["q_ranges"] > 12.0).any() and len(z["q_poses"]) == 3
    assert (z["valid_counts"] != z["valid_counts_first"]).any() and (z["valid_counts"] != z["valid_counts_mean"]).any()
    # the returned poses are diff (+) q, which is no rigid motion of the set: the distance between two of them changes
    z = load_case("scan_sets_two")[0]
    r = restated("scan_sets_two")
    rigid = [S.compose(S.compose(r["corrected_centre"], S.inverse((r["centre"][0], r["centre"][1], 0.0))), tuple(p)) for p in z["q_poses"]]
    assert np.abs(np.array(rigid) - z["poses"]).max() > 1e-3
    # a base sensor that sees farther than the matcher's threshold: readings outside G x G, stamps on its rim
    z, cfg, _, base = load_case("scan_sets_far_base")
    assert float(z["base_thresholds"][0]) > cfg["range_threshold"]
    r = restated("scan_sets_far_base")
    G, half = r["G"], S.smear_kernel(cfg["resolution"], cfg["smear_deviation"]).shape[0] // 2
    outside = rim = 0
    for ranges, pose, sensor in base:
        px, py = S.point_readings(ranges, pose, sensor)
        keep = S.validate(px, py, *r["view"])[0]
        gx = np.round((px[keep] - r["origin"][0]) / cfg["resolution"])
        gy = np.round((py[keep] - r["origin"][1]) / cfg["resolution"])
        inside = (gx >= 0) & (gx < G) & (gy >= 0) & (gy < G)
        outside += int((~inside).sum())
        rim += int((inside & ((gx < half) | (gx >= G - half) | (gy < half) | (gy >= G - half))).sum())
    assert outside > 0 and rim > 0
    # a query scan without a valid reading in the middle of the set, and lattices that differ between the passes
    z = load_case("scan_sets_r02_blank")[0]
    with np.errstate(invalid="ignore"):
        assert not (z["q_ranges"][1] <= 12.0).any() and (z["q_ranges"][0] <= 12.0).any() and (z["q_ranges"][2] <= 12.0).any()
    assert z["coarse_sums"].shape != z["fine_sums"].shape
    for name in CASES:
        assert os.path.getsize(os.path.join(GOLDEN, name + ".npz")) < 64 * 1024


def test_the_view_point_is_the_last_query_not_the_first_and_not_the_mean():
    z, cfg, queries, base = load_case("scan_sets_dirty_three")
    r = restated("scan_sets_dirty_three")
    assert r["view"] == (float(z["q_poses"][-1][0]), float(z["q_poses"][-1][1]))
    for view, want in ((r["view"], z["valid_counts"]), (tuple(z["q_poses"][0][:2]), z["valid_counts_first"]), (r["centre"], z["valid_counts_mean"])):
        got = [int(S.validate(*S.point_readings(rr, p, s), view[0], view[1])[0].sum()) for rr, p, s in base]
        assert got == want.tolist()


def test_exports_and_argtypes_match_the_header(tmp_path):
    from yag_slam_amd import _capi
    L = _capi.lib()
    hdr = open(os.path.join(REPO, "include", "yagmatch.h")).read()
    code = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    for f in FUNCS:
        assert re.search(r"\b%s\s*\(" % f, code), f
        assert f in _capi.EXPORTS and hasattr(L, f), f
    vp, ip = C.c_void_p, C.POINTER(C.c_int32)
    assert list(L.ym_match_sets.argtypes) == [vp, C.POINTER(vp), C.c_int, C.POINTER(vp), C.c_int, C.c_int, C.c_int, C.POINTER(_capi.YmResult)]
    assert list(L.ym_match_sets_many.argtypes) == [vp, C.POINTER(vp), ip, C.POINTER(vp), ip, C.c_int, C.c_int, C.c_int,
                                                   C.POINTER(_capi.YmResult)]
    cc = shutil.which("cc") or shutil.which("gcc") or shutil.which("clang")
    assert cc, "no C compiler to read the header with"
    src = tmp_path / "protos.c"
    src.write_text('#include <stdio.h>\n#include "yagmatch.h"\n%s\nint main(void) { printf("%%d %%zu\\n", YM_DEBUG_COUNTERS, sizeof(ym_result)); return 0; }\n'
                   % PROTOS)
    obj = str(tmp_path / "protos.o")
    subprocess.run([cc, "-Wall", "-Werror", "-I", os.path.join(REPO, "include"), "-c", "-o", obj, str(src)], check=True, capture_output=True)
    stub = tmp_path / "stubs.c"  # (the entries are only named, never called: the program links against empty stand-ins)
    stub.write_text("".join("int %s(void) { return 0; }\n" % f for f in FUNCS))
    exe = str(tmp_path / "protos")
    subprocess.run([cc, "-o", exe, obj, str(stub)], check=True, capture_output=True)
    n, size = subprocess.run([exe], check=True, capture_output=True, text=True).stdout.split()
    assert int(n) == 10 and int(size) == C.sizeof(_capi.YmResult)


def test_null_negative_empty_and_overlong_arguments_are_refused_before_any_device_is_touched():
    from yag_slam_amd import _capi
    L = _capi.lib()
    fake = C.c_void_p(16)  # never dereferenced: an argument beside it is refused first
    res = _capi.YmResult()
    many = (_capi.YmResult * 2)()
    scans = (C.c_void_p * 70)(*([16] * 70))  # (not dereferenced either: the counts are refused before a scan is looked at)
    i32 = lambda *v: (C.c_int32 * len(v))(*v)  # noqa: E731
    inv = -1
    for args in ((None, scans, 1, scans, 1), (fake, None, 1, scans, 1), (fake, scans, 1, None, 1)):
        assert L.ym_match_sets(*args, 1, 1, C.byref(res)) == inv and "null" in _capi.last_error()
    assert L.ym_match_sets(fake, scans, 1, scans, 1, 1, 1, None) == inv and "null" in _capi.last_error()
    assert L.ym_match_sets(fake, scans, 0, scans, 1, 1, 1, C.byref(res)) == inv and "empty set" in _capi.last_error()
    assert L.ym_match_sets(fake, scans, -2, scans, 1, 1, 1, C.byref(res)) == inv and "empty set" in _capi.last_error()
    assert L.ym_match_sets(fake, scans, 65, scans, 1, 1, 1, C.byref(res)) == inv and "1 to 64" in _capi.last_error()
    assert L.ym_match_sets(fake, scans, 1, scans, -1, 1, 1, C.byref(res)) == inv and "negative" in _capi.last_error()
    so, co = i32(0, 1, 2), i32(0, 1, 2)
    for args in ((None, scans, so, scans, co), (fake, None, so, scans, co), (fake, scans, None, scans, co), (fake, scans, so, None, co),
                 (fake, scans, so, scans, None)):
        assert L.ym_match_sets_many(*args, 2, 1, 1, many) == inv and "null" in _capi.last_error()
    assert L.ym_match_sets_many(fake, scans, so, scans, co, 2, 1, 1, None) == inv and "null" in _capi.last_error()
    for n in (0, -1, 2 ** 20 + 1):
        assert L.ym_match_sets_many(fake, scans, so, scans, co, n, 1, 1, many) == inv and "n_items" in _capi.last_error()
    assert L.ym_match_sets_many(fake, scans, i32(-1, 1, 2), scans, co, 2, 1, 1, many) == inv and "negative" in _capi.last_error()
    assert L.ym_match_sets_many(fake, scans, so, scans, i32(-1, 1, 2), 2, 1, 1, many) == inv and "negative" in _capi.last_error()
    assert L.ym_match_sets_many(fake, scans, i32(0, 1, 1), scans, co, 2, 1, 1, many) == inv and "empty set" in _capi.last_error()
    assert L.ym_match_sets_many(fake, scans, i32(0, 2, 1), scans, co, 2, 1, 1, many) == inv and "empty set" in _capi.last_error()
    assert L.ym_match_sets_many(fake, scans, i32(0, 1, 66), scans, co, 2, 1, 1, many) == inv and "1 to 64" in _capi.last_error()
    assert L.ym_match_sets_many(fake, scans, so, scans, i32(0, 2, 1), 2, 1, 1, many) == inv and "negative chain" in _capi.last_error()


class _Untouchable(object):
    """stands for a matcher whose library must not be reached"""

    def __getattr__(self, name):
        raise AssertionError("the library was touched: %s" % name)


def test_the_batch_call_refuses_empty_input_before_touching_the_library():
    from yag_slam_amd.scan_matching import ScanMatcher
    m = ScanMatcher.__new__(ScanMatcher)
    m._lib = m._m = _Untouchable()
    scan = object()
    with pytest.raises(ValueError):
        m.match_scan_sets_batch([], [[scan]])
    with pytest.raises(ValueError):
        m.match_scan_sets_batch([[scan]], [])
    with pytest.raises(ValueError):
        m.match_scan_sets_batch([[scan], []], [[scan], [scan]])
    with pytest.raises(ValueError):
        m.match_scan_sets_batch([[scan], [scan]], [[scan]])
    with pytest.raises(ValueError):
        m.match_scan_sets([], [scan])
    m._m = None  # (nothing to destroy)
