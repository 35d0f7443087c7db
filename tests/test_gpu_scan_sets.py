"""`match_scan_sets` on the device (ym_match_sets / ym_match_sets_many) against what the REFERENCE's own
`Scan2DMatcherPy.match_scan_sets` produced (tests/golden/make_golden_scan_sets.py), and -- on inputs no fixture has -- against the
numpy restatement that reproduces those fixtures (tests/scansets_ref.py, tests/test_scan_sets_host.py)."""
import ctypes as C
import gc
import math

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from tests import scansets_ref as S  # noqa: E402
from tests.test_scan_sets_host import CASES, load_case, restated  # noqa: E402

UNSUPPORTED = -4


def _native(triple):
    from yag_slam_amd.models import LocalizedRangeScan
    r, p, s = triple
    n = len(r)
    return LocalizedRangeScan(r, s["min_angle"], s["min_angle"] + (n - 1) * s["angle_increment"], s["angle_increment"], s["min_range"],
                              30.0, s["range_threshold"], float(p[0]), float(p[1]), float(p[2]))


def _case(name):
    from yag_slam_amd.scan_matching import ScanMatcher
    z, cfg, queries, base = load_case(name)
    return z, ScanMatcher(cfg, semantics="yagpy"), [_native(q) for q in queries], [_native(b) for b in base]


def _handles(m, scans):
    return (C.c_void_p * max(1, len(scans)))(*[m._require_native(s) for s in scans])


def _raw_one(m, qs, bs, penalty, fine):
    from yag_slam_amd import _capi
    res = _capi.YmResult()
    _capi.check(m._lib.ym_match_sets(m._m, _handles(m, qs), len(qs), _handles(m, bs), len(bs), int(penalty), int(fine), C.byref(res)))
    return res


def _raw_many(m, sets, chains, penalty, fine):
    from yag_slam_amd import _capi
    fq, oq, fb, ob = [], [0], [], [0]
    for s, c in zip(sets, chains):
        fq += list(s)
        oq.append(len(fq))
        fb += list(c)
        ob.append(len(fb))
    per = (_capi.YmResult * len(sets))()
    _capi.check(m._lib.ym_match_sets_many(m._m, _handles(m, fq), (C.c_int32 * len(oq))(*oq), _handles(m, fb), (C.c_int32 * len(ob))(*ob),
                                          len(sets), int(penalty), int(fine), per))
    return per


def _sums(m, res, item=0):
    """both sum volumes [nt][ny][nx] of an item of the last set call (the second is None without a fine pass)"""
    c, f = tuple(res.coarse_dims), tuple(res.fine_dims)
    return m.debug_sums(0, item, c), (m.debug_sums(1, item, f) if f[0] else None)


def _key(r):
    return (r.response, tuple(map(tuple, r.covariance)), tuple((p.x, p.y, p.euler[-1]) for p in r.best_pose),
            tuple((p.x, p.y, p.euler[-1]) for p in r.meta["rigid_poses"]), r.meta["corrected_centre"], r.meta["n_query_points"])


def _check_against(r, m, want, grid=True):
    """a match_scan_sets result and the matcher's debug state against a restatement / fixture dict `want`"""
    assert r.meta["n_query_points"] == want["n_points"]
    assert r.meta["centre"][:2] == tuple(want["centre"])
    if grid:
        g, info = m.debug_grid(0)
        assert g.shape == (want["G"], want["G"])
        assert np.array_equal(g, want["g8"].astype(np.uint8))
    cs = m.debug_sums(0, 0, r.meta["coarse_dims"])
    assert np.array_equal(cs, want["coarse_sums"])
    if want.get("fine_sums") is not None:
        assert np.array_equal(m.debug_sums(1, 0, r.meta["fine_dims"]), want["fine_sums"])
    assert abs(r.meta["coarse_response"] - want["coarse"][0]) <= 1e-12
    assert abs(r.response - want["response"]) <= 1e-12
    np.testing.assert_allclose(r.meta["corrected_centre"], want["corrected_centre"], rtol=0, atol=1e-9)
    np.testing.assert_allclose(np.array(r.covariance), want["covariance"], rtol=1e-9, atol=1e-15)
    np.testing.assert_allclose(np.array([(p.x, p.y, p.euler[-1]) for p in r.best_pose]), np.array(want["poses"]), rtol=0, atol=1e-9)


@pytest.mark.parametrize("name", CASES)
def test_every_fixture_through_match_scan_sets(name):
    from yag_slam_amd.scan_matching import _move_rigidly
    z, m, qs, bs = _case(name)
    r = m.match_scan_sets(qs, bs, bool(z["penalty"]), bool(z["do_fine"]))
    G = int(z["grid_size"])
    g8 = np.zeros((G, G), dtype=np.int64)
    g8[z["grid_nz_y"], z["grid_nz_x"]] = (100 * z["grid_nz_val"]).astype(np.int64)
    want = dict(n_points=len(z["pts_local_x"]), centre=(float(z["centre"][0]), float(z["centre"][1])), G=G, g8=g8,
                coarse_sums=z["coarse_sums"], fine_sums=z["fine_sums"] if bool(z["do_fine"]) else None, coarse=z["coarse"],
                response=float(z["response"]), corrected_centre=z["final"][1:4], covariance=z["covariance"], poses=z["poses"])
    _check_against(r, m, want)
    g, info = m.debug_grid(0)
    nzy, nzx = np.nonzero(g)
    assert np.array_equal(nzy, z["grid_nz_y"]) and np.array_equal(nzx, z["grid_nz_x"])
    assert (info.offset_x, info.offset_y) == restated(name)["origin"]
    pts = m.debug_query_local(0)
    np.testing.assert_allclose(pts[:, 0], z["pts_local_x"], rtol=0, atol=1e-12)
    np.testing.assert_allclose(pts[:, 1], z["pts_local_y"], rtol=0, atol=1e-12)
    c0, c1 = r.meta["centre"], r.meta["corrected_centre"]
    rigid = _move_rigidly([q.corrected_pose for q in qs], c0[0], c0[1], c1[0], c1[1], c1[2] - c0[2])
    assert [(p.x, p.y, p.euler[-1]) for p in r.meta["rigid_poses"]] == [(p.x, p.y, p.euler[-1]) for p in rigid]
    if not bool(z["do_fine"]):
        assert r.meta["fine_dims"] == (0, 0, 0) and r.covariance[2][2] == 4 * m.config.coarse_angle_resolution


@pytest.mark.parametrize("name", CASES)
def test_the_fast_path_and_the_rule_as_written_agree(name):
    z, m, qs, bs = _case(name)
    pen, fine = bool(z["penalty"]), bool(z["do_fine"])
    a = _raw_one(m, qs, bs, pen, fine)
    sa = _sums(m, a)
    c = m.debug_counters()
    assert (c["sets_kernel_items"], c["sets_fallback_items"]) == (1, 0)  # no fallback on a fixture unforced
    m.debug_option(46, 0)  # both passes pair by pair
    b = _raw_one(m, qs, bs, pen, fine)
    sb = _sums(m, b)
    c = m.debug_counters()
    assert (c["sets_kernel_items"], c["sets_fallback_items"]) == (1, 1)
    assert bytes(a) == bytes(b) and a.status == 0
    assert np.array_equal(sa[0], sb[0]) and np.array_equal(sa[0], z["coarse_sums"])
    if fine:
        assert np.array_equal(sa[1], sb[1]) and np.array_equal(sa[1], z["fine_sums"])


def test_a_batch_equals_its_single_calls_whatever_the_chunk_length():
    z, m, qs, bs = _case("scan_sets_two")
    sets = [qs] * 9
    chains = [bs] * 9
    chains[1] = bs[:2]   # a shorter chain
    sets[4] = qs[:1]     # a one-scan set
    singles = [_raw_one(m, s, c, True, True) for s, c in zip(sets, chains)]
    assert bytes(singles[0]) != bytes(singles[1]) and bytes(singles[0]) != bytes(singles[4])
    per = _raw_many(m, sets, chains, True, True)
    for i in range(9):
        assert bytes(per[i]) == bytes(singles[i]), (i, per[i].response, singles[i].response, per[i].status)
    for i in (0, 3, 6, 8):
        cs, fs = _sums(m, per[i], i)
        assert np.array_equal(cs, z["coarse_sums"]) and np.array_equal(fs, z["fine_sums"]), i
    assert m.debug_counters()["sets_fallback_items"] == 0
    m.debug_option(48, 2)  # five chunks, the last of one item
    per2 = _raw_many(m, sets, chains, True, True)
    assert [bytes(r) for r in per2] == [bytes(r) for r in singles]
    cs, fs = _sums(m, per2[8], 8)
    assert np.array_equal(cs, z["coarse_sums"]) and np.array_equal(fs, z["fine_sums"])
    g, _ = m.debug_grid(8)  # (the last chunk's grid is still there)
    assert np.array_equal(np.nonzero(g)[0], z["grid_nz_y"])
    m.debug_option(48, 0)
    # one set broadcast over N chains: the loop-closure use
    three = [bs, bs[:2], bs[1:]]
    got = m.match_scan_sets_batch(qs, three)
    assert [_key(r) for r in got] == [_key(m.match_scan_sets(qs, c)) for c in three]
    assert _key(got[0]) != _key(got[1])
    assert [_key(r) for r in m.match_scan_sets_batch([qs, qs[:1]], [bs, bs[:2]], penalty=False, do_fine=False)] == \
        [_key(m.match_scan_sets(qs, bs, False, False)), _key(m.match_scan_sets(qs[:1], bs[:2], False, False))]


def test_an_item_without_a_query_point_leaves_its_neighbours_alone():
    from yag_slam_amd import _capi
    z, m, qs, bs = _case("scan_sets_two")
    _, _, q3, _ = load_case("scan_sets_r02_blank")
    blank = _native((q3[1][0], (2.3, 3.0, 0.0), q3[1][2]))  # no valid reading
    sets = [qs, [blank], qs[:1], [blank, blank], qs]
    chains = [bs, bs, bs[:2], bs, bs[1:]]
    got = m.match_scan_sets_batch(sets, chains, strict=False)
    assert [r is None for r in got] == [False, True, False, True, False]
    for i in (0, 2, 4):
        assert _key(got[i]) == _key(m.match_scan_sets(sets[i], chains[i]))
    per = _raw_many(m, sets, chains, True, True)
    assert [r.status != 0 for r in per] == [False, True, False, True, False] and per[1].n_query_points == 0
    for i in (0, 2, 4):
        assert bytes(per[i]) == bytes(_raw_one(m, sets[i], chains[i], True, True))
    with pytest.raises(_capi.YmError):
        m.match_scan_sets_batch(sets, chains)
    with pytest.raises(_capi.YmError):
        m.match_scan_sets([blank], bs)


# ---- block and wave edges against the restatement ------------------------------------------------------------------------------
EDGE_CFG = dict(resolution=0.05, smear_deviation=0.05, range_threshold=12.0, search_size=1.0, coarse_search_angle_offset=0.349,
                coarse_angle_resolution=0.0349)
_EDGE = {}


def _edge_inputs(beams, blank_last=False, blank_base=False):
    """a seeded set (one scan per entry of `beams`, every reading valid) and a chain of three scans for which the restatement meets no
    decision within 1e-9 of its boundary; computed once per shape"""
    from yag_slam_amd import synth
    key = (tuple(beams), blank_last, blank_base)
    if key in _EDGE:
        return _EDGE[key]
    scene = synth.Scene()
    for seed in range(16):
        def triple(n, truth, prior, index, blank=False):
            inc = 1.5 * math.pi / (n - 1)
            sensor = dict(min_angle=-0.75 * math.pi, angle_increment=inc, min_range=synth.MIN_RANGE, range_threshold=12.0)
            r = scene.scan_ranges(truth, index=index + 1000 * seed, n_beams=n, min_angle=sensor["min_angle"], inc=inc)
            if blank:
                r = np.where(np.arange(n) % 2 == 0, np.nan, 31.0)
            return (r, prior, sensor)
        queries = [triple(n, (3.04 + 0.1 * i, 3.03, 0.03), (3.0 + 0.1 * i, 3.0, 0.0), 600 + i) for i, n in enumerate(beams)]
        if blank_last:  # no reading, but its position -- behind the boxes along the wall -- is the filter's view-point
            queries.append(triple(181, (6.5, 0.6, 0.0), (6.5, 0.6, 0.0), 700, blank=True))
        base = [triple(181, p, p, 10 + i, blank=(blank_base and i == 1)) for i, p in enumerate([(2.8, 3.0, 0.0), (3.0, 3.1, 0.2), (3.3, 2.9, -0.2)])]
        ref = S.match_scan_sets(EDGE_CFG, queries, base, True, True)
        if min(ref["tie"], ref["near_d"], ref["near_s"]) >= 1e-9:
            break
    else:
        raise AssertionError("no seed keeps every decision 1e-9 from its boundary")
    ref["corrected_centre"] = np.array(ref["corrected_centre"])
    _EDGE[key] = (queries, base, ref)
    return _EDGE[key]


def _split(total):
    return [total // 2, total - total // 2]


@pytest.mark.parametrize("beams", [_split(63), _split(64), _split(65), _split(255), _split(256), _split(257), _split(1025), [1081] * 7],
                         ids=["63", "64", "65", "255", "256", "257", "1025", "7x1081"])
def test_block_and_wave_edges_against_the_restatement(beams):
    from yag_slam_amd.scan_matching import ScanMatcher
    queries, base, ref = _edge_inputs(beams)
    assert ref["n_points"] == sum(beams) and ref["status"] == 0  # (every reading is one; 7 x 1081 is above a scan's 6000 in total)
    m = ScanMatcher(EDGE_CFG, semantics="yagpy")
    r = m.match_scan_sets([_native(q) for q in queries], [_native(b) for b in base])
    _check_against(r, m, ref)
    assert m.debug_counters()["sets_fallback_items"] == 0


@pytest.mark.parametrize("what", ["blank_last_query", "blank_base_scan"])
def test_scans_without_a_reading_against_the_restatement(what):
    from yag_slam_amd.scan_matching import ScanMatcher
    queries, base, ref = _edge_inputs([181, 181], blank_last=what == "blank_last_query", blank_base=what == "blank_base_scan")
    m = ScanMatcher(EDGE_CFG, semantics="yagpy")
    r = m.match_scan_sets([_native(q) for q in queries], [_native(b) for b in base])
    _check_against(r, m, ref)
    if what == "blank_last_query":
        # the blank scan counts in the mean and is the view-point: the kept readings differ from those under the first query's
        assert ref["n_points"] == 362 and ref["view"] == (6.5, 0.6)
        other = S.build_grid(EDGE_CFG, ref["G"], ref["origin"][0], ref["origin"][1], base, (queries[0][1][0], queries[0][1][1]))[1]
        assert other != ref["kept"]
    else:
        assert ref["kept"][1] == 0 and ref["kept"][0] > 0 and ref["kept"][2] > 0


# ---- the matcher's kept state --------------------------------------------------------------------------------------------------
def test_set_calls_neither_see_nor_disturb_what_the_matcher_keeps():
    from yag_slam_amd import synth
    from yag_slam_amd.scan_matching import ScanMatcher
    z, _, qs, bs = _case("scan_sets_two")
    cfg = load_case("scan_sets_two")[1]
    scene = synth.Scene()
    base_poses, q_truth, q_prior = synth.single_match_poses()
    q = synth.resident_scan(scene.scan_ranges(q_truth, index=10), q_prior, 12.0)
    exact = [scene.cast(*p) for p in base_poses[:4]]
    chains = []
    for c in range(64):
        rng = np.random.default_rng(9000 + c)
        chains.append([synth.resident_scan(e + rng.normal(0.0, synth.SIGMA_RANGE, size=e.shape), p, 12.0) for e, p in zip(exact, base_poses)])
    image = np.full((140, 180), 255, dtype=np.uint8)
    image[[20, 120], 20:160] = 0
    image[20:121, [20, 159]] = 0
    key1 = lambda r: (r.response, tuple(map(tuple, r.covariance)), r.best_pose.x, r.best_pose.y, r.best_pose.euler[-1])  # noqa: E731

    def run(m, with_sets):
        out = []
        out.append(key1(m.match_scan(q, chains[0], True, True)))
        out.append(m.debug_sums(0, 0, m.match_scan(q, chains[0], True, True).meta["coarse_dims"]).tobytes())
        out.append([key1(r) for r in m.match_scan_batch(q, chains, True, True)[0]])
        if with_sets:
            a = m.match_scan_sets(qs, bs)
            assert np.array_equal(m.debug_sums(0, 0, a.meta["coarse_dims"]), z["coarse_sums"])
            b = m.match_scan_sets_batch(qs, [bs, bs[:2], bs[1:]])
            assert _key(b[0]) == _key(a)
            cmap = m.correlation_grid_from_occupancy(image, occupied_value=0)
            m.match_map_batch(cmap, -1.0, -1.0, [[q], [qs[0], qs[1]]], strict=False)
            cmap.close()
            assert _key(m.match_scan_sets(qs, bs)) == _key(a)  # (a map call in between changes nothing for a set call either)
        out.append([key1(r) for r in m.match_scan_batch(q, chains, True, True)[0]])
        out.append(key1(m.match_scan(q, chains[0], True, True)))
        out.append(m.debug_sums(0, 0, m.match_scan(q, chains[0], True, True).meta["coarse_dims"]).tobytes())
        return out, m.debug_counters()["list_cache_hits"]
    got, hits = run(ScanMatcher(cfg, semantics="yagpy"), True)
    want, hits0 = run(ScanMatcher(cfg, semantics="yagpy"), False)
    assert got == want and got[0] == got[4] and got[1] == got[5] and got[2] == got[3]
    assert hits == hits0  # the pair lists kept from call to call are found, or built again, exactly as without the set calls


def test_a_karto_matcher_is_refused_and_nothing_changes():
    from yag_slam_amd import _capi
    from yag_slam_amd.scan_matching import ScanMatcher
    z, _, qs, bs = _case("scan_sets_two")
    cfg = load_case("scan_sets_two")[1]
    m = ScanMatcher(cfg)  # "karto"
    key1 = lambda r: (r.response, tuple(map(tuple, r.covariance)), r.best_pose.x, r.best_pose.y, r.best_pose.euler[-1])  # noqa: E731
    before = key1(m.match_scan(qs[0], bs, True, True))
    sums = m.debug_sums(0, 0, m.coarse_dims()).tobytes()
    res = _capi.YmResult()
    res.response = 123.0
    assert m._lib.ym_match_sets(m._m, _handles(m, qs), len(qs), _handles(m, bs), len(bs), 1, 1, C.byref(res)) == UNSUPPORTED
    assert "YM_SEM_YAGPY" in _capi.last_error() and res.response == 123.0
    per = (_capi.YmResult * 1)()
    per[0].response = 123.0
    off = (C.c_int32 * 2)(0, 2)
    assert m._lib.ym_match_sets_many(m._m, _handles(m, qs), off, _handles(m, bs), off, 1, 1, 1, per) == UNSUPPORTED
    assert per[0].response == 123.0
    with pytest.raises(_capi.YmError):
        m.match_scan_sets(qs, bs)
    assert m.debug_sums(0, 0, m.coarse_dims()).tobytes() == sums  # (the debug getters still describe the match call)
    assert key1(m.match_scan(qs[0], bs, True, True)) == before
    c = m.debug_counters()
    assert (c["sets_kernel_items"], c["sets_fallback_items"]) == (0, 0)


def test_a_matcher_that_served_set_calls_gives_back_its_memory():
    from tests.test_gpu_lifetime import live
    from yag_slam_amd.scan_matching import ScanMatcher
    z, cfg, queries, base = load_case("scan_sets_two")
    before = live()
    m = ScanMatcher(cfg, semantics="yagpy")
    qs, bs = [_native(q) for q in queries], [_native(b) for b in base]
    m.match_scan_sets(qs, bs)
    m.match_scan_sets_batch(qs, [bs, bs[:2], bs[1:]])
    m.debug_option(48, 2)
    m.match_scan_sets_batch([qs, qs[:1], qs], [bs, bs, bs[:1]], do_fine=False)
    assert live() != before
    m.close()
    del qs, bs, m
    gc.collect()
    assert live() == before
