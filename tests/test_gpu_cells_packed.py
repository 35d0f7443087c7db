"""The per-item window cells are one 32-bit word each (x in the low 16 bits, y in the high 16, signed; x = -32768 = no cell) and
the point cache keeps a reading's deciding pair the same way (s, t).  Everything below is about what such halves can get wrong:
negative coordinates, coordinates past the window, the window's first and last row and column, "no cell", the largest window
there is, slots cleared on ragged batches, the select kernels' reads, the records' extreme values (s = -1, t = np) and the
geometry the format cannot hold.  Smallest shapes that reach each case; cells against the oracle's own pieces (point readings,
valid-point filter, WorldToGrid), window bytes against the oracle's grid, bit for bit."""
import itertools

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from tests.util import PlainScan, cfg2_scans  # noqa: E402

NONE = np.iinfo(np.int32).min
CFG = dict(range_threshold=6.0)  # (ROI of 51 + 1200 cells; the query below reaches 1 m, so the window is a small part of it)
QPOSE = (3.0, 3.0, 0.0)


def _mk_native(plain):
    from yag_slam_amd.models import LocalizedRangeScan
    p = plain.corrected_pose
    return LocalizedRangeScan(plain.ranges, plain.min_angle, plain.max_angle, plain.angle_increment,
                              plain.min_range, plain.max_range, plain.range_threshold, p.x, p.y, p.euler[-1])


def _ring(n, radius, wobble, phase):
    """n beams over the full circle, beam k at -pi + k * 2 pi / (n - 1 if n is odd else n): the beams at a quarter, a half and
    three quarters of the way point exactly down, right and up, beam 0 left"""
    per = n - 1 if n % 2 else n
    k = np.arange(n)
    return radius + wobble * np.sin(5 * (2 * np.pi * k / per) + phase), -np.pi, 2 * np.pi / per, per


def _query():
    r, a0, inc, _ = _ring(257, 1.0, 0.05, 0.3)
    return PlainScan(r, a0, inc, 0.05, 6.0, QPOSE)


def _kt_round(v):
    r = np.floor(np.abs(v) + 0.5).astype(np.int64)
    return np.where(v < 0.0, -r, r)


class _Geom:
    """window and region of interest of a call with `_query()` under CFG, read from a probe call"""

    def __init__(self, cfg=CFG):
        from yag_slam_amd.scan_matching import ScanMatcher
        m = ScanMatcher(cfg)
        r, a0, inc, _ = _ring(17, 0.8, 0.0, 0.0)
        m.match_scan(_mk_native(_query()), [_mk_native(PlainScan(r, a0, inc, 0.05, 6.0, QPOSE))], True, True)
        _, info = m.debug_grid()
        m.close()
        self.win_w, self.origin, self.border, self.roi_w = info.width, info.origin_x, info.roi_x, info.roi_w
        self.scale = 1.0 / 0.01
        self.res = 1.0 / self.scale
        self.off = [QPOSE[i] - (0.5 * (self.roi_w - 1) * self.res) for i in (0, 1)]
        assert (info.offset_x, info.offset_y) == tuple(self.off)

    def world(self, axis, cell):
        """world coordinate of the centre of window cell `cell` along `axis`"""
        return self.off[axis] + (cell + self.origin - self.border) * self.res

    def cells_of(self, scan):
        """the oracle's cells of one base scan: its point readings, the valid-point filter seen from the query, WorldToGrid"""
        from oracle import oracle as orc
        p = scan.corrected_pose
        xs, ys = orc.point_readings(scan.ranges, scan.min_angle, scan.angle_increment, scan.min_range, scan.range_threshold,
                                    (p.x, p.y, p.euler[-1]))
        keep = orc.valid_points(xs, ys, QPOSE[0], QPOSE[1])
        gx, gy = _kt_round((xs - self.off[0]) * self.scale), _kt_round((ys - self.off[1]) * self.scale)
        keep &= (gx >= 0) & (gx < self.roi_w) & (gy >= 0) & (gy < self.roi_w)
        out = np.full((len(xs), 2), NONE, dtype=np.int64)
        out[keep, 0] = gx[keep] + self.border - self.origin
        out[keep, 1] = gy[keep] + self.border - self.origin
        return out


def _edge_scan(geom, n, variant, targets):
    """A ring of n readings 0.8 m around a sensor a few cells off the query, with the four axis beams (left, down, right, up)
    lengthened so that their end points land in the window cells `targets` = (x of the left beam, y of the down beam, x of the
    right beam, y of the up beam); None leaves the beam on the ring, "far" sends it out of the region of interest."""
    r, a0, inc, per = _ring(n, 0.8, 0.03, 0.7 * variant)
    sx, sy = QPOSE[0] + 0.03 * variant, QPOSE[1] - 0.02 * variant
    for beam, axis, sign, pos, tgt in ((0, 0, -1.0, sx, targets[0]), (per // 4, 1, -1.0, sy, targets[1]),
                                       (per // 2, 0, 1.0, sx, targets[2]), (3 * per // 4, 1, 1.0, sy, targets[3])):
        if tgt is None:
            continue
        r[beam] = 7.5 if tgt == "far" else sign * (geom.world(axis, tgt) - pos)
        assert r[beam] > 0.9
    return PlainScan(r, a0, inc, 0.05, 8.0, (sx, sy, 0.0))  # (the scan's own threshold lets the 7.5 m reading through)


def _edge_chains(geom, n_items):
    w = geom.win_w
    variants = []
    for v in range(4):
        variants.append([
            _edge_scan(geom, 17, v, (-3 - v, -40, w + 2 + v, w + 300)),        # left of, above, right of, below the window
            _edge_scan(geom, 256, v, (0, 0, w - 1, w - 1)),                     # first and last column and row
            _edge_scan(geom, 257, v, ("far", -1, w, None)),                     # outside the region of interest; one cell outside
        ])
    orders = list(itertools.permutations(range(3)))
    return [[variants[i % 4][j] for j in orders[(i // 4) % 6]] for i in range(n_items)]


@pytest.fixture(scope="module")
def geom():
    return _Geom()


@pytest.fixture(scope="module")
def edge_oracle(geom):
    """per distinct chain (variant, order): the oracle's window bytes and result, computed once"""
    from oracle import oracle as orc
    o = orc.Oracle(CFG, "karto")
    q = _query()
    memo = {}
    for i, ch in enumerate(_edge_chains(geom, 24)):
        ro = o.match_scan(q, ch, True, True)
        og, _ = o.grid_u8()
        memo[i] = (ro, og[geom.origin:geom.origin + geom.win_w, geom.origin:geom.origin + geom.win_w].copy())
    return memo


@pytest.mark.parametrize("n_items", [8, 48])
def test_edge_coordinates_against_the_oracle(geom, edge_oracle, n_items):
    from yag_slam_amd.scan_matching import ScanMatcher
    chains = _edge_chains(geom, n_items)
    m = ScanMatcher(CFG)
    per, _ = m.match_scan_batch(_mk_native(_query()), [[_mk_native(s) for s in ch] for ch in chains], True, True)
    w = geom.win_w
    seen = dict(neg_x=False, neg_y=False, past_x=False, past_y=False, first=False, last=False, none_far=False)
    for i, ch in enumerate(chains):
        cells, max_n = m.debug_cells(i)
        assert max_n == 257
        cells = cells[:3 * max_n].reshape(3, max_n, 2)
        for slot, s in enumerate(ch):
            want = np.full((max_n, 2), NONE, dtype=np.int64)
            oc = geom.cells_of(s)
            want[:len(oc)] = oc
            assert np.array_equal(cells[slot], want), (i, slot, np.argwhere(cells[slot] != want)[:4])
            has = oc[:, 0] != NONE
            seen["neg_x"] |= bool((oc[has, 0] < 0).any())
            seen["neg_y"] |= bool((oc[has, 1] < 0).any())
            seen["past_x"] |= bool((oc[has, 0] >= w).any())
            seen["past_y"] |= bool((oc[has, 1] >= w).any())
            seen["first"] |= bool((oc[has, 0] == 0).any() and (oc[has, 1] == 0).any())
            seen["last"] |= bool((oc[has, 0] == w - 1).any() and (oc[has, 1] == w - 1).any())
            if len(s.ranges) == 257:  # beam 0 is a point reading 7.5 m out: beyond the region of interest, no cell
                seen["none_far"] |= bool(oc[0, 0] == NONE and s.ranges[0] == 7.5)
        ro, og = edge_oracle[i % 24]
        g, info = m.debug_grid(i)
        assert (info.width, info.origin_x) == (w, geom.origin)
        assert np.array_equal(g, og), "item %d: %d window bytes differ" % (i, int((g != og).sum()))
        assert abs(per[i].response - ro["response"]) <= 1e-12
        np.testing.assert_allclose([per[i].best_pose.x, per[i].best_pose.y, per[i].best_pose.euler[-1]], ro["pose"], rtol=0, atol=1e-9)
    assert all(seen.values()), seen
    m.close()


def _same(a, b):
    va = [a.response, a.best_pose.x, a.best_pose.y, a.best_pose.euler[-1]] + list(np.ravel(a.covariance))
    vb = [b.response, b.best_pose.x, b.best_pose.y, b.best_pose.euler[-1]] + list(np.ravel(b.covariance))
    return np.array_equal(np.array(va), np.array(vb), equal_nan=True)


def test_largest_window_item_equals_its_single_call():
    """A query reading beyond the matcher's range threshold makes the window Karto's whole storage: 4073 cells a side under the
    default configuration, the largest coordinates a cell can take."""
    from yag_slam_amd.scan_matching import ScanMatcher
    q, base = cfg2_scans()
    r = np.array(q.ranges)
    r[len(r) // 2] = 25.0
    fq = _mk_native(PlainScan(r, q.min_angle, q.angle_increment, q.min_range, 28.0, (3.0, 3.0, 0.0)))
    nb = [_mk_native(b) for b in base[:3]]
    a, b = ScanMatcher(), ScanMatcher()
    per, _ = a.match_scan_batch(fq, [nb], True, True)
    single = b.match_scan(fq, nb, True, True)
    ga, info = a.debug_grid(0)
    gb, _ = b.debug_grid(0)
    assert info.width == 4073 and info.origin_x == 0
    assert _same(per[0], single)
    assert np.array_equal(ga, gb) and ga.max() == 100
    ca, cb = a.debug_cells(0)[0], b.debug_cells(0)[0]
    assert np.array_equal(ca, cb) and ca[ca[:, 0] != NONE].max() > 2036
    a.close(); b.close()


def test_ragged_and_empty_chains_equal_their_single_calls(geom):
    from yag_slam_amd.scan_matching import ScanMatcher
    nq = _mk_native(_query())
    full = [[_mk_native(s) for s in ch] for ch in _edge_chains(geom, 8)]
    m, ref = ScanMatcher(CFG), ScanMatcher(CFG)
    m.match_scan_batch(nq, full, True, True)  # (real cells in every slot, which a ragged batch's unused slots must not keep)
    # with empty chains (the library answers those items in a call of their own, so the debug readers see only that one: results)
    chains = [full[0], [], full[1][:1], full[2][:2], [], full[3], full[4][1:], full[5][2:]]
    per, _ = m.match_scan_batch(nq, chains, True, True)
    for i, ch in enumerate(chains):
        assert _same(per[i], ref.match_scan(nq, ch, True, True)), i
    # ragged only: results, window bytes, cells, and "no cell" in every slot past a chain's end
    chains = [full[0], full[1][:1], full[2][:2], full[3], full[4][1:], full[5][2:], full[6][:1], full[7]]
    per, _ = m.match_scan_batch(nq, chains, True, True)
    for i, ch in enumerate(chains):
        one = ref.match_scan(nq, ch, True, True)
        assert _same(per[i], one), i
        gm, gr = m.debug_grid(i)[0], ref.debug_grid(0)[0]
        assert np.array_equal(gm, gr), "item %d: %d window bytes differ, first at %s" % (i, int((gm != gr).sum()), np.argwhere(gm != gr)[:3].tolist())
        cb, max_n = m.debug_cells(i)
        cb = cb[:3 * max_n].reshape(3, max_n, 2)
        cs, one_n = ref.debug_cells(0)
        assert one_n == max_n == 257
        for slot in range(3):
            if slot < len(ch):
                assert np.array_equal(cb[slot], cs[slot * one_n:(slot + 1) * one_n]), (i, slot)
            else:
                assert (cb[slot] == NONE).all(), (i, slot)
    m.close(); ref.close()


def test_order_dependent_smear_reads_the_cells_like_the_oracle():
    """smear_deviation = 10 * resolution: the select kernels read every cell and erase the ones Karto's "value already set" rule
    skips"""
    from oracle import oracle as orc
    from yag_slam_amd.scan_matching import ScanMatcher
    cfg = dict(resolution=0.005, smear_deviation=0.05, range_threshold=12.0)
    q, base = cfg2_scans(range_threshold=12.0, n_base=4)
    nq, nb = _mk_native(q), [_mk_native(b) for b in base]
    m, o = ScanMatcher(cfg), orc.Oracle(cfg, "karto")
    plain = [base[:3], base[1:][::-1]]
    per, _ = m.match_scan_batch(nq, [nb[:3], nb[1:][::-1]], True, True)
    for i, ch in enumerate(plain):
        ro = o.match_scan(q, ch, True, True)
        og, _ = o.grid_u8()
        g, info = m.debug_grid(i)
        sub = og[info.origin_y:info.origin_y + info.height, info.origin_x:info.origin_x + info.width]
        assert np.array_equal(g, sub), "item %d: %d window bytes differ" % (i, int((g != sub).sum()))
        assert abs(per[i].response - ro["response"]) <= 1e-12
    m.close()


@pytest.mark.parametrize("semantics", ["karto", "yagpy"])
def test_cache_records_at_their_extreme_values(semantics):
    """A scan of 257 readings matched twice, so that the second call reads the records the first one wrote.  Under the Python
    matcher's rules the first reading has no deciding node (s = -1); under either the last run never closes (t = np = 257)."""
    from tests.util import load_case
    from yag_slam_amd.scan_matching import ScanMatcher
    if semantics == "yagpy":
        c = load_case("small_dirty_rot")
        cfg, q = c["cfg"], c["query"]
        p = q.corrected_pose
        pose = (p.x, p.y, p.euler[-1])
    else:
        cfg, q, pose = CFG, _query(), QPOSE
    r, a0, inc, _ = _ring(257, 0.8, 0.03, 0.2)
    scan = PlainScan(r, a0, inc, 0.05, 6.0, (pose[0] + 0.02, pose[1] - 0.01, pose[2]))
    nq, ns = _mk_native(q), _mk_native(scan)
    m, fresh = ScanMatcher(cfg, semantics=semantics), ScanMatcher(cfg, semantics=semantics)
    fresh.debug_option(7, 1)  # (never caches)
    want = fresh.match_scan(nq, [ns], True, True)
    cw, gw = fresh.debug_cells()[0], fresh.debug_grid()[0]
    assert (cw[:257, 0] != NONE).sum() > 100
    for call in range(2):
        got = m.match_scan(nq, [ns], True, True)
        assert _same(got, want), call
        assert np.array_equal(m.debug_cells()[0], cw), call
        assert np.array_equal(m.debug_grid()[0], gw), call
    # eight chains in one call go through the point cache (a single match projects a scan whose chain structure is known in
    # its own block): the first batch writes the scan's records, the second reads them
    chains = [[ns]] * 8
    pb, _ = fresh.match_scan_batch(nq, chains, True, True)
    cb = [fresh.debug_cells(i)[0] for i in range(8)]
    assert np.array_equal(cb[0][:257], cw[:257])
    hits = []
    for call in range(2):
        pa, _ = m.match_scan_batch(nq, chains, True, True)
        hits.append(m.cache_stats()[0])
        for i in range(8):
            assert _same(pa[i], pb[i]), (call, i)
            assert np.array_equal(m.debug_cells(i)[0], cb[i]), (call, i)
    assert hits[1] > hits[0]
    m.close(); fresh.close()


def test_geometry_beyond_the_coordinate_bound_is_refused():
    """roi_w + border must stay below 32768.  The geometry belongs to the matcher, so every call of such a matcher is refused --
    with the ordinary error, again and again, and without disturbing a matcher just inside the bound."""
    from yag_slam_amd import _capi
    from yag_slam_amd.scan_matching import ScanMatcher
    q = _query()
    r, a0, inc, _ = _ring(17, 0.8, 0.0, 0.0)
    base = PlainScan(r, a0, inc, 0.05, 6.0, QPOSE)
    # resolution 0.005, search 0.5: side 101; range_threshold 82 -> roi_w = 101 + 2 * 16400 = 32901; 81 -> 32501 (+ border 9)
    too_wide = ScanMatcher(dict(resolution=0.005, smear_deviation=0.02, range_threshold=82.0))
    inside = ScanMatcher(dict(resolution=0.005, smear_deviation=0.02, range_threshold=81.0))
    nq, nb = _mk_native(q), [_mk_native(base)]
    for _ in range(2):
        with pytest.raises(_capi.YmError) as e:
            too_wide.match_scan(nq, nb, True, True)
        assert e.value.code == -4 and "32768" in str(e.value)
        with pytest.raises(_capi.YmError):
            too_wide.match_scan_batch(nq, [nb] * 8, True, True)
        ok = inside.match_scan(nq, nb, True, True)
        assert ok.response > 0.0
        _, info = inside.debug_grid()
        assert info.roi_w + info.roi_x == 32501 + 9
        cells = inside.debug_cells()[0]
        assert (cells[:17, 0] != NONE).sum() >= 8
    too_wide.close(); inside.close()
