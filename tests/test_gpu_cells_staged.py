"""Batches turn a cached base scan into an item's cells with the scan's points staged in LDS (cells_kernel<true>: one round of
loads for a group of five chunks of 256 readings, one barrier, the deciding pair of every reading from LDS) while the call's
longest scan has at most 1440 readings, and with the register path (cells_kernel<false>) beyond.  What the staging can get
wrong: a chunk's or a group's first and last reading, a scan shorter than the LDS the call allocates, the block-uniform exits,
deciding pairs that do not exist (s = -1, t = np), a deciding line through the end point (ss == 0, where Karto keeps the
reading and the Python matcher drops it), cleared slots beside filled ones.  Batches of 8 items -- the smallest that take
the batch path -- with ragged chains; cells against the oracle's own pieces (point readings, valid-point filter,
WorldToGrid), window bytes against the oracle's grid, bit for bit; the call twice on one matcher (the first fills the point
cache, the second reads it) and every item against its single call on a matcher that never caches (the fused path)."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from tests.util import PlainScan  # noqa: E402

NONE = np.iinfo(np.int32).min
RES = 0.01
CFG = dict(range_threshold=6.0, resolution=RES, use_response_expansion=False)  # (no expansion: an empty item stays in its call)
QPOSE = (3.0, 3.0, 0.0)
CHUNK, GROUP, STAGED_MAX = 256, 5 * 256, 1440  # ym_k_prepare.hpp: NT, YM_CELLS_GROUP * NT, YM_CELLS_STAGED_MAX_N
MAX_BASE = 4


def _mk_native(plain):
    from yag_slam_amd.models import LocalizedRangeScan
    p = plain.corrected_pose
    return LocalizedRangeScan(plain.ranges, plain.min_angle, plain.max_angle, plain.angle_increment,
                              plain.min_range, plain.max_range, plain.range_threshold, p.x, p.y, p.euler[-1])


def _ring(n, variant):
    """n readings over the full circle, 0.8 m (with a wobble) around a sensor that is a few cells off the query (even variants:
    the query looks at the ring from inside and nearly every reading is kept) or 1.4 m away (odd variants: the query sees the
    near half of the ring from behind, and which readings it keeps depends on every reading's own deciding pair)"""
    per = max(n, 2)
    k = np.arange(n)
    r = 0.8 + 0.03 * np.sin(5 * (2 * np.pi * k / per) + 0.7 * variant)
    far = (1.3, 0.45) if variant % 2 else (0.0, 0.0)
    return PlainScan(r, -np.pi, 2 * np.pi / per, 0.05, 6.0,
                     (QPOSE[0] + far[0] + 0.03 * (variant % 5), QPOSE[1] + far[1] - 0.02 * (variant % 7), 0.3 * variant))


def _collinear():
    """Reading 0 has range 0 (the sensor itself, whatever its beam's angle), reading 1 lies on the beam of angle exactly 0; the
    sensor is half a metre left of the viewpoint at the same height, so the viewpoint, reading 0 and reading 1 lie on one
    horizontal line in exact arithmetic: every product and sum of the side test is exact and ss == 0.  Reading 0 opens the
    trigger chain and reading 1 (0.8 m on) closes its run: Karto decides reading 0 by the pair (0, 1) and keeps it (!(ss < 0)),
    the Python matcher decides reading 1 by it and drops it (ss > 0 fails)."""
    n = 257
    inc = 2 * np.pi / 256
    r = 0.8 + 0.02 * np.cos(np.arange(n) * 0.37)
    r[0], r[1] = 0.0, 0.8
    return PlainScan(r, -(1 * inc), inc, 0.0, 6.0, (QPOSE[0] - 0.5, QPOSE[1], 0.0))


def _pool(longest):
    lengths = [1, 15, 16, 17, CHUNK - 1, CHUNK, CHUNK + 1, 1081, GROUP - 1, GROUP, GROUP + 1, longest]
    pool = [_ring(n, v) for v, n in enumerate(lengths)]
    pool.append(PlainScan(np.full(33, 9.0), -1.0, 0.06, 0.05, 6.0, (QPOSE[0], QPOSE[1] + 0.1, 0.0)))  # 12: no reading is valid
    pool.append(_collinear())                                                                          # 13
    return pool


# scans of the pool per item: 0 to MAX_BASE of them, every length beside every other, the longest scan first and last
CHAINS = [[11, 0, 12, 7], [], [8, 9, 10], [4, 5, 6, 13], [12], [1, 2, 3, 11], [13, 7], [10, 0, 9, 5]]


def _query():
    per = 256
    k = np.arange(257)
    return PlainScan(1.0 + 0.05 * np.sin(5 * (2 * np.pi * k / per) + 0.3), -np.pi, 2 * np.pi / per, 0.05, 6.0, QPOSE)


def _kt_round(v):
    r = np.floor(np.abs(v) + 0.5).astype(np.int64)
    return np.where(v < 0.0, -r, r)


def _oracle_cells(scan, semantics, info):
    """the oracle's cells of one base scan in the window `info` describes: its point readings, the valid-point filter seen
    from the query, WorldToGrid (Karto) or the Python matcher's rounding"""
    from oracle import oracle as orc
    p = scan.corrected_pose
    xs, ys = orc.point_readings(scan.ranges, scan.min_angle, scan.angle_increment, scan.min_range, scan.range_threshold,
                                (p.x, p.y, p.euler[-1]), semantics)
    keep = orc.valid_points(xs, ys, QPOSE[0], QPOSE[1], semantics)
    off = [QPOSE[i] - (0.5 * (info.roi_w - 1) * RES) for i in (0, 1)]
    assert (info.offset_x, info.offset_y) == tuple(off)
    if semantics == "karto":
        scale = 1.0 / RES
        gx, gy = _kt_round((xs - off[0]) * scale), _kt_round((ys - off[1]) * scale)
    else:
        gx, gy = np.rint((xs - off[0]) / RES).astype(np.int64), np.rint((ys - off[1]) / RES).astype(np.int64)
    keep = keep & (gx >= 0) & (gx < info.roi_w) & (gy >= 0) & (gy < info.roi_w)
    out = np.full((len(xs), 2), NONE, dtype=np.int64)
    out[keep, 0] = gx[keep] + info.roi_x - info.origin_x
    out[keep, 1] = gy[keep] + info.roi_x - info.origin_x
    return out, keep


def _oracle_window(o, semantics, info):
    if semantics == "karto":
        og, oinfo = o.grid_u8()
        assert info.storage_w == oinfo["width"]
    else:
        og = (100 * o.grid_f64()).astype(np.int64).astype(np.uint8)
        assert info.storage_w == og.shape[0]
    return og[info.origin_y:info.origin_y + info.height, info.origin_x:info.origin_x + info.width]


def _same(a, b):
    va = [a.response, a.best_pose.x, a.best_pose.y, a.best_pose.euler[-1]] + list(np.ravel(a.covariance))
    vb = [b.response, b.best_pose.x, b.best_pose.y, b.best_pose.euler[-1]] + list(np.ravel(b.covariance))
    return np.array_equal(np.array(va), np.array(vb), equal_nan=True)


def test_the_side_test_is_exactly_zero_on_the_collinear_scan():
    """the inputs of the ss == 0 case are what they claim to be, by the oracle's own point readings and filter"""
    from oracle import oracle as orc
    s = _collinear()
    p = s.corrected_pose
    for sem, reading, kept in (("karto", 0, True), ("yagpy", 1, False)):
        xs, ys = orc.point_readings(s.ranges, s.min_angle, s.angle_increment, s.min_range, s.range_threshold, (p.x, p.y, 0.0), sem)
        assert len(xs) == 257 and (xs[0], ys[0]) == (2.5, 3.0) and (xs[1], ys[1]) == (2.5 + 0.8, 3.0)
        fx, fy, cx, cy, vpx, vpy = xs[0], ys[0], xs[1], ys[1], QPOSE[0], QPOSE[1]
        assert cx * (vpy - fy) + cy * (fx - vpx) + (fy * vpx - fx * vpy) == 0.0
        assert bool(orc.valid_points(xs, ys, vpx, vpy, sem)[reading]) is kept


@pytest.mark.parametrize("tile_lists", [False, True])
@pytest.mark.parametrize("longest", [STAGED_MAX, STAGED_MAX + 1])
@pytest.mark.parametrize("semantics", ["karto", "yagpy"])
def test_ragged_batch_of_every_length_against_the_oracle(semantics, longest, tile_lists):
    """longest = 1440: the longest scan that is staged in LDS (every shorter scan of the call leaves part of it unused);
    1441: the first call that takes the register path.  tile_lists: the raster's work lists and hit slots from 8 items on
    (they are built from the chunk boxes, which have no read-back of their own), with 2 hit slots per tile so that most
    tiles are reached by more chunks than fit."""
    from oracle import oracle as orc
    from yag_slam_amd.scan_matching import ScanMatcher
    pool = _pool(longest)
    native = [_mk_native(s) for s in pool]
    q, nq = _query(), _mk_native(_query())
    chains = [[native[j] for j in ch] for ch in CHAINS]
    m, fresh = ScanMatcher(CFG, semantics=semantics), ScanMatcher(CFG, semantics=semantics)
    fresh.debug_option(7, 1)  # (never caches: a single match projects its scans in the fused kernel)
    if tile_lists:
        m.debug_option(40, 8)
        m.debug_option(18, 2)
    o = orc.Oracle(CFG, semantics)
    want = []
    seen = dict(kept=0, dropped=0, s_none=False, collinear=False)
    hits = []
    for call in range(2):
        per, _ = m.match_scan_batch(nq, chains, True, True)
        hits.append(m.cache_stats()[0])
        for i, ch in enumerate(CHAINS):
            cells, max_n = m.debug_cells(i)
            assert max_n == longest
            cells = cells[:MAX_BASE * max_n].reshape(MAX_BASE, max_n, 2)
            g, info = m.debug_grid(i)
            if call == 0:
                ro = o.match_scan(q, [pool[j] for j in ch], True, True)
                exp = np.full((MAX_BASE, max_n, 2), NONE, dtype=np.int64)
                for slot, j in enumerate(ch):
                    oc, keep = _oracle_cells(pool[j], semantics, info)
                    exp[slot, :len(oc)] = oc
                    seen["kept"] += int(keep.sum())
                    seen["dropped"] += int((~keep).sum())
                    if j == 13:
                        seen["collinear"] |= bool(keep[0]) if semantics == "karto" else not bool(keep[1])
                    if semantics == "yagpy" and len(keep):
                        seen["s_none"] |= not bool(keep[0])  # (point 0 has no deciding node there: never kept)
                want.append((ro, exp, _oracle_window(o, semantics, info).copy()))
            ro, exp, win = want[i]
            assert np.array_equal(cells, exp), (call, i, np.argwhere(cells != exp)[:4].tolist())
            assert np.array_equal(g, win), "call %d item %d: %d window bytes differ" % (call, i, int((g != win).sum()))
            assert abs(per[i].response - ro["response"]) <= 1e-12, (call, i)
            if call == 0:  # the single call: the fused kernel, nothing cached
                one = fresh.match_scan(nq, chains[i], True, True)
                assert _same(per[i], one), i
                cs, one_n = fresh.debug_cells(0)
                n1 = max([len(pool[j].ranges) for j in ch] + [len(q.ranges)])
                assert one_n == n1
                for slot in range(len(ch)):
                    assert np.array_equal(cs[slot * n1:(slot + 1) * n1], exp[slot, :n1]), (i, slot)
                    assert (exp[slot, n1:] == NONE).all()
                assert np.array_equal(fresh.debug_grid(0)[0], g), i
    assert hits[1] > hits[0]
    assert seen["kept"] > 4000 and seen["dropped"] > 2000 and seen["collinear"], seen
    assert semantics == "karto" or seen["s_none"]
    m.close(); fresh.close()


def test_tile_lists_beyond_what_a_thread_keeps():
    """tiles_kernel keeps a thread's first three chunk boxes in registers between its two passes and loads the tile_zero bytes
    of its first two tiles with them; what lies beyond is read as before.  Item 0 has 9 scans of 1440 readings = 810 boxes, more
    than 3 x 256; a query reading beyond the matcher's range makes the window the whole storage (1273 cells a side) and option 2
    launches all its 20 x 40 tiles, more than 2 x 256; with 2 hit slots per tile most tiles are reached by more chunks than fit.
    The second call moves every chain three items on: tiles that were stamped and are not reached now are listed for clearing
    only.  Window bytes of every item of both calls against the oracle's grid."""
    from oracle import oracle as orc
    from yag_slam_amd.scan_matching import ScanMatcher
    q = _query()
    r = np.array(q.ranges)
    r[128] = 7.0
    q = PlainScan(r, q.min_angle, q.angle_increment, 0.05, 8.0, QPOSE)
    long9 = [_ring(STAGED_MAX, v) for v in range(9)]
    short = [_ring(n, v) for v, n in enumerate([1081, 257, 17, CHUNK, GROUP + 1, 16])]
    plain = [long9, short[:1], short[1:4], [], short[3:], long9[:4], short[::-1], long9[4:] + short[:2]]
    cache = {}

    def nat(s):
        return cache.setdefault(id(s), _mk_native(s))
    nq = _mk_native(q)
    m, o = ScanMatcher(CFG), orc.Oracle(CFG, "karto")
    for option, value in ((40, 8), (18, 2), (2, 1)):
        m.debug_option(option, value)
    for call in range(2):
        chains = plain[-3 * call:] + plain[:-3 * call] if call else plain
        per, _ = m.match_scan_batch(nq, [[nat(s) for s in ch] for ch in chains], True, True)
        for i, ch in enumerate(chains):
            ro = o.match_scan(q, ch, True, True)
            g, info = m.debug_grid(i)
            assert info.width == info.storage_w == 1273 and m.debug_cells(i)[1] == STAGED_MAX
            win = _oracle_window(o, "karto", info)
            assert np.array_equal(g, win), "call %d item %d: %d window bytes differ" % (call, i, int((g != win).sum()))
            assert abs(per[i].response - ro["response"]) <= 1e-12, (call, i)
    m.close()
