"""The numpy restatement of the pair-list contract (tests/pairlist_ref.py) is not trusted on its own word: its lookup cells must
reproduce the oracle's integer sums bit for bit, its decoder must invert its encoder, the kernel's reciprocal divide must be the
division, clause (b) of the fitting test must be unreachable by the host's own arithmetic -- and the sparse-scan inputs with which
tests/test_gpu_pair_lists.py reaches bin_kernel's refusal clauses WITHOUT a forcing option are chosen and pinned here, so that a GPU
failure can never be "the input did not do what was meant".  No device code runs in this file."""
import functools

import numpy as np
import pytest

from tests import pairlist_ref as ref
from tests.util import PlainScan, cfg2_scans, load_case


def _oracle():
    from oracle import oracle as orc
    orc.build()
    return orc


def _cfg(over=None):
    from oracle import oracle as orc
    return dict(orc.DEFAULT_CONFIG, **(over or {}))


def karto_problem(cfg_over, query, base):
    """One Karto match on the oracle -> what the restatement needs of it: the sensor-frame points, the grid offset, the angle table
    (ScanMatcher::CorrelateScan: start + k * resolution), the hypothesis cells in the oracle's storage coordinates, the oracle itself."""
    orc = _oracle()
    cfg = _cfg(cfg_over)
    o = orc.Oracle(cfg_over, "karto")
    r = o.match_scan(query, base, True, False)
    assert r["expansions"] == 0, "the input must score above zero: a response expansion would change the angle table"
    nx, ny, nt = r["coarse_dims"]
    p = query.corrected_pose
    off_x, off_y = o.grid_offset()
    grid, info = o.grid_u8()
    res = 1.0 / (1.0 / cfg["resolution"])
    side = int(ref.kt_round_int(cfg["search_size"] / cfg["resolution"])) + 1
    coarse_off, step = 0.5 * (side - 1) * res, 2 * res
    angles = (p.euler[-1] - cfg["coarse_search_angle_offset"]) + np.arange(nt) * cfg["coarse_angle_resolution"]
    ctrig = np.stack([np.cos(angles), np.sin(angles)], axis=1)
    # the oracle's own start cell and lattice: WorldToGrid(centre + (start + i * step)) + the ROI's corner
    hx = ref.kt_round_int(((p.x + (-coarse_off + np.arange(nx) * step)) - off_x) * (1.0 / cfg["resolution"])) + info["roi"][0]
    hy = ref.kt_round_int(((p.y + (-coarse_off + np.arange(ny) * step)) - off_y) * (1.0 / cfg["resolution"])) + info["roi"][1]
    return dict(o=o, r=r, cfg=cfg, ql=o.query_local(), off=(off_x, off_y), ctrig=ctrig, hx=hx, hy=hy, grid=grid, info=info,
                scale=1.0 / cfg["resolution"], dims=(nx, ny, nt))


def _accumulate(grid, cells, hx, hy):
    """sums[k][iy][ix] = sum over the points of grid[hy[iy] + cell_y, hx[ix] + cell_x]"""
    nt = cells.shape[0]
    out = np.zeros((nt, len(hy), len(hx)), dtype=np.uint32)
    for k in range(nt):
        rows = cells[k, :, 1][:, None, None] + hy[None, :, None]
        cols = cells[k, :, 0][:, None, None] + hx[None, None, :]
        assert rows.min() >= 0 and cols.min() >= 0 and rows.max() < grid.shape[0] and cols.max() < grid.shape[1]
        out[k] = grid[rows, cols].sum(axis=0, dtype=np.uint32)
    return out


@pytest.mark.parametrize("beams", [1081, 400])
def test_restated_karto_cells_reproduce_the_oracles_sums(beams):
    q, base = cfg2_scans()
    if beams != 1081:
        q = PlainScan(q.ranges[:beams], q.min_angle, q.angle_increment, q.min_range, 20.0, (3.0, 3.0, 0.0))
    P = karto_problem(None, q, base)
    assert np.array_equal(P["hx"], P["hx"][0] + 2 * np.arange(len(P["hx"]))) and np.array_equal(P["hy"], P["hy"][0] + 2 * np.arange(len(P["hy"])))
    cells = ref.lookup_cells_karto(P["ql"], P["ctrig"], P["off"][0], P["off"][1], P["scale"])
    want = P["o"].sums(0)
    assert want.any()
    assert np.array_equal(_accumulate(P["grid"], cells, P["hx"], P["hy"]), want)


def test_restated_yagpy_cells_reproduce_the_oracles_sums():
    """"yagpy": the reference rounds every (hypothesis, point) pair on its own; on an item whose roundings form a lattice (this
    fixture: the device's guard accepts it, tests/test_gpu_parity.py) hypothesis (0, 0)'s cells + 2 i are the same cells."""
    orc = _oracle()
    c = load_case("sums_cfg2")
    o = orc.Oracle(c["cfg"], "yagpy")
    r = o.match_scan(c["query"], c["base"], c["penalty"], False)
    nx, ny, nt = r["coarse_dims"]
    p = c["query"].corrected_pose
    cfg = _cfg(c["cfg"])
    res, s, ca, car = cfg["resolution"], cfg["search_size"] * 0.5, cfg["coarse_search_angle_offset"] * 0.5, cfg["coarse_angle_resolution"]
    xv, yv, tv = orc.arange(-s + p.x, s + p.x, 2 * res), orc.arange(-s + p.y, s + p.y, 2 * res), orc.arange(-ca + p.euler[-1], ca + p.euler[-1], car)
    assert (len(xv), len(yv), len(tv)) == (nx, ny, nt)
    off_x, off_y = o.grid_offset()
    grid, info = o.grid_u8()
    assert info["roi"][0] == 0 and info["roi"][1] == 0
    ctrig = np.stack([np.cos(tv), np.sin(tv)], axis=1)
    cells = ref.lookup_cells_yagpy(o.query_local(), ctrig, off_x, off_y, (xv[0], yv[0]), res, 0)
    want = o.sums(0)
    assert want.any()
    assert np.array_equal(_accumulate(grid, cells, 2 * np.arange(nx), 2 * np.arange(ny)), want)
    # and the z file's volume is the reference's own
    assert np.array_equal(want.astype(np.int64), c["z"]["coarse_sums"])


@pytest.mark.parametrize("rg_h", ref.HEIGHTS)
def test_decode_is_the_inverse_of_encode(rg_h):
    rng = np.random.default_rng(rg_h)
    rg_cls = ref.RG_PITCH * (rg_h + 26)
    nrx, nry = 64, (4096 + rg_h - 1) // rg_h
    X = rng.integers(0, 2 * ref.RG_W * nrx, size=20000)
    Y = rng.integers(0, 8192, size=20000)
    # the last class row below 4096, both row parities, every column class; the first and last row and byte of a region
    X[:8], Y[:8] = [0, 1, 126, 127, 128, 129, 8190, 8191], [8190, 8191, 8190, 8191, 8190, 8191, 8190, 8191]
    Y[8:12] = [2 * rg_h - 2, 2 * rg_h - 1, 2 * rg_h, 2 * rg_h + 1]
    valid, region, entry, er, ex = ref.encode(X, Y, rg_h, rg_cls, nrx, nry)
    assert valid.all()
    assert entry.max() < 4 * rg_cls <= 65535 - 3 and (er < rg_h).all() and (ex < ref.RG_W).all()
    assert np.array_equal(entry & 3, ex & 3), "class images and rows are multiples of four bytes: the misalignment is the byte's"
    X2, Y2, er2, ex2 = ref.decode(entry, region, rg_h, rg_cls, nrx)
    assert np.array_equal(X2, X) and np.array_equal(Y2, Y) and np.array_equal(er2, er) and np.array_equal(ex2, ex)
    # outside: negative cells, class rows from 4096 on, regions beyond the last
    valid, *_ = ref.encode([-1, 0, 0, 2 * ref.RG_W * nrx], [0, -1, 8192, 0], rg_h, rg_cls, nrx, nry)
    assert not valid.any()


@pytest.mark.parametrize("rg_h", ref.HEIGHTS)
def test_the_reciprocal_multiply_is_the_division(rg_h):
    """region_entry: ry = (yc * ceil(2^21 / rg_h)) >> 21 for every class row below 4096 (the kernel's comment proves it; this states it).
    The kernel multiplies with v_mul_u32_u24: both operands must fit 24 bits and the product 32."""
    yc = np.arange(4096, dtype=np.int64)
    mul = ((1 << 21) + rg_h - 1) // rg_h
    assert mul < (1 << 24) and int(yc.max()) * mul < (1 << 32)
    assert np.array_equal((yc * mul) >> 21, yc // rg_h)


def test_clause_b_is_a_belt():
    """bin_kernel's `pos0 + all <= 65532` cannot refuse: pos0 = part * entries_pstride and all <= entries_pstride (the clause before
    it), so the largest position is lparts * entries_pstride, with entries_pstride = min(28672, ceil64(lnw * max_n * 11 / 10)) and
    lparts = ceil(nt / lnw).  Over every (nt, max_n) the host admits to the region correlate (nt * max_n <= 28672, max_n < 2048,
    nt <= 256) and every lnw it can choose (nt itself up to 8 angles, else 8; debug option 15: 4 .. 8, 10, 11, 16) the product
    stays below 65532: three parts or more mean lnw * max_n <= 8 / 17 * 28672 at the worst."""
    worst = (0, None)
    n = np.arange(1, 2048, dtype=np.int64)
    for nt in range(1, 257):
        ok = n[nt * n <= ref.RG_MAX_ENTRIES]
        if len(ok) == 0:
            continue
        for lnw in sorted({nt if nt <= 8 else 8, 4, 5, 6, 7, 8, 10, 11, 16}):
            lparts = (nt + lnw - 1) // lnw
            pstride = np.minimum(ref.RG_MAX_ENTRIES, (lnw * ok * 11 // 10 + 63) // 64 * 64)
            top = int((lparts * pstride).max())
            if top > worst[0]:
                worst = (top, (nt, lnw, int(ok[np.argmax(lparts * pstride)])))
    assert worst[0] < ref.RG_LAST_POS, worst
    assert worst[0] == 2 * ref.RG_MAX_ENTRIES, worst  # (two parts of the largest list: 57344)


def test_split_bin_accepts_what_the_contract_allows_and_nothing_else():
    Z = 42400
    good = [[], [4, 8, 5, 9], [4, Z, 5, Z + 1], [4, 8, Z, Z], [4, Z, 6, Z + 2, 7, Z + 3, Z, Z], [5, Z + 1, Z, Z], [7, 11, 15, Z + 3]]
    for e in good:
        real, err = ref.split_bin(e, Z)
        assert err is None, (e, err)
        assert sorted(real.tolist()) == sorted(x for x in e if x < Z)
    bad = [[4, 5, 6, 7],            # odd runs without their padding
           [5, Z, Z, Z],            # rg_zero where rg_zero + 1 belongs
           [5, 4, Z, Z + 1],        # runs out of order
           [4, 8, Z, Z, Z, Z, Z, Z],  # more than one pair at the end
           [Z, Z, 4, 8],            # padding before the entries
           [4, 8, 12, Z, Z, Z]]     # length no multiple of four
    for e in bad:
        assert ref.split_bin(e, Z)[1] is not None, e


# ---- the inputs of tests/test_gpu_pair_lists.py that reach the refusal clauses on real counts ------------------------------------------------
# A sparse scan: `beams` readings over 270 degrees of which `valid` (a seeded choice) lie inside [lo, hi) metres, the others beyond the
# scan's own threshold; the query at (3, 3, 0).  The host sizes a part's share of the entry buffer by the scan's LENGTH (+ 10 %), the
# sets of 16-bit sums likewise (+ 15 %): a full-length scan whose points are scattered pads its bins beyond both, a long scan with few
# valid readings has room to spare and trips the region count alone.
SPARSE = {
    # name: (seed, beams, valid, lo, hi, config)
    "pad_mixed": (11, 1081, 1081, 0.5, 5.0, None),     # the 10 % allowance: two parts of eight angles refused, the part of five listed
    "angle_alone": (11, 1081, 1081, 0.5, 8.0, None),   # every part refused; the part of five angles by an angle's total ALONE
    "regions": (13, 1365, 400, 0.5, 12.0, None),       # more than 96 regions with work, nothing else: a 2561-cell window of 357 regions
    "regions_edge": (48, 1365, 400, 0.5, 8.0, None),   # exactly 96 regions with work in one part: listed, on the boundary of `<=`
}
# what the restatement says of them (default lattice 26 x 26 x 21: parts of 8, 8 and 5 angles); refused = indices into ref.CLAUSES
EXPECT = {
    'pad_mixed': dict(nq=1081, win_w=1153, nregions=80, entries_pstride=9536, angle_room=1304, region26=True, lost=0,
        parts=[
            dict(pairs=8648, total=9636, angle_max=1208, regions_used=46, refused=[0]),
            dict(pairs=8648, total=9644, angle_max=1220, regions_used=45, refused=[0]),
            dict(pairs=5405, total=6052, angle_max=1224, regions_used=46, refused=[]),
        ]),
    'angle_alone': dict(nq=1081, win_w=1665, nregions=154, entries_pstride=9536, angle_room=1304, region26=True, lost=0,
        parts=[
            dict(pairs=8648, total=10664, angle_max=1348, regions_used=96, refused=[0, 2]),
            dict(pairs=8648, total=10688, angle_max=1364, regions_used=94, refused=[0, 2]),
            dict(pairs=5405, total=6732, angle_max=1360, regions_used=94, refused=[2]),
        ]),
    'regions': dict(nq=400, win_w=2561, nregions=357, entries_pstride=12032, angle_room=1956, region26=True, lost=0,
        parts=[
            dict(pairs=3200, total=6292, angle_max=808, regions_used=181, refused=[3]),
            dict(pairs=3200, total=6272, angle_max=804, regions_used=185, refused=[3]),
            dict(pairs=2000, total=3900, angle_max=792, regions_used=167, refused=[3]),
        ]),
    'regions_edge': dict(nq=400, win_w=1665, nregions=154, entries_pstride=12032, angle_room=1956, region26=True, lost=0,
        parts=[
            dict(pairs=3200, total=5020, angle_max=640, regions_used=92, refused=[]),
            dict(pairs=3200, total=4980, angle_max=636, regions_used=96, refused=[]),
            dict(pairs=2000, total=3140, angle_max=656, regions_used=88, refused=[]),
        ]),
}


def sparse_scan(name, pose=(3.0, 3.0, 0.0)):
    from yag_slam_amd import synth
    seed, beams, valid, lo, hi, _ = SPARSE[name]
    rng = np.random.default_rng(seed)
    ranges = np.full(beams, 25.0)
    idx = np.sort(rng.choice(beams, size=valid, replace=False))
    ranges[idx] = rng.uniform(lo, hi, size=valid)
    inc = (synth.MAX_ANGLE - synth.MIN_ANGLE) / (beams - 1)
    return PlainScan(ranges, synth.MIN_ANGLE, inc, synth.MIN_RANGE, 20.0, pose)


def sparse_base(name):
    """a chain the sparse query scores on: its own readings seen from three poses nearby"""
    return [sparse_scan(name, pose) for pose in ((3.02, 2.99, 0.003), (2.98, 3.01, -0.004), (3.0, 3.03, 0.0))]


def named_query(name):
    """the queries of the GPU tests by name: the synthetic room's scan ("cfg2"), its first 707 / 400 beams, or a sparse scan"""
    if name.startswith("cfg2"):
        q, _ = cfg2_scans()
        n = int(name[5:]) if len(name) > 4 else len(q.ranges)
        return PlainScan(q.ranges[:n], q.min_angle, q.angle_increment, q.min_range, 20.0, (3.0, 3.0, 0.0))
    return sparse_scan(name)


def named_base(name):
    return cfg2_scans()[1][:3] if name.startswith("cfg2") else sparse_base(name)


def reach(q):
    """the largest reading Karto keeps: what sizes the call's window"""
    return float(q.ranges[(q.ranges >= q.min_range) & (q.ranges <= q.range_threshold)].max())


def prediction(name, cfg_over=None, rq=None, max_n=None):
    """-> (geometry the host must plan, the restatement's prediction, the oracle problem) for the named query in a call whose
    window is sized for a reach of rq metres and whose longest scan has max_n readings (default: the query's own)"""
    q, base = named_query(name), named_base(name)
    P = karto_problem(cfg_over, q, base)
    nx, ny, nt = P["dims"]
    g = ref.plan_geometry(P["cfg"], reach(q) if rq is None else rq, len(q.ranges) if max_n is None else max_n, nx, ny, nt)
    cells = ref.lookup_cells_karto(P["ql"], P["ctrig"], P["off"][0], P["off"][1], P["scale"])
    # the first hypothesis cell in WINDOW coordinates: storage cell - window origin
    cx0, cy0 = int(P["hx"][0]) - g["origin"], int(P["hy"][0]) - g["origin"]
    return g, ref.predict(cells, cx0, cy0, g), P


@functools.lru_cache(maxsize=None)
def sparse_prediction(name):
    return prediction(name, SPARSE[name][5])


# one match_pairs call of distinct queries, some of whose lists fit and some not: the window is the widest query's (8 m), for all of them
ACROSS = ("cfg2", "angle_alone", "cfg2_400", "pad_mixed")
EXPECT_ACROSS = {"cfg2": [[], [], []], "angle_alone": [[0, 2], [0, 2], [2]], "cfg2_400": [[], [], []], "pad_mixed": [[0], [0], []]}


@functools.lru_cache(maxsize=None)
def across_prediction():
    rq = max(reach(named_query(n)) for n in ACROSS)
    max_n = max(len(named_query(n).ranges) for n in ACROSS)
    return {n: prediction(n, None, rq, max_n) for n in ACROSS}


def test_the_mixed_call_holds_listed_and_refused_queries():
    got = {n: [p["refused"] for p in pred["parts"]] for n, (g, pred, P) in across_prediction().items()}
    assert got == EXPECT_ACROSS
    assert any(all(not r for r in parts) for parts in got.values()) and any(all(r for r in parts) for parts in got.values())


def summarize(name):
    g, pred, P = sparse_prediction(name)
    return dict(nq=len(P["ql"]), win_w=g["win_w"], nregions=g["nregions"], entries_pstride=g["entries_pstride"], angle_room=g["ng"] * ref.RG_FLUSH,
                region26=g["region26"], lost=pred["lost"],
                parts=[dict(pairs=p["pairs"], total=p["total"], angle_max=int(p["angle_tot"].max()), regions_used=p["regions_used"], refused=p["refused"])
                       for p in pred["parts"]])


@pytest.mark.parametrize("name", sorted(SPARSE))
def test_the_refusal_inputs_do_what_they_are_meant_to(name):
    got = summarize(name)
    assert got["region26"] and got["lost"] == 0
    assert got == EXPECT[name]
