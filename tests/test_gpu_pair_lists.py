"""The region correlate's pair lists themselves (bin_kernel, yag_slam_amd/csrc/ym_k_region.hpp), read back through
ym_debug_pair_lists and held against the numpy restatement of their contract (tests/pairlist_ref.py; DESIGN.md section 4, "The
pair-list contract") -- and bin_kernel's refusal clauses on REAL counts: sparse scans (tests/test_pairlist_host.py chooses and pins
them on the CPU) whose padded lists do not fit, with no forcing option, in calls where one angle block of an item is listed and
another refused, and where some queries are listed and others not.

Every call is a batch of 8 or 9 items with option 28 = 8 (the LDS correlates from 8 items on) and must have taken
correlate_region_kernel.  Every comparison is integer (or bit) equality."""
import ctypes as C
import functools

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from tests import pairlist_ref as ref  # noqa: E402
from tests import test_pairlist_host as host  # noqa: E402
from tests.util import PlainScan, cfg2_scans, load_case  # noqa: E402

REGION = "correlate_region_kernel"
GEOMETRY_KEYS = ("nt", "lnw", "lparts", "nbins", "nrx", "nry", "nregions", "rg_h", "rg_cls", "rg_zero", "ng", "entries_pstride")


def _native(plain):
    from yag_slam_amd.models import LocalizedRangeScan
    p = plain.corrected_pose
    return LocalizedRangeScan(plain.ranges, plain.min_angle, plain.max_angle, plain.angle_increment,
                              plain.min_range, plain.max_range, plain.range_threshold, p.x, p.y, p.euler[-1])


def _matcher(cfg=None, semantics="karto", opts=None):
    from yag_slam_amd.scan_matching import ScanMatcher
    m = ScanMatcher(cfg, semantics=semantics)
    m.debug_option(28, 8)
    m.debug_option(12, 1)  # keep the integer sums of batches
    for k, v in (opts or {}).items():
        m.debug_option(k, v)
    return m


def _window_origin(m, item):
    from yag_slam_amd import _capi
    info = _capi.YmGridInfo()
    _capi.check(m._lib.ym_debug_grid_info(m._m, int(item), C.byref(info)))
    return int(info.origin_x)


def _room_scan(beams, pose=(3.0, 3.0, 0.0)):
    """the synthetic room seen through a sensor of `beams` readings over the same 270 degrees"""
    from yag_slam_amd import synth
    inc = (synth.MAX_ANGLE - synth.MIN_ANGLE) / (beams - 1)
    r = synth.Scene().scan_ranges((3.07, 3.04, 0.05), index=10, n_beams=beams, inc=inc)
    return PlainScan(r, synth.MIN_ANGLE, inc, synth.MIN_RANGE, 20.0, pose)


def _chains(nb):
    return [nb, nb[:3], nb[2:9], nb[::-1], nb[4:5], nb[1:], nb[:7], nb[3:], nb[5:6]]


def _read_slots(m, cfg, yag=False):
    """every query slot of the matcher's last call: the lists, what the builder read, and what the restatement makes of that"""
    from oracle import oracle as orc
    full = dict(orc.DEFAULT_CONFIG, **(cfg or {}))
    slots, n = [], 1
    s = 0
    while s < n:
        L = m.debug_pair_lists(s)
        n = L["n_slots"]
        ql = m.debug_query_local(item=L["qrep"])
        assert len(ql) == L["nq"]
        if yag:
            cells = ref.lookup_cells_yagpy(ql, L["ctrig"], L["off_x"], L["off_y"], L["ylat"], full["resolution"], _window_origin(m, L["qrep"]))
        else:
            cells = ref.lookup_cells_karto(ql, L["ctrig"], L["off_x"], L["off_y"], 1.0 / full["resolution"])
        pred = ref.predict(cells, L["cx0"], L["cy0"], L)
        flat = L["entries"].reshape(-1).astype(np.int64)
        parts = []
        for p in range(L["lparts"]):
            if L["flags"][p] < 0:
                parts.append(None)
                continue
            st = L["starts"][p].astype(np.int64)
            ok = bool(st.min() >= 0 and st.max() <= flat.size and (np.diff(st) >= 0).all())
            raw = {int(b): flat[st[b]:st[b + 1]] for b in np.nonzero(np.diff(st))[0]} if ok else {}
            parts.append(dict(starts=st, in_range=ok, raw=raw, split={b: ref.split_bin(e, L["rg_zero"]) for b, e in raw.items()}))
        slots.append(dict(L=L, pred=pred, parts=parts))
        s += 1
    return slots


# ---- the contract, on inputs whose lists all fit ------------------------------------------------------------------------------------------
FEWER_ANGLES = {"coarse_search_angle_offset": 6 * 0.0349}  # 13 coarse angles: 13 x 2047 pairs still fit the region correlate's buffers
NO_EXPANSION = {"use_response_expansion": False}  # (a query without readings scores zero: its expansion would be the matcher's last call)
CONTRACT = {
    # name: (config, queries, what it reaches)
    "beams_1081": (None, ("cfg2",)),
    "beams_707": (None, ("cfg2_707",)),            # a set of 16-bit sums written out mid-way
    "beams_400": (None, ("cfg2_400",)),
    "lattice_13": ({"search_size": 0.24}, ("cfg2",)),  # one lane per lattice row
    "beams_1200": (None, ("room_1200",)),          # above 1152 readings: bin_kernel's MAXP = 32 instantiation
    "beams_2047": (FEWER_ANGLES, ("room_2047",)),  # the 11-bit rank's last value
    "yagpy": (None, ("sums_cfg2",)),               # YAG = true, a fixture the lattice guard accepts
    "regions_96": (None, ("regions_edge",)),       # a sparse scan with exactly 96 regions with work in one part: the last count that is listed
    "pairs": (NO_EXPANSION, ("cfg2", "cfg2_707", "one", "cfg2_400", "none", "room_1000", "cfg2_100", "cfg2_1000", "cfg2_33")),
}


def _query(name):
    if name.startswith("room_"):
        return _room_scan(int(name[5:]))
    if name in ("one", "none"):  # one valid reading / none: the others lie beyond the scan's threshold
        q = host.named_query("cfg2")
        r = np.full(len(q.ranges), 25.0)
        if name == "one":
            r[540] = q.ranges[540]
        return PlainScan(r, q.min_angle, q.angle_increment, q.min_range, 20.0, (3.0, 3.0, 0.0))
    return host.named_query(name)


@functools.lru_cache(maxsize=None)
def _contract(name):
    cfg, queries = CONTRACT[name]
    yag = name == "yagpy"
    if yag:
        c = load_case("sums_cfg2")
        cfg = c["cfg"]
        m = _matcher(cfg, "yagpy")
        base = [_native(b) for b in c["base"]]
        per, _ = m.match_scan_batch(_native(c["query"]), [base] * 7 + [base[:2]] + [base], c["penalty"], c["do_fine"])
        cnt = m.debug_counters()
        assert (cnt["yag_fast_items"], cnt["yag_fallback_items"]) == (9, 0)
        plain, max_n = [c["query"]], None
    else:
        m = _matcher(cfg)
        # (a sparse query scores on its own readings seen from nearby, not on the room: no response expansion may follow the call)
        base_plain = host.named_base(queries[0]) * 3 if queries[0] in host.SPARSE else cfg2_scans()[1]
        nb = [_native(b) for b in base_plain]
        plain = [_query(n) for n in queries]
        max_n = max(len(s.ranges) for s in plain + base_plain)
        if len(plain) == 1:
            per, _ = m.match_scan_batch(_native(plain[0]), _chains(nb), True, True)
            assert all(r.meta["expansions"] == 0 for r in per)
        else:
            per = m.match_pairs([_native(q) for q in plain], _chains(nb), True, True)
    assert m.debug_counters()["last_correlate"] == REGION
    slots = _read_slots(m, cfg, yag)
    assert len(slots) == len(plain)
    m.close()
    return dict(slots=slots, cfg=cfg, plain=plain, yag=yag, dims=per[0].meta["coarse_dims"], max_n=max_n)


def _listed(name):
    run = _contract(name)
    for s, slot in enumerate(run["slots"]):
        for p, part in enumerate(slot["parts"]):
            assert part is not None, "slot %d part %d has no list: these inputs fit" % (s, p)
            yield s, p, slot["L"], slot["pred"], part


@pytest.mark.parametrize("name", sorted(n for n in CONTRACT if n != "yagpy"))  # (plan_geometry restates the Karto window only)
def test_contract_geometry_is_what_the_host_plans(name):
    run = _contract(name)
    from oracle import oracle as orc
    nx, ny, nt = run["dims"]
    g = ref.plan_geometry(dict(orc.DEFAULT_CONFIG, **(run["cfg"] or {})), max(host.reach(q) for q in run["plain"] if (q.ranges <= 20.0).any()),
                          run["max_n"], nx, ny, nt, n_items=9)
    assert g["region26"]
    for slot in run["slots"]:
        assert {k: slot["L"][k] for k in GEOMETRY_KEYS} == {k: g[k] for k in GEOMETRY_KEYS}


@pytest.mark.parametrize("name", sorted(CONTRACT))
def test_contract_starts(name):
    """1: starts is non-decreasing, begins at the part's share of the buffer, spans the flag, every bin a multiple of four"""
    for s, p, L, pred, part in _listed(name):
        st = part["starts"]
        assert part["in_range"], (s, p)
        assert st[0] == p * L["entries_pstride"], (s, p)
        assert st[-1] - st[0] == L["flags"][p] <= L["entries_pstride"], (s, p)
        assert not (np.diff(st) % 4).any(), (s, p)


@pytest.mark.parametrize("name", sorted(CONTRACT))
def test_contract_runs_and_padding(name):
    """2: inside a bin the runs come in misalignment order, each is even, padding sits only where the contract allows it"""
    for s, p, L, pred, part in _listed(name):
        for b, (real, err) in part["split"].items():
            assert err is None, "slot %d part %d bin %d (region %d angle %d): %s" % (s, p, b, b // L["lnw"], p * L["lnw"] + b % L["lnw"], err)


@pytest.mark.parametrize("name", sorted(CONTRACT))
def test_contract_entries_are_the_restatements_as_a_multiset(name):
    """3: the real entries of bin (region, angle) are the restatement's; the order inside a run is free"""
    n_real = 0
    for s, p, L, pred, part in _listed(name):
        want = pred["parts"][p]["bins"]
        for b in sorted(set(want) | set(part["raw"])):
            got = np.sort(part["raw"].get(b, np.zeros(0, dtype=np.int64)))
            got = got[got < L["rg_zero"]]
            assert np.array_equal(got, want.get(b, np.zeros(0, dtype=np.int64))), (s, p, b)
            n_real += len(got)
    assert n_real > 0


@pytest.mark.parametrize("name", sorted(CONTRACT))
def test_contract_no_pair_is_lost_or_doubled(name):
    """4: over all bins of an angle the real entries number exactly the query's valid readings"""
    for s, p, L, pred, part in _listed(name):
        count = np.zeros(L["lnw"], dtype=np.int64)
        for b, e in part["raw"].items():
            count[b % L["lnw"]] += int((e < L["rg_zero"]).sum())
        nk = min(L["nt"], (p + 1) * L["lnw"]) - p * L["lnw"]
        assert count[:nk].tolist() == [L["nq"]] * nk and not count[nk:].any(), (s, p)


@pytest.mark.parametrize("name", sorted(CONTRACT))
def test_contract_flags(name):
    """5: every flag is the restatement's prediction (here: the padded total; the refused ones are further down)"""
    for slot in _contract(name)["slots"]:
        assert slot["pred"]["lost"] == 0
        assert slot["L"]["flags"].tolist() == [p["flag"] for p in slot["pred"]["parts"]]


@pytest.mark.parametrize("name", sorted(CONTRACT))
def test_contract_entries_lie_inside_their_boxes(name):
    """6a (correctness): a correlate block stages only its boxes: every real entry's (er, ex) lies inside rbox[region][part]"""
    for s, p, L, pred, part in _listed(name):
        for b, e in part["raw"].items():
            R = b // L["lnw"]
            _, _, er, ex = ref.decode(e[e < L["rg_zero"]], R, L["rg_h"], L["rg_cls"], L["nrx"])
            r0, r1, x0, x1 = L["rbox"][R, p]
            assert (er >= r0).all() and (er <= r1).all() and (ex >= x0).all() and (ex <= x1).all(), (s, p, b, L["rbox"][R, p].tolist())


@pytest.mark.parametrize("name", sorted(CONTRACT))
def test_contract_boxes_are_tight(name):
    """6b (cost): the box is exactly the tight one, or the empty sentinel 255, 0, 255, 0 -- a looser box is paid for in staging"""
    for s, p, L, pred, part in _listed(name):
        assert np.array_equal(L["rbox"][:, p], pred["box"][:, p]), (s, p, np.nonzero((L["rbox"][:, p] != pred["box"][:, p]).any(axis=1))[0][:8].tolist())


@pytest.mark.parametrize("name", ["beams_1081", "lattice_13", "beams_2047", "yagpy"])
def test_angle_table_is_within_one_ulp_of_numpy(name):
    """the cos / sin the builder read against numpy's of the oracle's angles (a report on the device's fp64 cos and sin: the
    multiset comparison above uses the device's own table)"""
    from oracle import oracle as orc
    run = _contract(name)
    cfg = dict(orc.DEFAULT_CONFIG, **(run["cfg"] or {}))
    L, q = run["slots"][0]["L"], run["plain"][0]
    t = q.corrected_pose.euler[-1]
    if run["yag"]:
        # numpy.arange's k-th value, start + k * ((start + step) - start): the launch lattice may hold one angle more than the item's own
        start, stop = -0.5 * cfg["coarse_search_angle_offset"] + t, 0.5 * cfg["coarse_search_angle_offset"] + t
        a = start + np.arange(L["nt"]) * ((start + cfg["coarse_angle_resolution"]) - start)
        own = orc.arange(start, stop, cfg["coarse_angle_resolution"])
        assert L["nt"] >= len(own) and np.array_equal(a[:len(own)], own)
    else:
        a = (t - cfg["coarse_search_angle_offset"]) + np.arange(L["nt"]) * cfg["coarse_angle_resolution"]
    want = np.stack([np.cos(a), np.sin(a)], axis=1)
    ulps = np.abs(L["ctrig"] - want) / np.spacing(np.abs(want))
    print("largest difference of the angle table: %.2f ulp" % ulps.max())
    assert ulps.max() <= 1.0


def test_read_back_refuses_calls_without_lists():
    from yag_slam_amd import _capi
    q, base = cfg2_scans()
    m = _matcher()
    with pytest.raises(_capi.YmError) as e:
        m.debug_pair_lists(0)  # no call yet
    assert e.value.code == -1
    nq, nb = _native(q), [_native(b) for b in base]
    m.match_scan(nq, nb, True, True)  # a single match: the direct kernel
    with pytest.raises(_capi.YmError) as e:
        m.debug_pair_lists(0)
    assert e.value.code == -1
    m.match_scan_batch(nq, _chains(nb), True, True)
    assert m.debug_pair_lists(0)["n_slots"] == 1
    with pytest.raises(_capi.YmError) as e:
        m.debug_pair_lists(1)  # one query: one slot
    assert e.value.code == -1
    m.debug_option(14, 4)  # the gather correlate: other lists
    m.match_scan_batch(nq, _chains(nb), True, True)
    with pytest.raises(_capi.YmError) as e:
        m.debug_pair_lists(0)
    assert e.value.code == -1
    m.close()


# ---- natural refusals: no forcing option ----------------------------------------------------------------------------------------------------
REFUSALS = ("pad_mixed", "angle_alone", "regions", "regions_edge", "across")


def _same_results(a, b, meta=True):
    for x, y in zip(a, b):
        assert x.response == y.response and x.covariance == y.covariance and (x.meta == y.meta or not meta)
        assert (x.best_pose.x, x.best_pose.y, x.best_pose.euler[-1]) == (y.best_pose.x, y.best_pose.y, y.best_pose.euler[-1])


def _lists_state(m, n_slots):
    """flags, starts and boxes as they are; the entries of every listed part sorted inside each bin (the order inside a run is free, and a
    call that builds its lists again may place them otherwise)"""
    out = []
    for s in range(n_slots):
        L = m.debug_pair_lists(s)
        listed = []
        for p in range(L["lparts"]):
            if L["flags"][p] >= 0:
                e = L["entries"][p, :L["flags"][p]].astype(np.int64)
                bin_of = np.repeat(np.arange(L["nbins"]), np.diff(L["starts"][p]))
                listed.append(e[np.lexsort((e, bin_of))].tobytes())
        out.append(dict(flags=L["flags"].tobytes(), starts=L["starts"].tobytes(), rbox=L["rbox"].tobytes(), entries=listed))
    return out


@pytest.mark.parametrize("kind", REFUSALS)
def test_lists_refused_on_their_real_counts(kind):
    """A sparse scan's padded lists do not fit (tests/test_pairlist_host.py says by which clause and by how much).  The flags are
    the restatement's; the integer sums of every item are the direct kernel's and the oracle's although part of an item's angles
    (or part of the call's queries) went through correlate_region_kernel's gather and the rest through its per-cell path; the
    results are the single calls'; a second enqueue of the same call gives the same bytes.

    Unreachable: `pos0 + all <= 65532` (test_clause_b_is_a_belt shows the arithmetic) -- left to option 14 = 3."""
    from oracle import oracle as orc
    from yag_slam_amd.scan_matching import ScanMatcher
    if kind == "across":
        names = [host.ACROSS[i % len(host.ACROSS)] for i in range(8)]
        preds = {n: v for n, v in host.across_prediction().items()}
        cfg = None
    else:
        names = [kind] * 8
        preds = {kind: host.sparse_prediction(kind)}
        cfg = host.SPARSE[kind][5]
    plain_q = {n: host.named_query(n) for n in set(names)}
    plain_b = {n: host.named_base(n) for n in set(names)}
    room = cfg2_scans()[1]
    subsets = [slice(0, 3), slice(0, 1), slice(1, 3), slice(None, None, -1), slice(0, 2), slice(2, 3), slice(0, 3), slice(1, 2)]
    plain_chains = [plain_b[n][subsets[i]] + (room[:2] if i % 3 == 1 else []) for i, n in enumerate(names)]
    nat_q = {n: _native(q) for n, q in plain_q.items()}
    nat_chains = [[_native(b) for b in ch] for ch in plain_chains]

    def call(m):
        if kind == "across":
            return m.match_pairs([nat_q[n] for n in names], nat_chains, True, True)
        return m.match_scan_batch(nat_q[kind], nat_chains, True, True)[0]

    m = _matcher(cfg)
    per = call(m)
    assert m.debug_counters()["last_correlate"] == REGION
    assert all(r.meta["expansions"] == 0 for r in per)
    dims = per[0].meta["coarse_dims"]
    # the flags: the CPU's prediction (from the oracle's points), and the restatement on what the builder itself read
    slots = _read_slots(m, cfg)
    order = list(dict.fromkeys(names))  # a query slot per distinct query, in the order of the items
    assert len(slots) == len(order)
    for slot, n in zip(slots, order):
        g, pred, _ = preds[n]
        assert {k: slot["L"][k] for k in GEOMETRY_KEYS} == {k: g[k] for k in GEOMETRY_KEYS}, n
        assert slot["L"]["flags"].tolist() == [p["flag"] for p in pred["parts"]], n
        assert slot["L"]["flags"].tolist() == [p["flag"] for p in slot["pred"]["parts"]], n
    sums = [m.debug_sums(0, item=i, dims=dims) for i in range(len(names))]
    assert all(s.any() for s in sums)
    first = _lists_state(m, len(slots))
    hits = m.debug_counters()["list_cache_hits"]
    # a second enqueue of the same call: the same bytes (a single-query call finds its lists in the buffers: read back all the same)
    again = call(m)
    assert m.debug_counters()["last_correlate"] == REGION
    assert m.debug_counters()["list_cache_hits"] == hits + (0 if kind == "across" else 1)
    _same_results(again, per)
    for i in range(len(names)):
        assert np.array_equal(m.debug_sums(0, item=i, dims=dims), sums[i]), i
    for a, b in zip(_lists_state(m, len(slots)), first):
        for key in ("flags", "starts", "rbox", "entries"):
            assert a[key] == b[key], key
    m.close()
    # the direct kernel
    d = _matcher(cfg, opts={14: 1})
    direct = call(d)
    assert d.debug_counters()["last_correlate"] == "correlate_kernel"
    for i in range(len(names)):
        assert np.array_equal(d.debug_sums(0, item=i, dims=dims), sums[i]), i
    _same_results(direct, per)
    d.close()
    # the oracle, and the single calls
    o = orc.Oracle(cfg, "karto")
    one = ScanMatcher(cfg)
    for i, n in enumerate(names):
        o.match_scan(plain_q[n], plain_chains[i], True, True)
        assert np.array_equal(o.sums(0), sums[i]), i
        _same_results([one.match_scan(nat_q[n], nat_chains[i], True, True)], [per[i]], meta=False)
    one.close()
