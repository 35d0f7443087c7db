"""The region correlate's gather loop (correlate_region_kernel's `gather`, rg_gather4_run and rg_gather4 in
yag_slam_amd/csrc/ym_k_region.hpp) on the smallest inputs at which its carried state can go wrong.  The loop keeps, for each of a
quad's two pair slots, the lane's dword base and byte selector of the slot's misalignment class (entry & 3) and recomputes them only
when the class in the slot changes; entries past the first 256 of a wave's segment take the older function.

Every case is a batch of nine items with option 28 = 8 (the LDS correlates from 8 items on) that must have taken
correlate_region_kernel; its integer sum volumes are compared bit for bit with the direct kernel's (option 14 = 1), one item with the
oracle's.  What a case is meant to reach is asserted on the lists read back from the device (ym_debug_pair_lists), so that no case
can pass without meeting it."""
import functools

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from tests.util import PlainScan, cfg2_scans  # noqa: E402

REGION = "correlate_region_kernel"
RG_FLUSH = 652  # patches per set of 16-bit sums (ym_k_region.hpp, YM_RG_FLUSH)
NO_EXPANSION = {"use_response_expansion": False}  # (debug_sums and the read-back see the matcher's LAST call)


def _native(plain):
    from yag_slam_amd.models import LocalizedRangeScan
    p = plain.corrected_pose
    return LocalizedRangeScan(plain.ranges, plain.min_angle, plain.max_angle, plain.angle_increment,
                              plain.min_range, plain.max_range, plain.range_threshold, p.x, p.y, p.euler[-1])


def _matcher(cfg, opts):
    from yag_slam_amd.scan_matching import ScanMatcher
    m = ScanMatcher(cfg)
    m.debug_option(28, 8)
    for k, v in opts.items():
        m.debug_option(k, v)
    return m


def _ragged(b):
    """nine chains of a base list of nine scans: ragged and reversed, none empty"""
    return [b, b[:3], b[2:9], b[::-1], b[4:5], b[1:], b[:7], b[3:], b[5:6]]


def _cut(q, n):
    return PlainScan(q.ranges[:n], q.min_angle, q.angle_increment, q.min_range, 20.0, (3.0, 3.0, 0.0))


def _near(pose):
    """1081 readings of 0.6 m: the patches of an angle crowd into one or two regions.  (Seen from a heading of pi most of them lie
    on the low-x side of the window's centre, which is a region boundary: one region then holds more than a set's worth.)"""
    q, _ = cfg2_scans()
    return PlainScan(np.full(len(q.ranges), 0.6), q.min_angle, q.angle_increment, q.min_range, 20.0, pose)


def _inputs(case):
    """-> (config, query, the nine chains) as plain scans; chains[0] is what the oracle matches item 0 against"""
    q, base = cfg2_scans()
    if case == "cfg2":
        return None, q, _ragged(base)
    if case == "beams_400":
        return None, _cut(q, 400), _ragged(base)
    if case == "lattice_13":  # 13 x 13 x 21: one lane per lattice row, the second half of the wave idles
        return {"search_size": 0.24}, q, _ragged(base)
    assert case == "near"
    th = 3.14159
    own = [_near((3.02, 2.99, th + 0.003)), _near((2.98, 3.01, th - 0.004)), _near((3.0, 3.03, th))]  # (the query scores on these)
    mixed = own + base[:6]
    return NO_EXPANSION, _near((3.0, 3.0, th)), _ragged(mixed)


def _bins(m):
    """the non-empty bins (region, angle) of query slot 0 of the last call: what ONE wave gathers in ONE round"""
    L = m.debug_pair_lists(0)
    assert L["n_slots"] == 1
    flat = L["entries"].reshape(-1).astype(np.int64)
    bins, per_angle = [], np.zeros(L["nt"], dtype=np.int64)
    for p in range(L["lparts"]):
        assert L["flags"][p] >= 0, "part %d has no list: these inputs fit" % p
        st = L["starts"][p].astype(np.int64)
        for b in np.nonzero(np.diff(st))[0]:
            bins.append(flat[st[b]:st[b + 1]])
            per_angle[p * L["lnw"] + b % L["lnw"]] += st[b + 1] - st[b]
    return L, bins, per_angle


@functools.lru_cache(maxsize=None)
def _run(case):
    """the case through correlate_region_kernel and through the direct kernel, each once; the lists of the former"""
    from oracle import oracle as orc
    cfg, query, chains = _inputs(case)
    nq, nchains = _native(query), [[_native(s) for s in ch] for ch in chains]
    out = {}
    # (neighbouring 0.6 m readings fall into the same cell: the matcher would merge equal lookup offsets and such a call takes
    #  another correlate -- option 13 = 2 keeps every reading a pair of its own)
    extra = {13: 2} if case == "near" else {}
    for kind, opts in (("region", {12: 1}), ("direct", {12: 1, 14: 1})):
        m = _matcher(cfg, {**opts, **extra})
        per, best = m.match_scan_batch(nq, nchains, True, True)
        assert m.debug_counters()["last_correlate"] == (REGION if kind == "region" else "correlate_kernel")
        assert all(r.meta["expansions"] == 0 for r in per)
        dims = per[0].meta["coarse_dims"]
        out[kind] = dict(sums=[m.debug_sums(0, item=i, dims=dims) for i in range(len(chains))], per=per, best=best, dims=dims)
        if kind == "region":
            out["L"], out["bins"], out["per_angle"] = _bins(m)
        m.close()
    o = orc.Oracle(cfg, "karto")
    o.match_scan(query, chains[0], True, True)
    out["oracle"] = o.sums(0)
    return out


def _pair_classes(e):
    """the class of every pair of a bin; both entries of a pair share it (the loop reads it off the pair's first entry)"""
    assert len(e) % 4 == 0
    assert np.array_equal(e[0::2] & 3, e[1::2] & 3)
    return e[0::2] & 3


def _assert_equal_sums(run):
    for i, (a, b) in enumerate(zip(run["region"]["sums"], run["direct"]["sums"])):
        assert np.array_equal(a, b), i
    assert run["region"]["sums"][0].any()
    assert np.array_equal(run["region"]["sums"][0], run["oracle"])
    for x, y in zip(run["region"]["per"], run["direct"]["per"]):
        assert x.response == y.response and x.covariance == y.covariance and x.meta == y.meta
        assert (x.best_pose.x, x.best_pose.y, x.best_pose.euler[-1]) == (y.best_pose.x, y.best_pose.y, y.best_pose.euler[-1])
    assert run["region"]["best"] == run["direct"]["best"]


def test_all_four_classes_and_every_kind_of_run_change():
    """cfg2 against nine ragged and reversed chains.  The lists hold all four classes; a quad whose two pairs differ in class (only
    the second slot's state changes); a run that changes on a quad boundary (both slots' states change at once); a bin of a single
    class (the states are set once); a bin that ends in an all-padding pair; and an angle with more than a set's worth of patches,
    all in segments of at most 256 entries: the set is written out from inside the new loop."""
    run = _run("cfg2")
    L, bins = run["L"], run["bins"]
    z = L["rg_zero"]
    assert z % 4 == 0
    pcs = [_pair_classes(e) for e in bins]
    assert set(np.concatenate(pcs).tolist()) == {0, 1, 2, 3}
    assert any((pc[0::2] != pc[1::2]).any() for pc in pcs), "no quad straddles two runs"
    assert any((pc[1:-1:2] != pc[2::2]).any() for pc in pcs), "no run changes on a quad boundary"
    assert any((pc == pc[0]).all() for pc in pcs), "no bin of a single class"
    assert any(e[-2] == z and e[-1] == z for e in bins), "no bin ends in an all-padding pair"
    assert max(len(e) for e in bins) <= 256
    assert run["per_angle"].min() > RG_FLUSH  # (1081 readings per angle: every wave fills a set)
    _assert_equal_sums(run)


def test_class_three_in_the_second_half_of_a_lattice_row():
    """The second half of a lattice row starts 13 bytes into the row: at class 3 its dword address carries (1 + 3 = 4), the only place
    where the lane base of a class is not the lane's own.  A bin of at least two quads holds entries of class 3, on a 26-wide lattice."""
    run = _run("cfg2")
    assert run["region"]["dims"][0] == 26
    assert any(len(e) >= 8 and ((e & 3) == 3).any() for e in run["bins"])
    _assert_equal_sums(run)


def test_a_segment_longer_than_256_entries_with_the_flush_inside_it():
    """1081 readings of 0.6 m: some (region, angle) bin holds more than 652 entries, so its wave gathers 256 of them from the register
    pair (the new loop), the rest as per-lane loads through rg_gather4 (the path this change leaves on the older function), and writes
    a set of sums out in the middle of a run."""
    run = _run("near")
    longest = max(len(e) for e in run["bins"])
    print("longest bin: %d entries" % longest)
    assert longest > RG_FLUSH
    _assert_equal_sums(run)


@pytest.mark.parametrize("case", ["lattice_13", "beams_400"])
def test_one_lane_per_row_and_a_short_query(case):
    """13 x 13 lattice: `half * YM_RG_G < nx` fails in the second half of the wave, whose lanes then read what lane (row 0, half 0)
    reads -- their states must be that lane's.  400 beams: no set is ever written out mid-way."""
    run = _run(case)
    if case == "lattice_13":
        assert tuple(run["region"]["dims"][:2]) == (13, 13)
    else:
        assert run["per_angle"].max() < RG_FLUSH
    assert {0, 1, 2, 3} == set(np.concatenate([_pair_classes(e) for e in run["bins"]]).tolist())
    _assert_equal_sums(run)


def test_the_production_form_scores_its_own_sums():
    """No kept sums: correlate_region_kernel scores the sums it gathered (fused scoring).  Nine distinct queries (cfg2's readings at
    nine priors), each against its own chain, as a resident pairs batch: response, pose and covariance are the single calls', as
    doubles."""
    from yag_slam_amd.scan_matching import ScanMatcher
    q, base = cfg2_scans()
    chains = [[_native(s) for s in ch] for ch in _ragged(base)]
    queries = [_native(PlainScan(q.ranges, q.min_angle, q.angle_increment, q.min_range, 20.0,
                                 (3.0 + 0.01 * (i % 3), 3.0 - 0.01 * (i // 3), 0.004 * (i - 4)))) for i in range(len(chains))]
    m = _matcher(None, {})
    b = m.make_pairs_batch(queries, chains)
    b.run_async(True, True, slot=0)
    per, _, _ = b.wait(0)
    assert m.debug_counters()["last_correlate"] == REGION
    one = ScanMatcher()
    for i in range(len(chains)):
        s, a = one.match_scan(queries[i], chains[i], True, True), per[i]
        assert a.response == s.response and a.covariance == s.covariance, i
        assert (a.best_pose.x, a.best_pose.y, a.best_pose.euler[-1]) == (s.best_pose.x, s.best_pose.y, s.best_pose.euler[-1]), i
    assert per[0].response > 0.0
    one.close()
    m.close()
