"""The region correlate's walk over its listed regions (correlate_region_kernel in yag_slam_amd/csrc/ym_k_region.hpp): the round table a
block builds before the walk, the one LDS read per round that takes a region's box, its source offset and the wave's segment of the
region after it, and the entry lists that are loaded two rounds before they are gathered.  The smallest inputs at which that can go
wrong: lists of 0, 1, 2 and 3 regions (the two-ahead load runs past the end of the list in every position), lists dealt out to 2 and
3 blocks of which some get nothing, 21 angles in blocks of eight (the last block has five working waves), and a segment of more than
256 entries in a round that was prefetched.

The small cases are batches of EIGHT items: the three items a case is about and five repeats of them.  Eight is the smallest batch
the library hands to this kernel -- below it a call has no query slots and no pair lists (ym_host_plan.hpp, plan_jobs), so a batch
of three takes the direct kernel whatever the options say.

Every call must have taken correlate_region_kernel; its integer sum volumes are compared bit for bit with the same kernel's per-cell
path (option 14 = 2: no lists, no regions, no LDS) and with the CPU oracle's.  What a case is meant to reach is asserted on the lists
read back from the device (ym_debug_pair_lists), the long segment also on the numpy restatement of the lists (tests/pairlist_ref.py),
so that no case can pass without meeting it."""
import functools

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from tests import pairlist_ref as ref  # noqa: E402
from tests.util import PlainScan, cfg2_scans  # noqa: E402

REGION = "correlate_region_kernel"
NO_EXPANSION = {"use_response_expansion": False}  # (debug_sums and the read-back see the matcher's LAST call)


def _native(plain):
    from yag_slam_amd.models import LocalizedRangeScan
    p = plain.corrected_pose
    return LocalizedRangeScan(plain.ranges, plain.min_angle, plain.max_angle, plain.angle_increment,
                              plain.min_range, plain.max_range, plain.range_threshold, p.x, p.y, p.euler[-1])


def _arcs(spec, pose=(3.0, 3.0, 0.0)):
    """a 1081-beam scan that sees only arcs: (bearing in degrees, half width in beams, range in metres) each; every other reading
    lies beyond the scan's threshold.  An arc close to the sensor keeps its patches of all 21 angles inside one region."""
    q, _ = cfg2_scans()
    r = np.full(len(q.ranges), 25.0)
    for deg, hw, rng in spec:
        b = int(round((np.radians(deg) - q.min_angle) / q.angle_increment))
        r[b - hw:b + hw + 1] = rng
    return PlainScan(r, q.min_angle, q.angle_increment, q.min_range, 20.0, pose)


def _near(pose):
    """1081 readings of 0.6 m: the patches of an angle crowd into four regions, two of which hold more than 256 of them"""
    q, _ = cfg2_scans()
    return PlainScan(np.full(len(q.ranges), 0.6), q.min_angle, q.angle_increment, q.min_range, 20.0, pose)


def _seen_from_nearby(make):
    """a chain a synthetic query scores on: its own readings from three poses around it"""
    return [make((3.02, 2.99, 0.003)), make((2.98, 3.01, -0.004)), make((3.0, 3.03, 0.0))]


ONE = [(45, 40, 0.6)]
TWO = ONE + [(-90, 6, 1.2)]
THREE = [(45, 6, 1.0), (-45, 6, 1.0), (120, 6, 1.0)]
TH = 3.14159


def _eight(queries, chains):
    """the three items a case is about, then five repeats of them: the smallest batch that takes the region correlate"""
    return [queries[i % 3] for i in range(8)], [chains[i % 3] for i in range(8)]


def _inputs(call):
    """-> (queries, chains, rsplits); one query: a match_scan_batch call, several: match_pairs, item i = queries[i] against chains[i]"""
    q, base = cfg2_scans()
    if call == "short_lists":  # items that list no region, one, and two (three in one angle block)
        return _eight([_arcs([]), _arcs(ONE), _arcs(TWO)],
                      [base[:2], _seen_from_nearby(lambda p: _arcs(ONE, p)), _seen_from_nearby(lambda p: _arcs(TWO, p))]) + ((1, 2, 3),)
    if call == "mixed":  # three regions; the room: 25 to 27 regions per angle block; a long segment in the third of four regions
        return _eight([_arcs(THREE), q, _near((3.0, 3.0, TH))],
                      [_seen_from_nearby(lambda p: _arcs(THREE, p)), base[:5],
                       [_near((3.02, 2.99, TH + 0.003)), _near((2.98, 3.01, TH - 0.004)), _near((3.0, 3.03, TH))] + base[:3]]) + ((1, 2, 3),)
    assert call == "batch_64"  # the room's scan against 64 ragged chains, the regions dealt out as the host decides
    return [q], [base[i % 10:i % 10 + 1 + i % 7] if i % 5 else base[::-1][:1 + i % 10] for i in range(64)], (0,)


def _matcher(opts):
    from yag_slam_amd.scan_matching import ScanMatcher
    m = ScanMatcher(NO_EXPANSION)
    m.debug_option(42, 8)  # the region correlate from eight items on
    m.debug_option(12, 1)  # keep the integer sums
    m.debug_option(13, 2)  # every reading a pair of its own (equal lookup offsets merged: another correlate)
    for k, v in opts.items():
        m.debug_option(k, v)
    return m


def _listed_regions(m):
    """per query slot (keyed by an item that uses it) and angle block: the regions in which a patch of the block's angles starts, in
    the order the kernel lists them; and every slot's read-back"""
    out, slots = {}, {}
    s, n = 0, 1
    while s < n:
        L = m.debug_pair_lists(s)
        n = L["n_slots"]
        per_part = []
        for p in range(L["lparts"]):
            assert L["flags"][p] >= 0, "slot %d part %d has no list: these inputs fit" % (s, p)
            st = L["starts"][p].astype(np.int64)
            nk = min(L["nt"], (p + 1) * L["lnw"]) - p * L["lnw"]
            per_part.append([R for R in range(L["nregions"]) if st[R * L["lnw"]] != st[R * L["lnw"] + nk]])
        slots[L["qrep"]] = L
        out[L["qrep"]] = per_part
        s += 1
    return out, slots


@functools.lru_cache(maxsize=None)
def _run(call):
    """the call through the region walk once per rsplit, once through the per-cell path; the lists of the former"""
    queries, chains, rsplits = _inputs(call)
    nq, nch = [_native(s) for s in queries], [[_native(s) for s in ch] for ch in chains]
    out = dict(queries=queries, chains=chains, walk={})

    def go(opts):
        m = _matcher(opts)
        if len(nq) == 1:
            per, _ = m.match_scan_batch(nq[0], nch, True, True)
        else:
            per = m.match_pairs(nq, nch, True, True)
        assert m.debug_counters()["last_correlate"] == REGION
        dims = max(tuple(r.meta["coarse_dims"]) for r in per)  # (an item without a reading reports none)
        sums = [m.debug_sums(0, item=i, dims=dims) for i in range(len(nch))]
        return m, dims, sums

    for rs in rsplits:
        m, dims, sums = go({34: rs} if rs else {})
        out["walk"][rs] = sums
        if "regions" not in out:
            out["dims"] = dims
            out["regions"], out["slots"] = _listed_regions(m)
            assert len(nq) == 1 or all(i in out["slots"] for i in range(3))
            if call == "mixed":  # the long segment, from what the builder itself read: the restatement's lists of item 2
                from oracle import oracle as orc
                L = out["slots"][2]
                cells = ref.lookup_cells_karto(m.debug_query_local(item=2), L["ctrig"], L["off_x"], L["off_y"],
                                               1.0 / dict(orc.DEFAULT_CONFIG, **NO_EXPANSION)["resolution"])
                out["restated"] = ref.predict(cells, L["cx0"], L["cy0"], L)
        m.close()
    m, _, out["per_cell"] = go({14: 2})
    m.close()
    return out


def _oracle_sums(query, chain):
    from oracle import oracle as orc
    o = orc.Oracle(NO_EXPANSION, "karto")
    o.match_scan(query, chain, True, True)
    return o.sums(0)


def _shares(n, rsplit):
    """how many of a list of n regions each of the rsplit blocks walks (correlate_region_kernel: region i of the list to block i % rsplit)"""
    return [(n - rsi + rsplit - 1) // rsplit if n > rsi else 0 for rsi in range(rsplit)]


def _assert_walk_is_per_cell(run, oracle_items):
    for rs, sums in run["walk"].items():
        for i, (a, b) in enumerate(zip(sums, run["per_cell"])):
            assert np.array_equal(a, b), (rs, i)
    first = next(iter(run["walk"].values()))
    for i in oracle_items:
        q = run["queries"][i if len(run["queries"]) > 1 else 0]
        assert first[i].any()
        assert np.array_equal(first[i], _oracle_sums(q, run["chains"][i])), i


def test_lists_of_zero_one_two_and_three_regions():
    """Items of distinct queries (items 0, 1, 2 and their repeats), 21 angles in blocks of 8, 8 and 5: an empty query lists nothing, an arc 0.6 m away one region
    in every angle block, two arcs two regions (three in one block); the three-arc query of the mixed call three in every block.
    With the list dealt out to 1, 2 and 3 blocks, blocks walk 0, 1, 2 and 3 regions: the reads and loads that run one and two rounds
    ahead end past the list in every position."""
    run, mixed = _run("short_lists"), _run("mixed")
    assert tuple(run["dims"]) == (26, 26, 21) and run["slots"][1]["lnw"] == 8 and run["slots"][1]["lparts"] == 3
    assert [len(r) for r in run["regions"][0]] == [0, 0, 0]
    assert [len(r) for r in run["regions"][1]] == [1, 1, 1]
    assert sorted(len(r) for r in run["regions"][2]) == [2, 2, 3]
    assert [len(r) for r in mixed["regions"][0]] == [3, 3, 3]
    walked = set()
    for regions in [run["regions"][i] for i in range(3)] + [mixed["regions"][0]]:
        for rs in (1, 2, 3):
            for part in regions:
                walked.update(_shares(len(part), rs))
    assert walked == {0, 1, 2, 3}
    assert 0 in _shares(1, 2) and 0 in _shares(2, 3)  # (a block of an item that HAS regions gets none)
    assert not run["per_cell"][0].any()
    _assert_walk_is_per_cell(run, (1, 2))


def test_a_long_segment_in_a_prefetched_round_and_the_rooms_lists():
    """Items 0, 1, 2 (and their repeats): the three-arc query, the room's 1081-beam scan (some 26 regions per angle block) and 1081 readings of 0.6 m.
    The last lists four regions; its third holds 360 patches per angle: more than the 256 entries a wave carries in registers, in a
    round whose table row and entries were fetched while earlier regions were gathered -- whether one block walks the four regions
    (third round), two (second round of block 0) or three.  Both the device's lists and their restatement on the CPU say so."""
    run = _run("mixed")
    L, regions = run["slots"][2], run["regions"][2]
    assert len(run["regions"][1][0]) > 20
    flat = L["entries"].reshape(-1)
    for p in range(L["lparts"]):
        st = L["starts"][p].astype(np.int64)
        nk = min(L["nt"], (p + 1) * L["lnw"]) - p * L["lnw"]
        assert len(regions[p]) == 4
        R = regions[p][2]
        for w in range(nk):
            b = R * L["lnw"] + w
            n = int(st[b + 1] - st[b])
            real = int((flat[st[b]:st[b + 1]] < L["rg_zero"]).sum())
            assert n > 256 and n % 4 == 0
            assert len(run["restated"]["parts"][p]["bins"][b]) == real > 256
    _assert_walk_is_per_cell(run, (0, 1, 2))


def test_a_batch_of_64_items():
    """The room's scan against 64 ragged chains in one call, the lists dealt out to as many blocks as the host chooses for a batch
    of that size: every item's sums are the per-cell path's, item 0's the oracle's."""
    run = _run("batch_64")
    assert len(run["per_cell"]) == 64 and tuple(run["dims"]) == (26, 26, 21)
    (regions,) = run["regions"].values()  # (one query: one slot)
    assert min(len(r) for r in regions) > 20
    _assert_walk_is_per_cell(run, (0,))
