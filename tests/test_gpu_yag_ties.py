"""The rounding proofs behind the "yagpy" fast paths, attacked on the device itself.

Three fp64 arguments let table-driven kernels stand in for the reference's rule np.round(((xvals[i] + r) - o) / res): the lattice proof
of yag_lattice_kernel (its guard), and yag_rint_div in yag_fine_kernel and in yag_map_kernel (its margin).  tests/test_yag_lattice_guard.py
attacks numpy copies of the predicates; here the readings themselves are aimed so that the DEVICE's operands land where the proofs
decide: within the guard of a rounding tie and regular, within it and genuinely irregular, just outside it; on the doubles where
rint(d * fl(1 / res)) and rint(d / res) part, at cells whose bytes differ.

Each case runs its queries once as they come, reads back what the kernels computed with (ym_debug_yag_frame), aims the ranges
(tests/yag_ties_ref.py: one Newton step on the read-back operands), creates the scans again and runs them again.  Nothing is assumed
about where the readings landed: the achieved distances are computed from the second read-back by the numpy restatement of the rule,
the bands a case must hold are ASSERTED (test_the_attack_reached_its_bands), and no step is repeated.  Everything compared is an
integer or a decision: no tolerance.  The restatement is held to reference-made numbers in tests/test_yag_ties_host.py.

The pair counters are exact: yag_lattice_kernel visits every (point, angle) pair of an item whatever it has found before, so
yag_pairs_checked and yag_pairs_failed are functions of the operands alone.

One band cannot be reached everywhere: kilometres from the origin d = (x + r) - o is a difference of coordinates whose ulp is a
thousand ulps of d, so no choice of ranges puts d within the few ulps of a tie where product and quotient round apart; neither can it
where the cell size has an exact reciprocal (0.25, the control).  There the band is required to be EMPTY (tests/yag_ties_ref.py,
rint_div_reachable) and the sums are still compared."""
import functools

import numpy as np
import pytest

from tests import yag_ties_ref as R

pytestmark = pytest.mark.gpu
ROLES = ("regular", "irregular", "fine")


def _scan(ranges, pose):
    from yag_slam_amd.models import LocalizedRangeScan
    return LocalizedRangeScan(np.asarray(ranges, dtype=np.float64), R.MIN_ANGLE, R.MIN_ANGLE + (R.N_BEAMS - 1) * R.ANGLE_INCREMENT,
                              R.ANGLE_INCREMENT, 0.05, 30.0, 6.0, float(pose[0]), float(pose[1]), float(pose[2]))


def _frame_equal(a, b):
    return all(np.array_equal(a[n], b[n]) for n in ("xvals", "yvals", "tvals", "trig", "points")) and all(
        a[n] == b[n] for n in ("ox", "oy", "res", "grid_w", "grid_h"))


def _pose(r):
    return (r.best_pose.x, r.best_pose.y, r.best_pose.euler[-1])


def _delta(after, before):
    return {k: after[k] - before[k] for k in ("yag_fast_items", "yag_fallback_items", "yag_pairs_checked", "yag_pairs_failed")}


@functools.lru_cache(maxsize=None)
def attacked(case):
    """One case, attacked once: the aimed scans, what the device computed with on the final run, what it answered and what the
    restatement expects -- shared, unchanged, by the tests below."""
    from yag_slam_amd.scan_matching import ScanMatcher
    cfg, problem = R.case_config(case), R.case_problem(case)
    base = [_scan(r, p) for r, p in problem["base"]]
    m = ScanMatcher(cfg, semantics="yagpy")
    runs = []

    def run(role, ranges):
        q = _scan(ranges, problem["queries"][role][1])  # (the product's creation path: a new scan for every new set of ranges)
        before = m.debug_counters()
        res = m.match_scan(q, base, True, True)
        cnt = m.debug_counters()
        f0, f1 = m.debug_yag_frame(0, 0), m.debug_yag_frame(0, 1)
        grid, info = m.debug_grid()
        assert (info.origin_x, info.origin_y, info.width) == (f0["win_origin"], f0["win_origin"], f0["win_w"])
        out = dict(query=q, result=res, counters=_delta(cnt, before), last_correlate=cnt["last_correlate"], f0=f0, f1=f1, grid=grid.copy(),
                   origin=(f0["win_origin"], f0["win_origin"]), sums0=m.debug_sums(0, dims=res.meta["coarse_dims"]).astype(np.int64),
                   sums1=m.debug_sums(1, dims=res.meta["fine_dims"]).astype(np.int64))
        runs.append(role)
        return out

    aimed = R.attack_chain_case(lambda role, ranges: (lambda o: (o["f0"], o["f1"], o["grid"], o["origin"]))(run(role, ranges)), problem)
    assert runs == list(ROLES)  # one run per query before the final one: nothing was tried twice
    out = dict(cfg=cfg, base=base, matcher=m, items={})
    for role in ROLES:
        it = run(role, aimed[role])
        it["want0"] = R.rule_sums(it["f0"], it["grid"], it["origin"])
        it["want1"] = R.rule_sums(it["f1"], it["grid"], it["origin"])
        it["bands"], it["facts"] = R.band_counts(it["f0"])
        it["decision"] = R.expected_decision(it["f0"], it["facts"])
        out["items"][role] = it
    return out


CASES = sorted(R.CHAIN_CASES)


@pytest.mark.parametrize("case", CASES)
def test_the_attack_reached_its_bands(case):
    """The conditions under which the other tests of this file mean anything, measured on the operands the device read back."""
    a = attacked(case)
    spec = R.CHAIN_CASES[case]
    far = abs(spec["shift"][0]) > 1000
    reg, irr, fine = (a["items"][r] for r in ROLES)
    print(case, {r: (a["items"][r]["bands"], a["items"][r]["decision"]) for r in ROLES})
    for axis in ("x", "y"):
        # inside the guard and regular along the axis (the exhaustive check accepts them), just outside it (accepted at once) -- in an item
        # that holds no irregular pair, so that the decision under test is "regular"
        assert reg["bands"][(axis, "inside_regular")] >= R.NEED, (axis, reg["bands"])
        assert reg["bands"][(axis, "just_outside")] >= R.NEED, (axis, reg["bands"])
        assert reg["bands"][(axis, "inside_irregular")] == 0, (axis, reg["bands"])
        # inside the guard and irregular: the item falls back
        assert irr["bands"][(axis, "inside_irregular")] >= R.NEED, (axis, irr["bands"])
        if far:  # between 2^-40 cells and the full guard from a tie: a guard without its M / res term would wave these through
            assert reg["bands"][(axis, "beyond_2m40")] >= R.NEED and irr["bands"][(axis, "beyond_2m40")] >= R.NEED, (axis, reg["bands"], irr["bands"])
    assert reg["decision"]["regular"] and not irr["decision"]["regular"]
    # the fine pass: positions where product and quotient round differently AND the two cells hold different bytes
    both, differ = R.rint_div_count(fine["f1"], fine["grid"], fine["origin"])
    print(case, "fine pass: product != quotient at", differ, "positions,", both, "of them on differing bytes")
    if R.rint_div_reachable(spec):
        assert both >= R.NEED, (both, differ)
    else:
        assert differ == 0, (both, differ)


@pytest.mark.parametrize("case", CASES)
def test_lattice_decision_and_pair_counts_are_the_restatements(case):
    a = attacked(case)
    for role in ROLES:
        it = a["items"][role]
        assert R.proof_claim_holds(it["facts"]), role  # every pair the guard lets through at once IS regular: the proof's claim
        d, c = it["decision"], it["counters"]
        assert (c["yag_fast_items"], c["yag_fallback_items"]) == ((1, 0) if d["regular"] else (0, 1)), (role, c, d)
        assert it["f0"]["regular"] == int(d["regular"]), role
        assert (c["yag_pairs_checked"], c["yag_pairs_failed"]) == (d["checked"], d["failed"]), (role, c, d)
        assert it["last_correlate"] == "correlate_kernel"


def _batch(a, n, options):
    """the three attacked queries, over and over, as one enqueue of n independent matches"""
    from yag_slam_amd.scan_matching import ScanMatcher
    m = ScanMatcher(a["cfg"], semantics="yagpy")
    for k, v in options:
        m.debug_option(k, v)
    roles = [ROLES[i % 3] for i in range(n)]
    per = m.match_pairs([a["items"][r]["query"] for r in roles], [a["base"]] * n, True, True)
    return m, roles, per


@pytest.mark.parametrize("route", ["direct", "pairwise", "region", "gather"])
@pytest.mark.parametrize("case", CASES)
def test_coarse_sums_of_attacked_items_on_every_route(case, route):
    from yag_slam_amd.scan_matching import ScanMatcher
    a = attacked(case)
    if route == "direct":
        for role in ROLES:
            it = a["items"][role]
            assert it["last_correlate"] == "correlate_kernel"
            assert np.array_equal(it["sums0"], it["want0"]), (role, int((it["sums0"] != it["want0"]).sum()))
        return
    if route == "pairwise":
        m = ScanMatcher(a["cfg"], semantics="yagpy")
        m.debug_option(46, 0)
        for role in ROLES:
            it = a["items"][role]
            r = m.match_scan(it["query"], a["base"], True, True)
            assert m.debug_counters()["last_correlate"] is None
            assert _frame_equal(m.debug_yag_frame(0, 0), it["f0"])
            got = m.debug_sums(0, dims=r.meta["coarse_dims"]).astype(np.int64)
            assert np.array_equal(got, it["want0"]), (role, int((got != it["want0"]).sum()))
            # the fast and the forced-slow matcher: the same bytes
            assert (r.response, r.covariance) == (it["result"].response, it["result"].covariance), role
            assert _pose(r) == _pose(it["result"]), role
        return
    m, roles, per = _batch(a, 10, [(28, 8)] + ([(14, 4)] if route == "gather" else []))
    cnt = m.debug_counters()
    fits_region = a["items"]["regular"]["f0"]["lat_nx"] <= 26
    assert cnt["last_correlate"] == ("correlate_region_kernel" if route == "region" and fits_region else "gather_kernel")
    n_reg = sum(a["items"][r]["decision"]["regular"] for r in roles)
    assert (cnt["yag_fast_items"], cnt["yag_fallback_items"]) == (n_reg, 10 - n_reg)
    assert cnt["yag_pairs_checked"] == sum(a["items"][r]["decision"]["checked"] for r in roles)
    assert cnt["yag_pairs_failed"] == sum(a["items"][r]["decision"]["failed"] for r in roles)
    for i, role in enumerate(roles):
        it = a["items"][role]
        if i < 3:
            assert _frame_equal(m.debug_yag_frame(i, 0), it["f0"]), role
        got = m.debug_sums(0, item=i, dims=per[i].meta["coarse_dims"]).astype(np.int64)
        assert np.array_equal(got, it["want0"]), (i, role, int((got != it["want0"]).sum()))
        assert (per[i].response, per[i].covariance, _pose(per[i])) == (it["result"].response, it["result"].covariance, _pose(it["result"])), (i, role)


@pytest.mark.parametrize("route", ["rows", "bytes", "pairwise", "batch64"])
@pytest.mark.parametrize("case", CASES)
def test_fine_sums_of_attacked_items_on_every_route(case, route):
    from yag_slam_amd.scan_matching import ScanMatcher
    a = attacked(case)
    if route == "rows":
        for role in ROLES:
            it = a["items"][role]
            assert np.array_equal(it["sums1"], it["want1"]), (role, int((it["sums1"] != it["want1"]).sum()))
        return
    if route in ("bytes", "pairwise"):
        m = ScanMatcher(a["cfg"], semantics="yagpy")
        m.debug_option(46, 2 if route == "bytes" else 0)
        for role in ROLES:
            it = a["items"][role]
            r = m.match_scan(it["query"], a["base"], True, True)
            assert _frame_equal(m.debug_yag_frame(0, 1), it["f1"]), role
            got = m.debug_sums(1, dims=r.meta["fine_dims"]).astype(np.int64)
            assert np.array_equal(got, it["want1"]), (role, int((got != it["want1"]).sum()))
        return
    m, roles, per = _batch(a, 64, [])  # 64 items: yag_fine_kernel<64>
    for i in (0, 1, 2, 30, 61, 62, 63):
        it = a["items"][roles[i]]
        assert _frame_equal(m.debug_yag_frame(i, 1), it["f1"]), (i, roles[i])
        got = m.debug_sums(1, item=i, dims=per[i].meta["fine_dims"]).astype(np.int64)
        assert np.array_equal(got, it["want1"]), (i, roles[i], int((got != it["want1"]).sum()))
        got0 = m.debug_sums(0, item=i, dims=per[i].meta["coarse_dims"]).astype(np.int64)
        assert np.array_equal(got0, it["want0"]), (i, roles[i])
        assert (per[i].response, per[i].covariance) == (it["result"].response, it["result"].covariance), (i, roles[i])


# ---- yag_map_kernel: the same attack through match_map_batch and match_scan_sets_batch --------------------------------------------
MAP_CASE_NAMES = sorted(R.MAP_CASES)


def _map_cfg(case):
    c = R.MAP_CASES[case]
    return dict(resolution=c["res"], search_size=c["cells"] * c["res"], smear_deviation=2 * c["res"], range_threshold=6.0)


def _read_items(m, results, n, grid_of):
    out = []
    for i in range(n):
        f0, f1 = m.debug_yag_frame(i, 0), m.debug_yag_frame(i, 1)
        out.append(dict(f0=f0, f1=f1, grid=grid_of(i) if grid_of else None, result=results[i],
                        sums0=m.debug_sums(0, item=i, dims=results[i].meta["coarse_dims"]).astype(np.int64) if f0["kind"] == 2
                        else m.debug_map_sums(0, i, results[i].meta["coarse_dims"]).astype(np.int64),
                        sums1=m.debug_sums(1, item=i, dims=results[i].meta["fine_dims"]).astype(np.int64) if f0["kind"] == 2
                        else m.debug_map_sums(1, i, results[i].meta["fine_dims"]).astype(np.int64)))
    return out


@functools.lru_cache(maxsize=None)
def attacked_map(case, sets):
    """A map case (sets=False: match_map_batch against an uploaded map) or a set case (sets=True: match_scan_sets_batch against the
    chain), attacked once: both queries run as they come, are aimed at the coarse pass's operands, run again, are aimed at the fine pass's and
    run a last time.  Three rounds, none repeated."""
    from yag_slam_amd.scan_matching import ScanMatcher
    cfg, problem, spec = _map_cfg(case), R.map_problem(case), R.MAP_CASES[case]
    res = spec["res"]
    base = [_scan(r, p) for r, p in problem["base"]]
    m = ScanMatcher(cfg, semantics="yagpy")
    out = dict(cfg=cfg, base=base, matcher=m, sets=sets)
    if not sets:
        # the map: the bytes of a chain call's grid around the room, as a correlation grid of its own
        m.match_scan(_scan(*problem["queries"][0]), base, True, True)
        win, _ = m.debug_grid()
        f = m.debug_yag_frame(0, 0)
        full = np.zeros((f["grid_h"], f["grid_w"]), dtype=np.uint8)
        full[f["win_origin"]:f["win_origin"] + win.shape[0], f["win_origin"]:f["win_origin"] + win.shape[1]] = win
        cx0, cy0 = (int(np.round((problem["room_corner"][i] - f[o]) / res)) for i, o in ((0, "ox"), (1, "oy")))
        W, H = spec["map_wh"]
        assert 0 <= cx0 and cx0 + W <= full.shape[1] and 0 <= cy0 and cy0 + H <= full.shape[0]
        cgrid = full[cy0:cy0 + H, cx0:cx0 + W] / 100.0
        out["bytes"] = (100 * cgrid).astype(np.int64)  # what the map keeps of a correlation grid: int(100 * cell)
        assert out["bytes"].max() == 100 and 200 <= min(W, H) and max(W, H) <= 300
        out["map"] = m.upload_correlation_grid(cgrid)
        out["corner"] = (f["ox"] + cx0 * res, f["oy"] + cy0 * res)
        out["coarse"] = R.map_search(case)

    def run(scans, n=None, matcher=None):
        mm = matcher or m
        n = n or len(scans)
        qs = [[scans[i % len(scans)]] for i in range(n)]
        if sets:
            rs = mm.match_scan_sets_batch(qs, [base] * n, True, True)
            # (a wide call may keep the grids of its last chunk only: they are the first run's anyway)
            return _read_items(mm, rs, min(n, 2), (lambda i: mm.debug_grid(i)[0].copy()) if n == len(scans) else None)
        rs = mm.match_map_batch(out["map"], out["corner"][0], out["corner"][1], qs, True, True, coarse=out["coarse"])
        return _read_items(mm, rs, min(n, 2), lambda i: out["bytes"])

    out["run"] = run
    ranges = [np.array(r, dtype=np.float64) for r, _ in problem["queries"]]
    poses = [p for _, p in problem["queries"]]
    first = run([_scan(r, p) for r, p in zip(ranges, poses)])
    assert all(it["f0"]["nq"] == len(r) for it, r in zip(first, ranges))
    ranges = [R.aim_coarse_pass(it["f0"], r, it["grid"]) for it, r in zip(first, ranges)]
    second = run([_scan(r, p) for r, p in zip(ranges, poses)])  # (the fine pass's centre is known only now)
    ranges = [R.aim_fine_pass(it["f1"], r, it["grid"]) for it, r in zip(second, ranges)]
    aimed = [_scan(r, p) for r, p in zip(ranges, poses)]
    out["queries"] = aimed
    before = m.debug_counters()
    out["items"] = run(aimed)
    out["counters"] = {k: m.debug_counters()[k] - before[k] for k in ("map_kernel_items", "map_fallback_items", "sets_kernel_items", "sets_fallback_items")}
    for it in out["items"]:
        it["want0"], it["want1"] = R.rule_sums(it["f0"], it["grid"]), R.rule_sums(it["f1"], it["grid"])
    return out


@pytest.mark.parametrize("sets", [False, True], ids=["map", "sets"])
@pytest.mark.parametrize("case", MAP_CASE_NAMES)
def test_map_kernel_sums_of_attacked_items(case, sets):
    """yag_map_kernel on operands aimed where rint(d * fl(1 / res)) and rint(d / res) part: both passes' sum volumes are the rule's as
    written, with the (item, angle) blocks split (a call of two items) and whole (a call of 48), and pair by pair."""
    from yag_slam_amd.scan_matching import ScanMatcher
    a = attacked_map(case, sets)
    spec = R.MAP_CASES[case]
    assert a["counters"]["sets_kernel_items" if sets else "map_kernel_items"] == 2 and a["counters"]["sets_fallback_items" if sets else "map_fallback_items"] == 0
    for i, it in enumerate(a["items"]):
        assert it["f0"]["kind"] == (2 if sets else 1) and it["f0"]["map_split"] > 1
        # the band: positions where product and quotient round differently and the two cells hold different bytes.  It is required of the
        # kernel's coarse pass, whose operands do not depend on the ranges and so stay where they were aimed.  The fine pass of a map or
        # set call is centred on the coarse mean, and against a lattice of single cells that mean often averages several tied
        # hypotheses: the last round's small moves can shift it, and the fine operands with it.  What the fine pass met is printed (on
        # the 5 cm cases over a hundred positions, on the 1 cm ones between none and 26); its sums are compared either way.
        counts = {}
        for p in ("f0", "f1"):
            counts[p] = R.rint_div_count(it[p], it["grid"])
            print(case, "sets" if sets else "map", "item", i, p, "product != quotient at", counts[p][1], "positions,", counts[p][0], "on differing bytes")
        if R.rint_div_reachable(spec):
            assert counts["f0"][0] >= R.NEED, (i, counts)
        else:
            assert counts["f0"][1] == 0 and counts["f1"][1] == 0, (i, counts)
        assert np.array_equal(it["sums0"], it["want0"]), (i, int((it["sums0"] != it["want0"]).sum()))
        assert np.array_equal(it["sums1"], it["want1"]), (i, int((it["sums1"] != it["want1"]).sum()))
    # a call wide enough that a block takes all the points of its (item, angle)
    wide = a["run"](a["queries"], n=48)
    for it, w in zip(a["items"], wide):
        assert w["f0"]["map_split"] == 1
        assert _frame_equal(w["f0"], it["f0"]) and _frame_equal(w["f1"], it["f1"])
        assert np.array_equal(w["sums0"], it["want0"]) and np.array_equal(w["sums1"], it["want1"])
        assert (w["result"].response, w["result"].covariance) == (it["result"].response, it["result"].covariance)
    # pair by pair: the rule as written on the device (sets: option 46 = 0; maps: the single call, which has no other form)
    if sets:
        slow = ScanMatcher(a["cfg"], semantics="yagpy")
        slow.debug_option(46, 0)
        ref = a["run"](a["queries"], matcher=slow)
        assert slow.debug_counters()["sets_fallback_items"] == 2
    else:
        ref = []
        for q in a["queries"]:
            r = a["matcher"].match_scan_sets_with_map(a["map"], a["corner"][0], a["corner"][1], [q], True, True, coarse=a["coarse"])
            ref += _read_items(a["matcher"], [r], 1, lambda i: a["bytes"])
    for it, w in zip(a["items"], ref):
        assert _frame_equal(w["f0"], it["f0"]) and _frame_equal(w["f1"], it["f1"])
        assert np.array_equal(w["sums0"], it["want0"]) and np.array_equal(w["sums1"], it["want1"])
        assert (w["result"].response, w["result"].covariance) == (it["result"].response, it["result"].covariance)
