"""Alternatives on the device: ScanMatcher.locate_in_map(places=K) and a MapLocalizer that starts with K places and follows
them all.  The room of tests/test_gpu_locate.py is itself ambiguous: a rectangular room has a twin
pose half a turn away, which the boxes inside tell from the truth only by degrees."""
import math

import pytest

pytestmark = pytest.mark.gpu

from tests import locate_ref as R  # noqa: E402

CFG = dict(resolution=R.ROOM_RES, smear_deviation=R.ROOM_RES)
STEP = 2 * math.pi / R.ROOM_ANGLES
OX, OY = R.ROOM_ORIGIN
TWIN = (8.0 - R.ROOM_TRUTH[0], 6.0 - R.ROOM_TRUTH[1], R.ROOM_TRUTH[2] + math.pi)
KW = dict(n_angles=R.ROOM_ANGLES, point_stride=6)
MOTION = (0.15, 0.05, 0.03)
# the tracker's search on this 0.1 m map (its default lattice is laid out for 0.05 m cells): the polish's own
COARSE = dict(xy_search=2 * R.ROOM_RES, xy_step=R.ROOM_RES / 4, angle_search=STEP, angle_step=STEP / 20, grid_resolution=R.ROOM_RES)


def _wrap(a):
    return (a + math.pi) % (2 * math.pi) - math.pi


def _truth(t):
    return tuple(R.ROOM_TRUTH[i] + t * MOTION[i] for i in range(3))


def _scan(t, pose=(0.0, 0.0, 0.0)):
    from yag_slam_amd import synth
    return synth.resident_scan(synth.Scene().scan_ranges(_truth(t), index=950 + t), pose)


def _odom(start, t):
    """the odometry pose of scan t for a robot whose scan 0 has the odometry pose `start`: the true motion, composed"""
    t0, tt = _truth(0), _truth(t)
    c, s = math.cos(-t0[2]), math.sin(-t0[2])
    rel = (c * (tt[0] - t0[0]) - s * (tt[1] - t0[1]), s * (tt[0] - t0[0]) + c * (tt[1] - t0[1]), tt[2] - t0[2])
    c, s = math.cos(start[2]), math.sin(start[2])
    return (start[0] + c * rel[0] - s * rel[1], start[1] + s * rel[0] + c * rel[1], start[2] + rel[2])


def _xyz(p):
    return (p.x, p.y, p.euler[-1])


class _Ctx(object):
    pass


@pytest.fixture(scope="module")
def ctx():
    from yag_slam_amd import synth
    from yag_slam_amd.scan_matching import ScanMatcher
    c = _Ctx()
    c.m = ScanMatcher(CFG, semantics="yagpy")
    c.room = c.m.correlation_grid_from_occupancy(R.room_image(synth.Scene()), occupied_value=0)
    yield c
    c.room.close()
    c.m.close()


def test_locate_in_map_with_two_places_finds_the_truth_and_its_twin(ctx):
    r = ctx.m.locate_in_map(ctx.room, OX, OY, [_scan(0)], places=2, **KW)
    cands, places = r.meta["candidates"], r.meta["places"]
    print("located", [(c.score, _xyz(c.pose)) for c in cands], "polished", [(p.response, _xyz(p.best_pose[0])) for p in places],
          "ambiguity", r.meta["ambiguity"])
    assert len(cands) == 2 == len(places)
    for c, want in zip(cands, (R.ROOM_TRUTH, TWIN)):  # before the polish: within one cell and half a heading step
        assert abs(c.pose.x - want[0]) <= R.ROOM_RES + 1e-9 and abs(c.pose.y - want[1]) <= R.ROOM_RES + 1e-9
        assert abs(_wrap(c.pose.euler[-1] - want[2])) <= STEP / 2
    for p, want in zip(places, (R.ROOM_TRUTH, TWIN)):
        q = p.best_pose[0]
        assert math.hypot(q.x - want[0], q.y - want[1]) <= 2 * R.ROOM_RES and abs(_wrap(q.euler[-1] - want[2])) <= STEP
    ranked = sorted(p.response for p in places)
    assert r.meta["ambiguity"] == ranked[0] / ranked[1] and 0.0 < r.meta["ambiguity"] < 1.0
    assert r.response == ranked[1] and _xyz(r.best_pose[0]) == _xyz(places[r.meta["polished_index"]].best_pose[0])
    one = ctx.m.locate_in_map(ctx.room, OX, OY, [_scan(0)], places=1, **KW)
    assert len(one.meta["places"]) == 1 and one.meta["ambiguity"] == 0.0
    assert _xyz(one.meta["candidates"][0].pose) == _xyz(cands[0].pose)


def test_localizer_follows_both_places_until_the_evidence_leaves_one(ctx):
    from yag_slam_amd.mapping import MapLocalizer
    GAP, MAX_LOST, MERGE = 0.3, 8, (0.2, 0.1)
    loc = MapLocalizer(ctx.m, ctx.room, OX, OY, coarse=COARSE, evidence_gap=GAP, max_lost=MAX_LOST)
    first = _scan(0)
    loc.start(first, places=2, **KW)
    assert loc.ambiguous and [a.place for a in loc.alternatives] == [0, 1] and all(a.evidence == 0.0 and a.lost == 0 for a in loc.alternatives)
    assert loc.merge == MERGE
    start = _xyz(first.odom_pose)
    assert start == _xyz(first.corrected_pose) and math.hypot(start[0] - R.ROOM_TRUTH[0], start[1] - R.ROOM_TRUTH[1]) <= 0.15
    evidence, lost = {0: 0.0, 1: 0.0}, {0: 0, 1: 0}
    scans, collapsed_at = [first], None
    for t in range(1, 11):
        s = _scan(t, _odom(start, t))
        scans.append(s)
        before = loc.alternatives
        was_ambiguous = loc.ambiguous
        r = loc.process_scan(s)
        if was_ambiguous:  # the five-step rule, recomputed from the responses the device returned
            for a in before:
                evidence[a.place] += a.results[-1].response
                lost[a.place] = 0 if a.results[-1].meta["accepted"] else lost[a.place] + 1
            lead = max(before, key=lambda a: (evidence[a.place], -a.place))
            alive = [a for a in before if a is lead or not (evidence[lead.place] - evidence[a.place] >= GAP or lost[a.place] >= MAX_LOST)]
            kept = [a for a in alive if not any(
                evidence[b.place] > evidence[a.place] and
                math.hypot(a.last.corrected_pose.x - b.last.corrected_pose.x, a.last.corrected_pose.y - b.last.corrected_pose.y) <= MERGE[0] and
                abs(_wrap(a.last.corrected_pose.euler[-1] - b.last.corrected_pose.euler[-1])) <= MERGE[1] for b in alive)]
            print("step", t, "responses", [(a.place, a.results[-1].response) for a in before], "evidence", evidence, "alive", [a.place for a in kept])
            assert [(a.place, a.evidence, a.lost) for a in loc.alternatives] == [(a.place, evidence[a.place], lost[a.place]) for a in kept]
            assert loc.leader is lead and _xyz(s.corrected_pose) == _xyz(lead.last.corrected_pose)
            assert loc.lost == lost[lead.place] and r is lead.results[-1] and loc.results[-1] is r
            if not loc.ambiguous and collapsed_at is None:
                collapsed_at = t
        q, want = s.corrected_pose, _truth(t)
        assert math.hypot(q.x - want[0], q.y - want[1]) <= 0.15 and abs(_wrap(q.euler[-1] - want[2])) <= 0.1, (t, _xyz(q), want)
        if t == 8:
            assert not loc.ambiguous and [a.place for a in loc.alternatives] == [0], "the twin is still followed after eight steps"
    assert collapsed_at is not None and collapsed_at <= 8
    # after the collapse every step is the step of a plain localizer started at the survivor's pose on fresh copies of the scans
    assert len(loc.results) == 10
    plain = MapLocalizer(ctx.m, ctx.room, OX, OY, coarse=COARSE)
    s0 = _scan(collapsed_at, _xyz(scans[collapsed_at].odom_pose))
    s0.corrected_pose = scans[collapsed_at].corrected_pose
    plain.start(s0)
    for t in range(collapsed_at + 1, 11):
        f = _scan(t, _xyz(scans[t].odom_pose))
        r = plain.process_scan(f)
        mine = loc.results[t - 1]
        assert _xyz(f.corrected_pose) == _xyz(scans[t].corrected_pose) and r.response == mine.response, t
        assert _xyz(r.best_pose) == _xyz(mine.best_pose) and r.meta["accepted"] == mine.meta["accepted"]
    assert plain.lost == loc.lost


def test_a_localizer_started_without_places_is_the_plain_one(ctx):
    """the MapLocalizer route against the calls it has always made, written out: locate_in_map, then one track_in_map per step"""
    from yag_slam_amd.mapping import MapLocalizer
    from yag_slam_amd.transform import Transform
    loc = MapLocalizer(ctx.m, ctx.room, OX, OY, coarse=COARSE)
    first = _scan(0)
    res = loc.start(first, **KW)
    assert loc.alternatives == [] and not loc.ambiguous and loc.leader is None
    other = _scan(0)
    res2 = ctx.m.locate_in_map(ctx.room, OX, OY, [other], **KW)
    p = res2.best_pose[0]
    other.odom_pose = Transform(p.x, p.y, 0.0, p.euler[-1])
    other.corrected_pose = Transform(p.x, p.y, 0.0, p.euler[-1])
    assert res.response == res2.response and _xyz(first.corrected_pose) == _xyz(other.corrected_pose) and "places" not in res.meta
    start, last = _xyz(first.odom_pose), other
    for t in range(1, 4):
        a, b = _scan(t, _odom(start, t)), _scan(t, _odom(start, t))
        ra = loc.process_scan(a)
        rb, done = ctx.m.track_in_map(ctx.room, OX, OY, [last, b], 1, True, True, COARSE, 0.0)
        assert done == 2 and _xyz(a.corrected_pose) == _xyz(b.corrected_pose) and ra.response == rb[1].response
        assert _xyz(ra.best_pose) == _xyz(rb[1].best_pose) and not loc.ambiguous
        last = b
