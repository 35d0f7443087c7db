"""The branches of the finish stage that the injected volumes of tests/test_gpu_finish.py do not reach, in all three of its
forms -- fine_kernel + final_kernel, finish_kernel<1024>, finish_kernel<256> (debug options 6 and 11) -- on real matches of
the cfg2 scans on the default lattice: the generic fine lattice (Karto's row pitch in force, so the 3 x 3 block read is
off), a query without a reading, and a device-chained step finished by the one-block kernel."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from tests.util import PlainScan, cfg2_scans  # noqa: E402

FORMS = ((0, 0), (2, 1024), (2, 256))
NAMES = ("pair", "finish<1024>", "finish<256>")


def _native(plain):
    from yag_slam_amd.models import LocalizedRangeScan
    p = plain.corrected_pose
    return LocalizedRangeScan(plain.ranges, plain.min_angle, plain.max_angle, plain.angle_increment,
                              plain.min_range, plain.max_range, plain.range_threshold, p.x, p.y, p.euler[-1])


def _records(m, query, base, refine, regather=(0,)):
    """one refined match per (form, forced re-gather): the result and its bytes, fine sums included"""
    out = []
    for force in regather:
        for (form, threads), name in zip(FORMS, NAMES):
            m.debug_option(6, form)
            m.debug_option(11, threads)
            m.debug_option(49, force)
            r = m.match_scan(query, base, True, refine)
            bp = r.best_pose
            rec = np.array([r.response, bp.x, bp.y, bp.euler[-1]] + [v for row in r.covariance for v in row]).tobytes()
            if refine and r.meta["n_query_points"]:
                rec += m.debug_sums(1, dims=r.meta["fine_dims"]).tobytes()
            out.append((name + (" forced" if force else ""), r, rec))
    m.debug_option(49, 0)
    return out


def _assert_one_answer(recs):
    differ = [n for n, _, rec in recs if rec != recs[0][2]]
    assert not differ, "results differ from the pair's in: %s" % ", ".join(differ)


@pytest.mark.parametrize("pose", [(3.0, 3.0, 0.0), (3.02, 2.97, 0.4)])
def test_generic_fine_lattice_in_all_three_forms(pose):
    """the query of test_query_reading_beyond_the_matcher_threshold_is_answered_like_karto: a reading beyond the matcher's
    range threshold puts Karto's row pitch in force, and every form gathers the fine lattice cell by cell; with the
    re-gather forced the angular covariance gathers it once more.  One answer, and it is the oracle's"""
    from oracle import oracle as orc
    from yag_slam_amd.scan_matching import ScanMatcher
    q, base = cfg2_scans()
    cfg = dict(range_threshold=4.0)
    far = PlainScan(q.ranges, q.min_angle, q.angle_increment, q.min_range, 20.0, pose)
    assert np.nanmax(q.ranges) > 4.0
    o = orc.Oracle(cfg, "karto")
    ro = o.match_scan(far, base[:3], True, True)
    m = ScanMatcher(cfg)
    m.debug_option(12, 1)
    recs = _records(m, _native(far), [_native(b) for b in base[:3]], True, regather=(0, 1))
    assert len(recs) == 6
    _assert_one_answer(recs)
    r = recs[0][1]
    assert np.array_equal(m.debug_sums(1, dims=r.meta["fine_dims"]), o.sums(1)), "fine sums differ"
    assert abs(r.response - ro["response"]) <= 1e-12
    np.testing.assert_allclose([r.best_pose.x, r.best_pose.y, r.best_pose.euler[-1]], ro["pose"], rtol=0, atol=1e-9)
    np.testing.assert_allclose(np.array(r.covariance), ro["cov"], rtol=1e-9, atol=1e-15)
    m.close()


@pytest.mark.parametrize("refine", [True, False])
def test_no_readings_in_all_three_forms(refine):
    """MatchScan: "scan has no readings; cannot do scan matching": the pose as it came, the maximum variance, four angle
    steps squared, response 0 -- from every form, and from the oracle"""
    from oracle import oracle as orc
    from yag_slam_amd.scan_matching import ScanMatcher
    q, base = cfg2_scans()
    pose = (3.01, 2.98, 0.03)
    blind = PlainScan(np.full(len(q.ranges), 99.0), q.min_angle, q.angle_increment, q.min_range, 20.0, pose)
    ro = orc.Oracle(None, "karto").match_scan(blind, base, True, refine)
    assert ro["n_query_points"] == 0 and ro["hypotheses"] == 0
    m = ScanMatcher()
    query = _native(blind)
    pose = (query.corrected_pose.x, query.corrected_pose.y, query.corrected_pose.euler[-1])
    recs = _records(m, query, [_native(b) for b in base], refine)
    _assert_one_answer(recs)
    angle_res = orc.DEFAULT_CONFIG["coarse_angle_resolution"]
    for name, r, _ in recs:
        bp, cov = r.best_pose, np.array(r.covariance)
        assert r.meta["n_query_points"] == 0 and r.meta["hypotheses"] == 0, name
        assert (bp.x, bp.y, bp.euler[-1]) == pose, name
        assert r.response == 0.0, name
        want = np.zeros((3, 3))
        want[0, 0] = want[1, 1] = 500.0
        want[2, 2] = 4 * (angle_res * angle_res)
        assert np.array_equal(cov, want), name
    r = recs[0][1]
    assert abs(r.response - ro["response"]) <= 1e-12
    np.testing.assert_allclose([r.best_pose.x, r.best_pose.y, r.best_pose.euler[-1]], ro["pose"], rtol=0, atol=1e-9)
    np.testing.assert_allclose(np.array(r.covariance), ro["cov"], rtol=1e-9, atol=1e-15)
    m.close()


def test_chained_steps_through_the_one_block_kernel():
    """a device-chained sequence leaves each step's pose on the device for the next: whichever kernel finishes the step"""
    from yag_slam_amd import synth
    from yag_slam_amd.mapping import SequentialMapper
    from yag_slam_amd.scan_matching import ScanMatcher
    runs = []
    for form, threads in FORMS:
        _, scans = synth.trajectory_scans(4)
        m = ScanMatcher()
        m.debug_option(6, form)
        m.debug_option(11, threads)
        out = SequentialMapper(m).process_scans(scans, device_chain=True)
        assert out[0] is None and len(out) == 4
        assert m.sequence_stats()[1] == 0  # (no step faulted: every pose came down the chain)
        runs.append([(s.corrected_pose.x, s.corrected_pose.y, s.corrected_pose.euler[-1]) for s in scans] +
                    [(r.response,) + tuple(v for row in r.covariance for v in row) for r in out[1:]])
        m.close()
    assert runs[0] == runs[1] == runs[2]
