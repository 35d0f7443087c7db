"""tests/finish_ref.py -- the plain restatement of the finish stage the GPU tests compare against -- held against the C
oracle ("karto" semantics) on the suite's end-to-end inputs, and against answers written out by hand.  No GPU."""
import math

import numpy as np
import pytest

from tests import finish_ref as R
from tests.util import PlainScan, cfg2_scans, load_case


def _oracle_case(cfg, query, base, penalty, fine, loop=False):
    """the oracle's integer sums -> responses -> finish_ref, against the oracle's own response, pose and covariance at the
    tolerances of tests/test_gpu_parity.py (compare)"""
    from oracle import oracle as orc
    o = orc.Oracle(cfg, "karto", loop=loop)
    ro = o.match_scan(query, base, penalty, fine)
    assert ro["expansions"] == 0 and ro["n_query_points"] > 0
    full = dict(orc.DEFAULT_CONFIG_LOOP if loop else orc.DEFAULT_CONFIG)
    full.update(cfg or {})
    p = query.corrected_pose
    pose = (p.x, p.y, p.euler[-1])
    lc, lf = R.lattices(full)
    assert (lc["nx"], lc["ny"], lc["nt"]) == tuple(ro["coarse_dims"])
    nq, pen = ro["n_query_points"], R.penalties(full)
    assert R.grid_offset(full, pose) == o.grid_offset()
    resp = R.responses(o.sums(0), nq, lc, pose[2], penalty, pen)
    np.testing.assert_allclose(resp, o.responses(0), rtol=0, atol=1e-15)
    fin = None
    if fine:
        assert (lf["nx"], lf["ny"], lf["nt"]) == tuple(ro["fine_dims"])
        fin = dict(sums=o.sums(1), nq=nq, lat=lf, penalize=penalty, pen=pen, grid_off=R.grid_offset(full, pose),
                   scale=1.0 / full["resolution"])
    ref = R.finish_ref(resp, lc, pose, fine=fin)
    R.assert_margin(ref)
    assert ref["status"] == 0
    assert abs(ref["response"] - ro["response"]) <= 1e-12
    np.testing.assert_allclose(ref["pose"], ro["pose"], rtol=0, atol=1e-9)
    np.testing.assert_allclose(ref["cov"], ro["cov"], rtol=1e-9, atol=1e-15)
    return ref, ro


@pytest.mark.parametrize("penalty,fine", [(True, True), (False, True), (True, False), (False, False)])
def test_cfg2_default(penalty, fine):
    q, base = cfg2_scans()
    _oracle_case(None, q, base, penalty, fine)


@pytest.mark.parametrize("fine", [False, True])
def test_loop_config(fine):
    q, base = cfg2_scans()
    _oracle_case(None, q, base, False, fine, loop=True)


@pytest.mark.parametrize("name,penalty", [("small_pen1_fine1", True), ("small_dirty_rot", False)])
def test_small_lattice_goldens(name, penalty):
    c = load_case(name)
    _oracle_case(dict(c["cfg"], search_size=0.32), c["query"], c["base"], penalty, True)


def test_heading_across_the_wrap():
    from yag_slam_amd import synth
    scene = synth.Scene()
    mk = lambda r, p: PlainScan(r, synth.MIN_ANGLE, synth.ANGLE_INCREMENT, synth.MIN_RANGE, 20.0, p)
    poses = [(4.0, 3.0, 3.10 + 0.01 * i) for i in range(3)]
    base = [mk(scene.scan_ranges(p, index=220 + i), p) for i, p in enumerate(poses)]
    q = mk(scene.scan_ranges((4.02, 3.01, -3.12), index=230), (4.0, 3.0, 3.14))
    ref, ro = _oracle_case(None, q, base, True, True)
    assert abs(ref["pose"][2]) > 3.0  # (the answer lies at the wrap, on either side of it)


def test_zero_response_without_expansion():
    mk = lambda r, p: PlainScan(r, -0.5, 0.01, 0.05, 20.0, p)
    base = [mk(np.full(101, 2.0), (0.0, 0.0, 0.0))]
    q = mk(np.full(101, 2.0), (10.0, 10.0, 0.0))
    ref, ro = _oracle_case(dict(search_size=0.3, range_threshold=12.0, use_response_expansion=False), q, base, True, True)
    assert ref["response"] == 0.0 and ref["n_ties"] == 16 * 16 * 21 and ref["cov"][0, 0] == 500.0


# ---- volumes of a few cells, answers written out by hand: a 3 x 3 x 3 lattice of 2 cm and 0.1 rad steps
def _tiny(pose_heading):
    lat = R.lattice(0.02, 0.02, 0.1, 0.1)
    assert (lat["nx"], lat["ny"], lat["nt"]) == (3, 3, 3)
    return lat, np.zeros((3, 3, 3)), (1.0, 2.0, pose_heading)


def test_by_hand_two_ties():
    lat, v, pose = _tiny(0.3)
    v[1, 1, 0] = v[1, 1, 2] = 0.5  # x = 0.98 and 1.02 on the row y = 2, both at heading 0.3
    ref = R.finish_ref(v, lat, pose)
    R.assert_margin(ref)
    assert ref["n_ties"] == 2 and ref["response"] == 0.5 and ref["status"] == 0
    np.testing.assert_allclose(ref["pose"], (1.0, 2.0, 0.3), rtol=0, atol=1e-15)
    # members: the two cells; about the mean x = -+0.02, y = 0: vxx = 0.0004, vyy = 0 -> 0.1 * 0.02^2; both times 1 / 0.5
    np.testing.assert_allclose(ref["cov"], [[8e-4, 0, 0], [0, 8e-5, 0], [0, 0, 4 * 0.1 * 0.1]], rtol=1e-12, atol=1e-18)


def test_by_hand_three_ties_across_the_wrap():
    lat, v, pose = _tiny(3.1)  # headings 3.0, 3.1 and 3.2 = -3.083...: their circular mean is 3.1, their arithmetic mean is not
    v[0, 0, 0] = v[1, 0, 1] = v[2, 2, 1] = 0.5  # (x, y) = (0.98, 1.98), (1.0, 1.98), (1.0, 2.02)
    ref = R.finish_ref(v, lat, pose)
    R.assert_margin(ref)
    assert ref["n_ties"] == 3 and ref["response"] == 0.5
    np.testing.assert_allclose(ref["pose"], (1.0 - 0.02 / 3, 2.0 - 0.02 / 3, 3.1), rtol=0, atol=1e-14)
    # about the mean the members lie at x = -0.04/3, 0.02/3, 0.02/3 and y = -0.04/3, -0.04/3, 0.08/3, weights 0.5 of 1.5
    vxx, vxy, vyy = 0.0024 / 27, 0.0024 / 27, 0.0096 / 27
    np.testing.assert_allclose(ref["cov"], [[2 * vxx, 2 * vxy, 0], [2 * vxy, 2 * vyy, 0], [0, 0, 0.04]], rtol=1e-12, atol=1e-18)


def test_by_hand_sharp_peak_is_clamped():
    lat, v, pose = _tiny(-0.2)
    v[:] = 0.25
    v[2, 1, 1] = 1.25  # one cell above everything else by more than 0.1, and above 1
    ref = R.finish_ref(v, lat, pose)
    R.assert_margin(ref)
    assert ref["n_ties"] == 1 and ref["coarse_best"] == 1.25 and ref["response"] == 1.0
    np.testing.assert_allclose(ref["pose"], (1.0, 2.0, -0.2 + 0.1), rtol=0, atol=1e-15)
    # a single member at the mean: both variances are zero and become 0.1 * step^2 = 4e-5, times 1 / 1.25
    np.testing.assert_allclose(ref["cov"], [[3.2e-5, 0, 0], [0, 3.2e-5, 0], [0, 0, 0.04]], rtol=1e-12, atol=1e-18)


def test_margin_reports_a_comparison_at_its_threshold():
    lat, v, pose = _tiny(0.0)
    v[1, 1, 1] = 0.5
    v[1, 0, 0] = 0.5 - 1e-6 - 1e-12  # a hair outside the tie tolerance
    ref = R.finish_ref(v, lat, pose)
    assert ref["n_ties"] == 1 and ref["margin"] < 1e-11
    with pytest.raises(AssertionError):
        R.assert_margin(ref)
    v[1, 0, 0] = 0.5 - 0.1 + 2.0 ** -40  # a hair inside the covariance's membership
    ref = R.finish_ref(v, lat, pose)
    assert ref["margin"] < 1e-11 and ref["cov"][0, 1] != 0.0
    assert math.isfinite(ref["cov"][0, 0])
