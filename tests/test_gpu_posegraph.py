"""The pose-graph optimiser on the device (include/yagmatch.h ym_graph_*, yag_slam_amd/posegraph.py) against the test-side
numpy / scipy solver tests/posegraph_ref.py: chi2 and the linear system, exact recovery, agreement of the optimised poses,
the band preconditioner's iteration counts, determinism, incremental use, the edges of the interface, and one loop closure
through LoopClosingMapper."""
import ctypes as C
import math

import numpy as np
import pytest

from tests import posegraph_ref as ref
from tests.test_posegraph_host import RECOVERY_LAMBDA

pytestmark = pytest.mark.gpu


def _optimizer(g, upto_nodes=None, upto_edges=None, cls=None):
    from yag_slam_amd.posegraph import PoseGraphOptimizer
    opt = (cls or PoseGraphOptimizer)()
    _add(opt, g, 0, len(g["poses"]) if upto_nodes is None else upto_nodes, 0, len(g["edges"]) if upto_edges is None else upto_edges)
    return opt


def _add(opt, g, n0, n1, e0, e1):
    for i in range(n0, n1):
        opt.add_node(*g["poses"][i], i)
    for m in range(e0, e1):
        opt.add_constraint(int(g["edges"][m, 0]), int(g["edges"][m, 1]), *g["means"][m], g["infos"][m])


def _pose_diff(a, b):
    d = np.array(a) - np.array(b)
    d[:, 2] = ref.wrap(d[:, 2])
    return np.abs(d).max()


@pytest.fixture(scope="module")
def graphs():
    """every graph the tests share, with the yardstick's answer (computed once, never modified)"""
    out = {}
    for name, g in (("ring64", ref.ring(64, noise=0.02, seed=1)), ("ring600", ref.ring(600, noise=0.02, seed=2)),
                    ("ring600x", ref.ring(600, noise=0.02, seed=2, extra=10)), ("grid5", ref.grid(5, 5, noise=0.02, seed=3))):
        poses, rep = ref.optimize(g)
        out[name] = dict(g, want=poses, want_report=rep)
    return out


@pytest.fixture(scope="module")
def ring600_run(graphs):
    """the 600-ring optimised once with the reference's call: (poses, report)"""
    opt = _optimizer(graphs["ring600"])
    rep = opt.compute(100, 1.0e-4, True, 1.0e-9, 50)
    return opt.nodes_xyt.copy(), rep


@pytest.mark.parametrize("name", ["ring64", "grid5"])
def test_chi2_and_linear_system(graphs, name):
    g = graphs[name]
    opt = _optimizer(g)
    want_chi2 = ref.chi2(g["poses"], g["edges"], g["means"], g["infos"])
    h, grad = ref.linear_system(g["poses"], g["edges"], g["means"], g["infos"])
    h = h.toarray()
    assert abs(opt.chi2() - want_chi2) <= 1e-9 * want_chi2
    chi2, diag, got_grad = opt.linearise()
    assert abs(chi2 - want_chi2) <= 1e-9 * want_chi2
    n = len(g["poses"])
    assert diag.shape == (n, 3, 3) and got_grad.shape == (n, 3)
    for i in range(n):  # node 0's row as assembled: holding it is the solver's business
        want = h[3 * i:3 * i + 3, 3 * i:3 * i + 3]
        assert np.abs(diag[i] - want).max() <= 1e-9 * np.abs(want).max(), i
        wg = grad[3 * i:3 * i + 3]
        assert np.abs(got_grad[i] - wg).max() <= 1e-9 * np.abs(wg).max(), i


def test_exact_recovery_of_the_noise_free_ring():
    g = ref.ring(64, noise=0.0, seed=1)
    opt = _optimizer(g)
    rep = opt.compute(100, RECOVERY_LAMBDA, True, 1.0e-9, 50)  # (RECOVERY_LAMBDA: see tests/test_posegraph_host.py)
    err = _pose_diff(opt.nodes_xyt, g["truth"])
    print("exact recovery: error %.3g, chi2 %.3g -> %.3g, %d steps" % (err, rep.chi2_initial, rep.chi2_final, rep.lm_steps))
    assert err <= 1e-9
    assert rep.chi2_final <= 1e-18 * rep.chi2_initial
    assert abs(opt.chi2() - rep.chi2_final) <= 1e-6 * rep.chi2_final + 1e-30


@pytest.mark.parametrize("name", ["ring64", "ring600", "ring600x"])
def test_agreement_with_the_yardstick(graphs, ring600_run, name):
    g = graphs[name]
    if name == "ring600":
        got, rep = ring600_run
    else:
        opt = _optimizer(g)
        rep = opt.compute(100, 1.0e-4, True, 1.0e-9, 50)
        got = opt.nodes_xyt
    want_chi2 = g["want_report"]["chi2_final"]
    err = _pose_diff(got, g["want"])
    print("%s: pose difference %.3g, chi2 %.12g against %.12g, steps %d / %d, cg %d, band %d"
          % (name, err, rep.chi2_final, want_chi2, rep.lm_steps, g["want_report"]["lm_steps"], rep.cg_iterations, rep.band))
    assert err <= 1e-9
    assert abs(rep.chi2_final - want_chi2) <= 1e-9 * want_chi2
    assert rep.chi2_initial > 100 * rep.chi2_final and rep.accepted >= 1


def test_the_band_does_its_work(graphs, ring600_run):
    got, rep = ring600_run
    assert rep.band == 3
    print("band 3: %d cg iterations over %d steps" % (rep.cg_iterations, rep.lm_steps))
    assert rep.cg_iterations <= 20 * rep.lm_steps


def test_block_jacobi_reaches_the_same_answer(graphs, ring600_run):
    got, rep = ring600_run
    opt = _optimizer(graphs["ring600"])
    opt.band = 0
    rep0 = opt.compute(100, 1.0e-4, True, 1.0e-9, 50)
    print("band 0: %d cg iterations over %d steps" % (rep0.cg_iterations, rep0.lm_steps))
    assert rep0.band == 0 and rep0.cg_iterations > 20 * rep0.lm_steps  # (the out-of-band products did the work)
    assert _pose_diff(opt.nodes_xyt, got) <= 1e-9
    assert _pose_diff(opt.nodes_xyt, graphs["ring600"]["want"]) <= 1e-9


def test_capped_solves_never_raise_chi2(graphs):
    opt = _optimizer(graphs["ring64"])
    chi2 = [opt.chi2()]
    accepted = 0
    for _ in range(12):  # one Levenberg-Marquardt step a call (lambda starts again at 1e-4 each time)
        rep = opt.compute(1, 1.0e-4, False, 1.0e-9, 5)
        assert rep.lm_steps <= 1 and rep.cg_iterations <= 5
        assert rep.chi2_initial == chi2[-1]
        assert rep.chi2_final <= chi2[-1]
        if rep.accepted:
            assert rep.chi2_final < chi2[-1]
        accepted += rep.accepted
        chi2.append(rep.chi2_final)
        assert opt.chi2() == rep.chi2_final
    assert accepted >= 3 and chi2[-1] < 0.5 * chi2[0]


def test_two_fresh_handles_give_identical_bytes(graphs, ring600_run):
    got, _ = ring600_run
    opt = _optimizer(graphs["ring600"])
    opt.compute(100, 1.0e-4, True, 1.0e-9, 50)
    assert opt.nodes_xyt.tobytes() == got.tobytes()


def test_incremental_use_equals_one_upload(graphs):
    g = graphs["ring64"]
    # the instalments: nodes / edges known after each (every edge's nodes exist when it is added)
    order = np.argsort(g["edges"].max(axis=1), kind="stable")
    g = dict(g, edges=g["edges"][order], means=g["means"][order], infos=g["infos"][order])
    cuts_n = [20, 45, 64]
    cuts_e = [int((g["edges"].max(axis=1) < n).sum()) for n in cuts_n]
    a = _optimizer(g, 0, 0)
    n0 = e0 = 0
    for k, (n1, e1) in enumerate(zip(cuts_n, cuts_e)):
        _add(a, g, n0, n1, e0, e1)
        n0, e0 = n1, e1
        if k < 2:
            a.compute(100, 1.0e-4, True, 1.0e-9, 50)
    before = a.nodes_xyt.copy()
    assert not np.array_equal(before[:45], g["poses"][:45])  # the first two computes moved the early nodes
    rep_a = a.compute(100, 1.0e-4, True, 1.0e-9, 50)
    b = _optimizer(dict(g, poses=before))
    rep_b = b.compute(100, 1.0e-4, True, 1.0e-9, 50)
    assert a.nodes_xyt.tobytes() == b.nodes_xyt.tobytes()
    assert (rep_a.lm_steps, rep_a.cg_iterations, rep_a.chi2_final) == (rep_b.lm_steps, rep_b.cg_iterations, rep_b.chi2_final)


def test_edges_of_the_interface():
    from yag_slam_amd import _capi
    from yag_slam_amd.posegraph import PoseGraphOptimizer
    # the heading residual across +-pi: 3.1 -> -3.1 is a turn of 2 pi - 6.2, not of -6.2
    opt = PoseGraphOptimizer()
    opt.add_node(0.0, 0.0, 3.1, 0)
    opt.add_node(0.0, 0.0, -3.1, 1)
    opt.add_constraint(0, 1, 0.0, 0.0, 0.0, np.diag([1.0, 1.0, 2.0]))
    want = 2.0 * (2 * math.pi - 6.2) ** 2
    assert abs(opt.chi2() - want) <= 1e-9 * want
    rep = opt.compute()
    assert rep.chi2_final <= 1e-18 * rep.chi2_initial
    assert abs(float(ref.wrap(opt.nodes[1].yaw - 3.1))) <= 1e-9 and opt.nodes[0].yaw == 3.1
    # one node; no constraints
    one = PoseGraphOptimizer()
    one.add_node(1.0, 2.0, 0.5, 0)
    rep = one.compute()
    assert (rep.lm_steps, rep.cg_iterations, rep.chi2_final) == (0, 0, 0.0) and one.chi2() == 0.0
    assert (one.nodes[0].x, one.nodes[0].y, one.nodes[0].yaw) == (1.0, 2.0, 0.5)
    one.add_node(2.0, 2.0, 0.5, 1)
    rep = one.compute()
    assert rep.lm_steps == 0 and len(one.nodes) == 2 and one.nodes[1].x == 2.0
    # the C entry refuses an index out of range with a code and a text
    L = _capi.lib()
    h = L.ym_graph_create(0)
    assert h
    try:
        xyt = np.zeros((2, 3))
        dp, ip = C.POINTER(C.c_double), C.POINTER(C.c_int32)
        assert L.ym_graph_add_nodes(h, xyt.ctypes.data_as(dp), 2) == 0
        ft = np.array([[0, 2]], dtype=np.int32)
        mean, info = np.zeros((1, 3)), np.eye(3).reshape(1, 9).copy()
        rc = L.ym_graph_add_constraints(h, ft.ctypes.data_as(ip), mean.ctypes.data_as(dp), info.ctypes.data_as(dp), 1)
        assert rc == -1 and "out of range" in _capi.last_error()
        ft[0] = (1, 1)
        assert L.ym_graph_add_constraints(h, ft.ctypes.data_as(ip), mean.ctypes.data_as(dp), info.ctypes.data_as(dp), 1) == -1
        assert "itself" in _capi.last_error()
        n, m = C.c_int32(), C.c_int32()
        assert L.ym_graph_size(h, C.byref(n), C.byref(m)) == 0 and (n.value, m.value) == (2, 0)
        assert L.ym_graph_get_poses(h, 1, xyt.ctypes.data_as(dp), 2) == -1 and "out of range" in _capi.last_error()
    finally:
        L.ym_graph_destroy(h)


def square_loop(n_side=10, step=0.5, drift=(0.004, 0.002, 0.003)):
    """ground-truth poses of one lap of a square (heading along the side) and the drifting odometry over it"""
    truth = []
    for side in range(4):
        th = side * math.pi / 2
        x0, y0 = [(0, 0), (1, 0), (1, 1), (0, 1)][side]
        for k in range(n_side):
            truth.append([step * n_side * x0 + step * k * math.cos(th), step * n_side * y0 + step * k * math.sin(th), float(ref.wrap(th))])
    truth = np.array(truth)
    odom = [truth[0]]
    for i in range(1, len(truth)):
        odom.append(ref.compose(odom[-1], ref.relative(truth[i - 1], truth[i]) + np.array(drift)))
    return truth, np.array(odom)


def run_square_loop(optimizer):
    """LoopClosingMapper with stub matchers over the square: sequential matches return the odometry prior, the loop
    matcher passes every chain, the closing fine match returns the true pose.  Returns (mapper, truth, index of the scan
    that closed the loop or None)."""
    from collections import namedtuple
    from yag_slam_amd.mapping import LoopClosingMapper
    from yag_slam_amd.models import LocalizedRangeScan
    from yag_slam_amd.transform import Transform
    R = namedtuple("R", "best_pose response covariance meta")
    cov = [[0.01, 0, 0], [0, 0.01, 0], [0, 0, 0.005]]
    truth, odom = square_loop()
    state = {"i": 0}

    class Seq:
        def match_scan(self, q, base, pen, fine):
            if not pen:  # the fine stage of a closure: the true pose
                t = truth[state["i"]]
                return R(Transform(t[0], t[1], 0, t[2]), 0.9, cov, {})
            p = q.corrected_pose
            return R(Transform(p.x, p.y, 0, p.euler[-1]), 0.9, cov, {})

    class Loop:
        def match_scan_batch(self, q, chains, pen, fine):
            return [R(q.corrected_pose, 0.8, cov, {}) for _ in chains], None

    mp = LoopClosingMapper(Seq(), Loop(), loop_search_dist=3.0, loop_search_min_chain_size=3, optimizer=optimizer)
    for i in range(len(truth)):
        state["i"] = i
        s = LocalizedRangeScan([1.0] * 5, -1, 1, 0.5, 0, 10, 5, 0, 0, 0)
        s.odom_pose = Transform(odom[i][0], odom[i][1], 0, odom[i][2])
        _, closed = mp.process_scan(s)
        if closed:
            return mp, truth, i
    return mp, truth, None


def test_a_closure_through_the_mapper_reposes_every_vertex():
    from yag_slam_amd.posegraph import PoseGraphOptimizer

    class Recording(PoseGraphOptimizer):
        def compute(self, *args):
            self.before = self.nodes_xyt.copy()
            self.calls = getattr(self, "calls", 0) + 1
            return super().compute(*args)

    opt = Recording()
    mp, truth, closed_at = run_square_loop(opt)
    assert closed_at is not None and closed_at >= 30, closed_at
    assert opt.calls == 1 and len(opt.nodes) == len(mp.scans) == closed_at + 1
    after = opt.nodes_xyt
    for s, row in zip(mp.scans, after):
        p = s.corrected_pose
        assert (p.x, p.y) == (row[0], row[1]) and abs(float(ref.wrap(p.euler[-1] - row[2]))) < 1e-12
    edges = np.array([(f, t) for f, t, _, _ in mp.constraints], dtype=np.int32)
    means = np.array([(m.x, m.y, m.euler[-1]) for _, _, m, _ in mp.constraints])
    infos = np.array([np.linalg.inv(np.array(c)) for _, _, _, c in mp.constraints])
    chi_before, chi_after = ref.chi2(opt.before, edges, means, infos), ref.chi2(after, edges, means, infos)
    end_before = np.hypot(*(opt.before[-2, :2] - truth[closed_at - 1, :2]))
    end_after = np.hypot(*(after[-2, :2] - truth[closed_at - 1, :2]))
    print("closure at %d: chi2 %.4g -> %.4g, error of the scan before the closing one %.3g -> %.3g m"
          % (closed_at, chi_before, chi_after, end_before, end_after))
    assert chi_after < chi_before
    assert abs(opt.last_report.chi2_final - chi_after) <= 1e-9 * chi_after
    assert end_after < end_before
    assert np.hypot(*(after[-1, :2] - truth[closed_at, :2])) < np.hypot(*(opt.before[-1, :2] - truth[closed_at, :2]))
    # the spatial index was rebuilt at the new poses
    assert sum(len(v) for v in mp.index.buckets.values()) == len(mp.scans)
    assert all(s in mp.index.buckets[mp.index.key(s.corrected_pose)] for s in mp.scans)
    moved = [s for s, old in zip(mp.scans, opt.before) if mp.index.key(s.corrected_pose) != (int(old[0] / 3.0), int(old[1] / 3.0))]
    assert moved, "no scan changed its bucket: the index check shows nothing"
