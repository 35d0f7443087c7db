"""Robust kernels and switchable constraints of the pose-graph optimiser on the device (DESIGN.md section 9.2;
ym_graph_set_robust / _enable / _edge_terms / _cost, PoseGraphOptimizer.set_robust / enable / disable / edge_terms / cost,
LoopClosingMapper(robust_closures=...)) against the numpy yardstick tests/posegraph_robust_ref.py.  The cases, and what the
yardstick itself shows on them, are those of tests/test_posegraph_robust_host.py."""
import ctypes as C

import numpy as np
import pytest

from tests import posegraph_ref as ref
from tests import posegraph_robust_ref as rr
from tests.test_posegraph_robust_host import E2E_KINDS, E2E_SEEDS, EDGE_COUNTS, e2e_cases, lin_graph

pytestmark = pytest.mark.gpu

NAME_OF = {v: k for k, v in rr.KIND_OF.items()}
CALL = (100, 1.0e-4, True, 1.0e-9, 50)  # the reference's compute


def _optimizer(g, held=(), hold_all=False):
    """a fresh handle with the graph's nodes, edges, kinds, parameters and switches"""
    from yag_slam_amd.posegraph import PoseGraphOptimizer
    opt = PoseGraphOptimizer()
    for i, p in enumerate(g["poses"]):
        opt.add_node(p[0], p[1], p[2], i)
    kinds, params, enabled = rr.settings(g)
    for m, (a, b) in enumerate(g["edges"]):
        robust = (NAME_OF[int(kinds[m])], float(params[m])) if kinds[m] else None
        assert opt.add_constraint(int(a), int(b), *g["means"][m], g["infos"][m], robust=robust) == m
    if hold_all:
        opt.hold(range(len(g["poses"])))
    elif len(held):
        opt.hold(held)
    if not enabled.all():
        opt.disable(np.flatnonzero(~enabled))
    return opt


def _pose_diff(a, b):
    d = np.array(a) - np.array(b)
    d[:, 2] = ref.wrap(d[:, 2])
    return float(np.abs(d).max())


def _report(rep):
    return tuple(getattr(rep, name) for name in rep.__slots__)


@pytest.mark.parametrize("count", EDGE_COUNTS)
@pytest.mark.parametrize("family", ["ring", "banded"])
def test_cost_terms_and_linearisation(family, count):
    """1e-9 relative, the bound of test_gpu_posegraph.py::test_chi2_and_linear_system.  Every node is held: the cut graphs leave
    nodes whose only edge is a disabled one, which ym_graph_enable refuses for a free node, and nothing compared here depends
    on the held set."""
    g = lin_graph(family, count)
    opt = _optimizer(g, hold_all=True)
    poses, n = g["poses"], len(g["poses"])
    want_cost, want_chi2 = rr.cost(poses, g), rr.chi2(poses, g)
    want_s, want_w = rr.edge_terms(poses, g)
    h, grad = rr.linear_system(poses, g)
    h = h.toarray()
    cost, chi2 = opt.cost(), opt.chi2()
    s, w = opt.edge_terms()
    lin_cost, diag, got_grad = opt.linearise()
    print("%s %d: cost %.12g against %.12g, chi2 %.12g against %.12g, s and w differ by %.3g and %.3g relative"
          % (family, count, cost, want_cost, chi2, want_chi2, np.abs(s / want_s - 1).max(), np.abs(w[want_w > 0] / want_w[want_w > 0] - 1).max()))
    assert abs(cost - want_cost) <= 1e-9 * want_cost and abs(lin_cost - want_cost) <= 1e-9 * want_cost
    assert abs(chi2 - want_chi2) <= 1e-9 * want_chi2
    assert s.shape == w.shape == (count,)
    assert np.all(np.abs(s - want_s) <= 1e-9 * want_s) and np.all(np.abs(w - want_w) <= 1e-9 * want_w)
    assert (w[~rr.settings(g)[2]] == 0).all()
    assert diag.shape == (n, 3, 3) and got_grad.shape == (n, 3)
    for i in range(n):
        want = h[3 * i:3 * i + 3, 3 * i:3 * i + 3]
        assert np.abs(diag[i] - want).max() <= 1e-9 * np.abs(want).max(), i
        wg = grad[3 * i:3 * i + 3]
        assert np.abs(got_grad[i] - wg).max() <= 1e-9 * np.abs(wg).max(), i


def test_a_graph_without_robust_edges_keeps_its_bytes():
    """w = 1.0 and rho = s: three handles, identical poses and reports"""
    g = ref.ring(600, noise=0.02, seed=2)
    m = len(g["edges"])
    plain = _optimizer(g)
    never = _optimizer(dict(g, kinds=np.full(m, rr.HUBER), params=np.full(m, 1e150)))
    back = _optimizer(g)
    back.set_robust(range(m), ("cauchy", 2.0))
    assert back.cost() < 0.5 * back.chi2()  # the library has seen the kernels
    back.set_robust(range(m), None)
    back.disable([m - 1])
    _, w = back.edge_terms()
    assert w[m - 1] == 0.0 and (w[:m - 1] == 1.0).all()
    back.enable([m - 1])
    runs = []
    for opt in (plain, never, back):
        assert opt.cost() == opt.chi2()
        rep = opt.compute(*CALL)
        runs.append((opt.nodes_xyt.tobytes(), _report(rep)))
        s, w = opt.edge_terms()
        assert (w == 1.0).all() and opt.cost() == opt.chi2() == rep.chi2_final
    assert runs[0] == runs[1] == runs[2]
    assert runs[0][1][4] >= 5  # (accepted steps: the run did something)


@pytest.fixture(scope="module")
def device_runs():
    """{(n, share, kind or "plain" or "held"): (poses, report, w)} of the end-to-end cases on the device, each computed once"""
    cases, done = e2e_cases(), {}

    def run(n, share, kind):
        key = (n, share, kind)
        if key not in done:
            if kind == "held":
                gr, held = cases["held"][:2]
                opt = _optimizer(gr, held)
            else:
                opt = _optimizer(cases[n, share]["graph"] if kind == "plain" else cases[n, share]["robust"][kind][0])
            rep = opt.compute(*CALL)
            done[key] = (opt.nodes_xyt.copy(), rep, opt.edge_terms()[1])
            opt.close()
        return done[key]
    return run


@pytest.mark.parametrize("kind", E2E_KINDS)
@pytest.mark.parametrize("n,share", list(E2E_SEEDS))
def test_agreement_with_the_robust_yardstick(device_runs, n, share, kind):
    """1e-9 in the poses and 1e-9 relative in the final cost, the bounds of test_gpu_posegraph.py::test_agreement_with_the_yardstick"""
    gr, want, want_rep, _ = e2e_cases()[n, share]["robust"][kind]
    got, rep, _ = device_runs(n, share, kind)
    err = _pose_diff(got, want)
    print("%d / %g %s: pose difference %.3g, F %.12g against %.12g, steps %d / %d, cg %d, band %d"
          % (n, share, kind, err, rep.chi2_final, want_rep["chi2_final"], rep.lm_steps, want_rep["lm_steps"], rep.cg_iterations, rep.band))
    assert err <= 1e-9
    assert abs(rep.chi2_final - want_rep["chi2_final"]) <= 1e-9 * want_rep["chi2_final"]
    assert abs(rep.chi2_initial - want_rep["chi2_initial"]) <= 1e-9 * want_rep["chi2_initial"]
    assert (rep.lm_steps, rep.accepted, rep.status) == (want_rep["lm_steps"], want_rep["accepted"], want_rep["status"])


def test_agreement_with_some_nodes_held(device_runs):
    gr, held, want, want_rep, _ = e2e_cases()["held"]
    got, rep, _ = device_runs(None, None, "held")
    err = _pose_diff(got, want)
    print("held: pose difference %.3g, F %.12g against %.12g, steps %d / %d" % (err, rep.chi2_final, want_rep["chi2_final"], rep.lm_steps, want_rep["lm_steps"]))
    assert err <= 1e-9 and abs(rep.chi2_final - want_rep["chi2_final"]) <= 1e-9 * want_rep["chi2_final"]
    assert got[list(held)].tobytes() == gr["poses"][list(held)].tobytes()


@pytest.mark.parametrize("n,share", list(E2E_SEEDS))
def test_robust_closures_do_what_they_are_for(device_runs, n, share):
    """the margins the yardstick shows (test_posegraph_robust_host.py), on the device: the plain optimiser ends at least ten
    times further from the truth, and every wrong closure weighs less than every right one"""
    c = e2e_cases()[n, share]
    truth, closures, wrong = c["graph"]["truth"], c["closures"], c["wrong"]
    right = np.setdiff1d(closures, wrong)
    plain_err = rr.pose_error(device_runs(n, share, "plain")[0], truth)
    for kind in E2E_KINDS:
        poses, rep, w = device_runs(n, share, kind)
        err = rr.pose_error(poses, truth)
        print("%d / %g %s: error against truth plain %.3g, robust %.3g; w of wrong closures <= %.2g, of right ones >= %.2g"
              % (n, share, kind, plain_err, err, w[wrong].max(), w[right].min()))
        assert plain_err >= 10.0 * err
        assert w[wrong].max() < w[right].min()
        assert (np.delete(w, closures) == 1.0).all()  # odometry and chain edges stay plain


def test_disabling_the_wrong_closures_is_the_graph_without_them():
    c = e2e_cases()[40, 0.10]
    g, wrong = c["graph"], c["wrong"]
    keep = np.setdiff1d(np.arange(len(g["edges"])), wrong)
    without = _optimizer(dict(g, edges=g["edges"][keep], means=g["means"][keep], infos=g["infos"][keep]))
    rep0 = without.compute(*CALL)
    opt = _optimizer(g)
    opt.disable(wrong)
    s, w = opt.edge_terms()
    assert (w[wrong] == 0.0).all() and (s[wrong] > 0).all() and (np.delete(w, wrong) == 1.0).all()
    rep = opt.compute(*CALL)
    err = _pose_diff(opt.nodes_xyt, without.nodes_xyt)
    print("disabled against never added: pose difference %.3g, chi2 %.12g against %.12g" % (err, rep.chi2_final, rep0.chi2_final))
    assert err <= 1e-9 and abs(rep.chi2_final - rep0.chi2_final) <= 1e-9 * rep0.chi2_final
    assert abs(opt.chi2() - rep.chi2_final) <= 1e-12 * rep.chi2_final  # chi2() counts the enabled edges only


def test_disabling_the_only_edge_of_a_free_node_is_refused():
    from yag_slam_amd import _capi
    g = ref.ring(12, noise=0.02, seed=4)
    lone = len(g["poses"])  # one more node, hanging on one edge
    poses = np.concatenate([g["poses"], [[0.5, 0.5, 0.1]]])
    g = dict(g, poses=poses, edges=np.concatenate([g["edges"], [[3, lone]]]).astype(np.int32),
             means=np.concatenate([g["means"], [[0.1, 0.2, 0.0]]]), infos=np.concatenate([g["infos"], [np.eye(3) * 100.0]]))
    last = len(g["edges"]) - 1
    opt = _optimizer(rr.robust_on(g, [2, last], "cauchy", 2.0))
    before = (opt.cost(), opt.chi2(), [v.tobytes() for v in opt.edge_terms()])
    with pytest.raises(_capi.YmError, match="free node %d" % lone):
        opt.disable([0, last])  # (nothing of the call is applied: edge 0 stays enabled too)
    assert (opt.cost(), opt.chi2(), [v.tobytes() for v in opt.edge_terms()]) == before
    opt.hold([lone])  # a held node needs no constraint
    opt.disable([0, last])
    _, w = opt.edge_terms()
    assert w[0] == 0.0 and w[last] == 0.0 and opt.cost() < before[0]
    rep = opt.compute(*CALL)
    assert rep.accepted >= 1 and opt.nodes_xyt[lone].tobytes() == poses[lone].tobytes()


def test_the_c_entries_refuse_bad_arguments():
    from yag_slam_amd import _capi
    L = _capi.lib()
    h = L.ym_graph_create(0)
    assert h
    try:
        dp, ip = C.POINTER(C.c_double), C.POINTER(C.c_int32)
        xyt = np.array([[0.0, 0, 0], [1.0, 0, 0], [2.0, 0, 0]])
        assert L.ym_graph_add_nodes(h, xyt.ctypes.data_as(dp), 3) == 0
        ft = np.array([[0, 1], [1, 2]], dtype=np.int32)
        mean, info = np.array([[1.0, 0, 0], [1.5, 0, 0]]), np.tile(np.eye(3).reshape(1, 9), (2, 1))
        assert L.ym_graph_add_constraints(h, ft.ctypes.data_as(ip), mean.ctypes.data_as(dp), info.ctypes.data_as(dp), 2) == 0
        s, w = np.zeros(2), np.zeros(2)
        cost = C.c_double()

        def state():
            assert L.ym_graph_edge_terms(h, s.ctypes.data_as(dp), w.ctypes.data_as(dp)) == 0 and L.ym_graph_cost(h, C.byref(cost)) == 0
            return s.tobytes(), w.tobytes(), cost.value
        first = state()
        assert s.tolist() == [0.0, 0.25] and w.tolist() == [1.0, 1.0] and cost.value == 0.25
        e = lambda *v: np.array(v, dtype=np.int32).ctypes.data_as(ip)  # noqa: E731
        assert L.ym_graph_set_robust(h, e(0, 2), 2, 1, 1.0) == -1 and "out of range" in _capi.last_error()
        assert L.ym_graph_set_robust(h, e(-1), 1, 1, 1.0) == -1 and "out of range" in _capi.last_error()
        assert L.ym_graph_set_robust(h, e(0), 1, 4, 1.0) == -1 and "kind" in _capi.last_error()
        assert L.ym_graph_set_robust(h, e(0), 1, -1, 1.0) == -1 and "kind" in _capi.last_error()
        for p in (0.0, -1.0, float("nan"), float("inf")):
            assert L.ym_graph_set_robust(h, e(0), 1, 2, p) == -1 and "positive" in _capi.last_error()
        assert L.ym_graph_enable(h, e(2), 1, 0) == -1 and "out of range" in _capi.last_error()
        assert L.ym_graph_enable(h, e(0, 1), 2, 0) == -1 and "free node" in _capi.last_error()
        assert L.ym_graph_set_robust(h, None, 1, 1, 1.0) == -1 and L.ym_graph_edge_terms(h, None, w.ctypes.data_as(dp)) == -1
        assert L.ym_graph_cost(h, None) == -1
        assert state() == first  # nothing of a refused call was applied
        assert L.ym_graph_enable(h, e(0), 1, 0) == 0  # (node 1 keeps edge 1)
        assert state()[1:] == (np.array([0.0, 1.0]).tobytes(), 0.25)
        assert L.ym_graph_set_robust(h, e(1), 1, 2, 0.5) == 0  # cauchy(0.5) at s = 0.25: w = 1 / 2, rho = 0.25 log 2
        state()
        assert w.tolist() == [0.0, 0.5] and abs(cost.value - 0.25 * np.log(2.0)) <= 1e-15
    finally:
        L.ym_graph_destroy(h)


def test_two_fresh_handles_with_robust_edges_give_identical_bytes(device_runs):
    for n, share, kind in ((600, 0.03, "cauchy"), (40, 0.10, "geman_mcclure")):
        poses, rep, w = device_runs(n, share, kind)
        opt = _optimizer(e2e_cases()[n, share]["robust"][kind][0])
        again = opt.compute(*CALL)
        assert opt.nodes_xyt.tobytes() == poses.tobytes() and _report(again) == _report(rep)
        assert opt.edge_terms()[1].tobytes() == w.tobytes()


# ---- through the mapper
ROBUST = ("cauchy", 2.0)
COV = [[0.01, 0, 0], [0, 0.01, 0], [0, 0, 0.005]]


def _square_mapper(optimizer, **kw):
    """tests/test_gpu_posegraph.py's run_square_loop with the mapper's keywords passed on: the square lap up to its closure"""
    from collections import namedtuple
    from tests.test_gpu_posegraph import square_loop
    from yag_slam_amd.mapping import LoopClosingMapper
    from yag_slam_amd.models import LocalizedRangeScan
    from yag_slam_amd.transform import Transform
    R = namedtuple("R", "best_pose response covariance meta")
    truth, odom = square_loop()
    state = {"i": 0}

    class Seq:
        def match_scan(self, q, base, pen, fine):
            if not pen:  # the fine stage of a closure: the true pose
                t = truth[state["i"]]
                return R(Transform(t[0], t[1], 0, t[2]), 0.9, COV, {})
            p = q.corrected_pose
            return R(Transform(p.x, p.y, 0, p.euler[-1]), 0.9, COV, {})

    class Loop:
        def match_scan_batch(self, q, chains, pen, fine):
            return [R(q.corrected_pose, 0.8, COV, {}) for _ in chains], None

    mp = LoopClosingMapper(Seq(), Loop(), loop_search_dist=3.0, loop_search_min_chain_size=3, optimizer=optimizer, **kw)
    for i in range(len(truth)):
        state["i"] = i
        s = LocalizedRangeScan([1.0] * 5, -1, 1, 0.5, 0, 10, 5, 0, 0, 0)
        s.odom_pose = Transform(odom[i][0], odom[i][1], 0, odom[i][2])
        _, closed = mp.process_scan(s)
        if closed:
            return mp, i
    raise AssertionError("the square did not close")


def _mapper_graph(mp, poses, robust_edges):
    edges = np.array([(f, t) for f, t, _, _ in mp.constraints], dtype=np.int32)
    means = np.array([(m.x, m.y, m.euler[-1]) for _, _, m, _ in mp.constraints])
    infos = np.array([np.linalg.inv(np.array(c)) for _, _, _, c in mp.constraints])
    return rr.robust_on(dict(poses=np.array(poses), edges=edges, means=means, infos=infos), list(robust_edges), *ROBUST)


def test_the_mapper_ranks_and_drops_a_false_closure():
    """What "equals a mapper that never saw it, within 1e-9" is held to.  A `compute` stops when a kept step gains no more than
    1e-9 F, which leaves the poses short of the optimum by up to sqrt(2e-9 F / mu), mu the smallest eigenvalue of the free
    nodes' H: two runs that come to the same optimum from different poses differ by the stop rule, not by what was dropped (on
    the yardstick the mapper that never saw the false closure itself ends 1.4e-8 from the tightly converged optimum of this
    graph, the one that dropped it 4.6e-9, 1.8e-8 apart; further `run_opt` calls do not bring them under 2e-9, the floor of
    comparing F in fp64).  So the bound of 1e-9 is asked of the mapper that never saw the false closure taken to the poses the
    drop starts from -- the same graph but for a disabled constraint, the same start -- and the mapper that never left the
    clean poses is held to the reach of the stop rule, twice sqrt(2e-9 F / mu) from the yardstick's H."""
    from yag_slam_amd.posegraph import PoseGraphOptimizer
    from yag_slam_amd.transform import Transform
    clean, closed_at = _square_mapper(PoseGraphOptimizer(), robust_closures=ROBUST)
    assert len(clean.closures) == 1 and clean.closure_edges == [len(clean.constraints) - 1]
    (num, edge, s, w), = clean.closure_weights()
    assert (num, edge) == (closed_at, clean.closure_edges[0]) and w > 0.9
    opt = PoseGraphOptimizer()
    mp, _ = _square_mapper(opt, robust_closures=ROBUST)
    assert [(p.x, p.y) for p in (s.corrected_pose for s in mp.scans)] == [(p.x, p.y) for p in (s.corrected_pose for s in clean.scans)]
    # one false closure: scan 20 seen from scan 5 where it is not
    a, b = mp.scans[5], mp.scans[20]
    assert b.num not in mp.adjacent[a.num]
    seen = b.copy()
    seen.num = b.num
    seen.corrected_pose = Transform(b.corrected_pose.x + 1.5, b.corrected_pose.y - 1.0, 0, b.corrected_pose.euler[-1] + 0.3)
    assert mp.link_scans(a, seen, COV, robust=mp.robust_closures)
    false_edge = mp.last_edge
    assert false_edge == len(mp.constraints) - 1 and b.num in mp.adjacent[a.num]
    mp.closures.append((b.num, [a.num], None, None))
    mp.closure_edges.append(false_edge)
    start = opt.nodes_xyt.copy()
    mp.run_opt()
    bent_poses = opt.nodes_xyt.copy()
    bent = _pose_diff(bent_poses, clean.opt.nodes_xyt)
    # the yardstick's weights on that graph, from the same start
    g = _mapper_graph(mp, start, mp.closure_edges)
    want, _ = rr.optimize(g)
    _, w_ref = rr.edge_terms(want, g)
    weights = mp.closure_weights()
    print("closure weights %s; the yardstick's %s; the false closure bent the map by %.3g" % (weights, w_ref[mp.closure_edges], bent))
    assert [c[:2] for c in weights] == [(closed_at, clean.closure_edges[0]), (b.num, false_edge)]
    assert weights[1][3] < weights[0][3] and w_ref[false_edge] < w_ref[mp.closure_edges[0]]
    for (_, e, s, w) in weights:
        assert abs(w - w_ref[e]) <= 1e-6 * w_ref[e]
    max_weight = float(np.sqrt(w_ref[false_edge] * w_ref[mp.closure_edges[0]]))  # between the two, from the yardstick
    dropped = mp.drop_closures(max_weight)
    assert [c[:2] for c in dropped] == [(b.num, false_edge)] and mp.dropped_edges == {false_edge}
    assert len(mp.closures) == 1 and mp.closure_edges == clean.closure_edges
    assert b.num not in mp.adjacent[a.num] and a.num not in mp.adjacent[b.num]  # the pair can close again
    never, _ = _square_mapper(PoseGraphOptimizer(), robust_closures=ROBUST)
    never.opt.set_poses(bent_poses)
    never.run_opt()
    err = _pose_diff(opt.nodes_xyt, never.opt.nodes_xyt)
    g_clean = _mapper_graph(clean, clean.opt.nodes_xyt, clean.closure_edges)
    h, _ = rr.linear_system(g_clean["poses"], g_clean)
    mu = float(np.linalg.eigvalsh(h.toarray()[3:, 3:]).min())
    reach = 2.0 * np.sqrt(2e-9 * rr.cost(g_clean["poses"], g_clean) / mu)
    apart = _pose_diff(opt.nodes_xyt, clean.opt.nodes_xyt)
    print("after the drop: %.3g from the mapper that never saw the false closure (same start), %.3g from the one that stayed "
          "clean (the stop rule reaches %.3g; the false closure had bent the map by %.3g)" % (err, apart, reach, bent))
    assert err <= 1e-9
    assert apart <= reach < 1e-2 * bent
    for s_, row in zip(mp.scans, opt.nodes_xyt):
        assert (s_.corrected_pose.x, s_.corrected_pose.y) == (row[0], row[1])
    assert mp.drop_closures(max_weight) == []  # nothing left below it


def test_the_mapper_without_the_keyword_keeps_its_bytes():
    from tests.test_gpu_posegraph import run_square_loop
    from yag_slam_amd.posegraph import PoseGraphOptimizer
    old, _, closed_at = run_square_loop(PoseGraphOptimizer())
    new, new_closed_at = _square_mapper(PoseGraphOptimizer(), robust_closures=None)
    assert closed_at == new_closed_at
    assert old.opt.nodes_xyt.tobytes() == new.opt.nodes_xyt.tobytes()
    assert [len(c) for c in new.closures] == [4] and new.closure_edges == [len(new.constraints) - 1]
    (num, edge, s, w), = new.closure_weights()
    assert w == 1.0 and new.drop_closures(0.5) == []
