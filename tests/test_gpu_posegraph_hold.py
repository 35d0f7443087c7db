"""The held set of the pose-graph optimiser on the device (ym_graph_hold / ym_graph_held, PoseGraphOptimizer.hold / release,
LoopClosingMapper.hold_vertices) against tests/posegraph_hold_ref.py: the factor and the substitutions over the slots alone,
the band in slots, far edges, block-Jacobi around the workgroup size, `compute` end to end, the byte identities with a handle
that never heard of holding, the degenerate sets, the C entry and one closure through the mapper with a held prior.  The
cases and what the yardstick itself does on them are tests/test_posegraph_hold_host.py's; the bound on z is
tests/test_posegraph_host.py's ETA_BOUND, derived there."""
import ctypes as C
import math

import numpy as np
import pytest

from tests import posegraph_hold_ref as href
from tests import posegraph_ref as ref
from tests.test_gpu_posegraph import _optimizer, _pose_diff, square_loop
from tests.test_posegraph_hold_host import CG_TOL, HOLD_WIDTHS, e2e_graphs, held_set, hold_cases
from tests.test_posegraph_host import BAND_LAMBDA, ETA_BOUND

pytestmark = pytest.mark.gpu

CONVERGED, PIVOT = 1, 2  # ym_graph_solve's flags
REFERENCE_CALL = (100, 1.0e-4, True, 1.0e-9, 50)


def _hold_only(opt, held):
    """the held set of `opt` becomes `held` (and node 0)"""
    n = len(opt.nodes_xyt)
    opt.release(list(range(1, n)))
    opt.hold(list(held))


def _held_optimizer(g, held):
    opt = _optimizer(g)
    opt.hold(list(held))
    return opt


@pytest.fixture(scope="module")
def cases():
    """{W: [(n, kind, graph, held, band, A, M, b)]}: the dense systems in solve order at the automatic band, computed once"""
    out = {}
    for W, n, kind, g, held in hold_cases():
        band = href.auto_band(g, held)
        out.setdefault(W, []).append((n, kind, g, held, band) + href.damped_system(g, BAND_LAMBDA, band, held))
    return out


@pytest.fixture(scope="module")
def handles():
    """one optimiser a graph; the cases change its held set, which is part of what is checked"""
    made = {}

    def get(W, n, g):
        if (W, n) not in made:
            made[W, n] = _optimizer(g)
        return made[W, n]
    yield get
    for opt in made.values():
        opt.close()


@pytest.mark.parametrize("W", HOLD_WIDTHS)
def test_factor_and_substitutions_over_the_slots(cases, handles, W):
    """max_cg_iters = 0: z = band(A, band)^-1 b in solve order, nothing else"""
    worst = 0.0
    for n, kind, g, held, band, A, M, b in cases[W]:
        opt = handles(W, n, g)
        _hold_only(opt, held)
        delta, z, used, iters, res, flags = opt.solve_step(BAND_LAMBDA, band=-1, max_cg_iters=0)
        eta = ref.backward_error(M, href.to_solve_order(z, held), b)
        worst = max(worst, eta)
        print("W %d n %d %s: band %d, eta %.3g" % (W, n, kind, used, eta))
        assert used == band, (W, n, kind, used, band)
        assert iters == 0 and not flags & PIVOT
        assert eta <= ETA_BOUND, (W, n, kind, eta)
        mask = href.held_mask(n, held)
        assert z[mask].tobytes() == np.zeros_like(z[mask]).tobytes() and delta.tobytes() == np.zeros_like(delta).tobytes()
        assert z[~mask].any()
        assert np.array_equal(opt.held, np.flatnonzero(mask))
    print("W %d: worst eta of z %.3g (bound %.3g)" % (W, worst, ETA_BOUND))
    if W == 1:  # far edges of index distance >= 17 inside the slot band
        assert any(n == 257 and kind == "every third" and band == 13 for n, kind, g, held, band, A, M, b in cases[1])


def test_the_band_lives_in_slots():
    """interleaved(12, 31): by index the band would be 6, in slots it is 1 and holds every edge between free nodes, so the
    preconditioner is the inverse and the solve takes one iteration"""
    g = href.interleaved(12, 31)
    held = g["held"]
    A, M, b = href.damped_system(g, BAND_LAMBDA, 1, held)
    assert ref.auto_band(g) == 6 and np.array_equal(A, M)
    opt = _held_optimizer(g, held)
    delta, z, used, iters, res, flags = opt.solve_step(BAND_LAMBDA, band=-1, cg_tol=CG_TOL, max_cg_iters=50)
    eta = ref.backward_error(A, href.to_solve_order(delta, held), b)
    print("interleaved(12, 31): band %d, %d iteration(s), residual %.3g, eta %.3g" % (used, iters, res, eta))
    assert used == 1 and flags == CONVERGED
    assert iters == 1
    assert res <= 1e-12
    assert eta <= ETA_BOUND
    assert not delta[held].any() and not delta[0].any()
    opt.close()


@pytest.mark.parametrize("W", HOLD_WIDTHS)
def test_edges_beyond_the_slot_band(cases, handles, W):
    """the device's iteration count is the yardstick's on the reduced system (one more for rounding at the stop), and the
    residual recomputed from delta stays within the tolerance (plus the drift of the recursively updated one)"""
    for n, kind, g, held, band, A, M, b in cases[W]:
        _, want_iters, _ = ref.pcg(A, M, b, CG_TOL, 50)
        opt = handles(W, n, g)
        _hold_only(opt, held)
        delta, z, used, iters, res, flags = opt.solve_step(BAND_LAMBDA, band=-1, cg_tol=CG_TOL, max_cg_iters=50)
        x = href.to_solve_order(delta, held)
        Al, dl, bl = (np.asarray(v, dtype=np.longdouble) for v in (A, x.ravel(), b))
        nb = float(np.sqrt((bl * bl).sum()))
        true_res = float(np.sqrt(((Al @ dl - bl) ** 2).sum())) / nb
        drift = 64 * 2.0 ** -53 * float(np.abs(np.linalg.eigvalsh(A)).max()) * float(np.linalg.norm(x)) / nb
        print("W %d n %d %s: band %d, %d iterations (yardstick %d), residual %.3g reported, %.3g recomputed (drift term %.3g)"
              % (W, n, kind, used, iters, want_iters, res, true_res, drift))
        assert used == band and flags == CONVERGED, (W, n, kind, flags)
        assert 1 <= iters <= want_iters + 1, (W, n, kind, iters, want_iters)
        assert true_res <= CG_TOL + drift, (W, n, kind, true_res)
        mask = href.held_mask(n, held)
        assert delta[mask].tobytes() == np.zeros_like(delta[mask]).tobytes()


@pytest.mark.parametrize("n_slots", [511, 512, 513])
def test_block_jacobi_around_the_workgroup_size(n_slots):
    """band 0 factors and applies by slot, 512 threads striding over them; every second node held"""
    n = 2 * (n_slots - 1) + 1
    g = ref.banded(n, 2, n)
    held = list(range(0, n, 2))
    A, M, b = href.damped_system(g, BAND_LAMBDA, 0, held)
    assert len(b) == 3 * n_slots and not np.array_equal(A, M)
    opt = _held_optimizer(g, held)
    delta, z, used, iters, res, flags = opt.solve_step(BAND_LAMBDA, band=0, max_cg_iters=0)
    eta = ref.backward_error(M, href.to_solve_order(z, held), b)
    print("band 0, %d slots of %d nodes: eta %.3g (bound %.3g)" % (n_slots, n, eta, ETA_BOUND))
    assert used == 0 and iters == 0 and not flags & PIVOT
    assert eta <= ETA_BOUND
    assert not z[held].any() and not delta.any() and z[1::2].any(axis=1).all()
    opt.close()


@pytest.fixture(scope="module")
def e2e_wanted():
    """the yardstick's answer of the end-to-end cases, computed once"""
    out = {}
    for name, (g, held) in e2e_graphs().items():
        poses, rep = href.optimize(g, held)
        out[name] = dict(g, held=held, want=poses, want_report=rep)
    return out


@pytest.mark.parametrize("name", ["ring64", "spliced"])
def test_compute_end_to_end(e2e_wanted, name):
    g = e2e_wanted[name]
    held, want = g["held"], g["want_report"]
    opt = _held_optimizer(g, held)
    rep = opt.compute(*REFERENCE_CALL)
    got = opt.nodes_xyt
    err = _pose_diff(got, g["want"])
    print("%s: pose difference %.3g, chi2 %.12g against %.12g, steps %d / %d, accepted %d / %d, cg %d, band %d"
          % (name, err, rep.chi2_final, want["chi2_final"], rep.lm_steps, want["lm_steps"], rep.accepted, want["accepted"],
             rep.cg_iterations, rep.band))
    assert err <= 1e-9
    assert abs(rep.chi2_final - want["chi2_final"]) <= 1e-9 * want["chi2_final"]
    assert abs(rep.chi2_initial - want["chi2_initial"]) <= 1e-9 * want["chi2_initial"]
    assert (rep.lm_steps, rep.accepted, rep.status) == (want["lm_steps"], want["accepted"], want["status"])
    assert rep.band == href.auto_band(g, held)
    assert got[held].tobytes() == g["poses"][held].tobytes()
    assert abs(opt.chi2() - rep.chi2_final) <= 1e-9 * rep.chi2_final
    opt.close()
    if name == "spliced":  # what the hold saves (DESIGN.md section 9 records these counts)
        free = _optimizer(g)
        rep0 = free.compute(*REFERENCE_CALL)
        print("spliced: cg iterations %d over %d steps with the prior held (band %d), %d over %d steps with nothing held (band %d)"
              % (rep.cg_iterations, rep.lm_steps, rep.band, rep0.cg_iterations, rep0.lm_steps, rep0.band))
        assert rep.cg_iterations < rep0.cg_iterations
        free.close()


def test_identities_byte_for_byte():
    g = ref.ring(64, noise=0.02, seed=1)
    fresh = _optimizer(g)
    rep = fresh.compute(*REFERENCE_CALL)
    want = fresh.nodes_xyt.tobytes()
    assert want != g["poses"].tobytes()
    some = [5, 6, 7, 30, 63]
    for prepare in (lambda o: o.hold([]), lambda o: o.hold([0]), lambda o: (o.hold(some), o.release(some)),
                    lambda o: (o.hold(some), o.chi2(), o.release(some))):  # (the last: the held set reached the library)
        opt = _optimizer(g)
        prepare(opt)
        assert opt.held.tolist() == [0]
        rep1 = opt.compute(*REFERENCE_CALL)
        assert opt.nodes_xyt.tobytes() == want
        assert (rep1.lm_steps, rep1.cg_iterations, rep1.chi2_final, rep1.band) == (rep.lm_steps, rep.cg_iterations, rep.chi2_final, rep.band)
        opt.close()
    fresh.close()
    # A held, compute, then B as well, compute: a fresh handle from the intermediate poses with A and B held
    A, B = list(range(12)), [40, 41, 42, 50]
    one = _held_optimizer(g, A)
    one.compute(*REFERENCE_CALL)
    mid = one.nodes_xyt.copy()
    assert mid[A].tobytes() == g["poses"][A].tobytes() and mid[B].tobytes() != g["poses"][B].tobytes()
    one.hold(B)
    rep_a = one.compute(*REFERENCE_CALL)
    two = _held_optimizer(dict(g, poses=mid), A + B)
    rep_b = two.compute(*REFERENCE_CALL)
    assert one.nodes_xyt.tobytes() == two.nodes_xyt.tobytes()
    assert one.nodes_xyt[A + B].tobytes() == mid[A + B].tobytes()
    assert (rep_a.lm_steps, rep_a.cg_iterations, rep_a.chi2_final) == (rep_b.lm_steps, rep_b.cg_iterations, rep_b.chi2_final)
    one.close()
    two.close()


def test_degenerate_held_sets():
    from yag_slam_amd.posegraph import PoseGraphOptimizer
    g = ref.ring(16, noise=0.02, seed=4)
    n = len(g["poses"])
    # every node held: nothing to solve, and the constant chi2 is reported
    opt = _held_optimizer(g, range(n))
    chi2 = opt.chi2()
    rep = opt.compute(*REFERENCE_CALL)
    assert (rep.lm_steps, rep.accepted, rep.cg_iterations, rep.status) == (0, 0, 0, 0)
    assert rep.chi2_initial == rep.chi2_final == chi2 > 0.0
    assert opt.nodes_xyt.tobytes() == g["poses"].tobytes()
    delta, z, used, iters, res, flags = opt.solve_step(BAND_LAMBDA, max_cg_iters=5)
    assert not delta.any() and not z.any() and (used, iters, res, flags) == (0, 0, 0.0, 0)
    # ... and the same handle with one node released: that node's edges all go to held nodes
    opt.release([9])
    rep = opt.compute(*REFERENCE_CALL)
    want, want_rep = href.optimize(g, [i for i in range(n) if i != 9])
    assert rep.band == 0 and rep.cg_iterations == rep.lm_steps == want_rep["lm_steps"] >= 1
    assert _pose_diff(opt.nodes_xyt, want) <= 1e-9 and abs(rep.chi2_final - want_rep["chi2_final"]) <= 1e-9 * want_rep["chi2_final"]
    rest = [i for i in range(n) if i != 9]
    assert opt.nodes_xyt[rest].tobytes() == g["poses"][rest].tobytes() and opt.nodes_xyt[9].tobytes() != g["poses"][9].tobytes()
    opt.close()
    # two nodes, both held
    two = PoseGraphOptimizer()
    two.add_node(0.0, 0.0, 0.1, 0)
    two.add_node(1.0, 0.2, 3.5, 1)  # (a heading outside (-pi, pi]: a held node's is not wrapped)
    two.add_constraint(0, 1, 1.1, 0.0, 0.0, np.eye(3))
    two.hold([1])
    rep = two.compute(*REFERENCE_CALL)
    assert rep.lm_steps == 0 and rep.chi2_final == rep.chi2_initial == two.chi2() > 0.0
    assert two.nodes_xyt.tolist() == [[0.0, 0.0, 0.1], [1.0, 0.2, 3.5]]
    two.close()
    # a star of free nodes around one held node: no block off the diagonal, band 0, one iteration a solve
    rng = np.random.default_rng(7)
    # (the centre is node 1: an edge at node 0 counts in the automatic band, as it does with nothing else held)
    truth = np.array([[-3.0, 0.0, 0.0], [0.0, 0.0, 0.0]] + [[2.0 * math.cos(k), 2.0 * math.sin(k), 0.3 * k] for k in range(2, 10)])
    star = ref._finish(truth, [(0, 1)] + [(1, k) if k % 2 else (k, 1) for k in range(2, 10)], 0.02, rng, jitter=(0.05, 0.05, 0.02))
    opt = _held_optimizer(star, [1])
    rep = opt.compute(*REFERENCE_CALL)
    want, want_rep = href.optimize(star, [1])
    assert rep.band == 0 and rep.cg_iterations == rep.lm_steps == want_rep["lm_steps"]
    assert _pose_diff(opt.nodes_xyt, want) <= 1e-9
    opt.close()
    # a free component without a held node: as a component not connected to node 0 behaves, the damping keeps it definite
    g2 = ref.ring(16, noise=0.02, seed=4)
    keep = [m for m, (a, b) in enumerate(g2["edges"].tolist()) if (a < 8) == (b < 8)]
    g2 = dict(g2, edges=g2["edges"][keep], means=g2["means"][keep], infos=g2["infos"][keep])
    opt = _held_optimizer(g2, range(8))
    rep = opt.compute(*REFERENCE_CALL)
    assert rep.accepted >= 1 and rep.chi2_final < rep.chi2_initial
    assert opt.nodes_xyt[:8].tobytes() == g2["poses"][:8].tobytes()
    opt.close()


def test_the_c_entry():
    from yag_slam_amd import _capi
    L = _capi.lib()
    h = L.ym_graph_create(0)
    assert h
    try:
        dp, ip, bp = C.POINTER(C.c_double), C.POINTER(C.c_int32), C.POINTER(C.c_uint8)
        xyt = np.zeros((4, 3))
        assert L.ym_graph_add_nodes(h, xyt.ctypes.data_as(dp), 4) == 0
        mask = np.full(4, 7, dtype=np.uint8)
        assert L.ym_graph_held(h, mask.ctypes.data_as(bp), 4) == 0 and mask.tolist() == [1, 0, 0, 0]
        nodes = np.array([2, 4], dtype=np.int32)
        assert L.ym_graph_hold(h, nodes.ctypes.data_as(ip), 2, 1) == -1 and "out of range" in _capi.last_error()
        nodes = np.array([3, -1], dtype=np.int32)
        assert L.ym_graph_hold(h, nodes.ctypes.data_as(ip), 2, 0) == -1 and "out of range" in _capi.last_error()
        assert L.ym_graph_held(h, mask.ctypes.data_as(bp), 4) == 0 and mask.tolist() == [1, 0, 0, 0]  # nothing was applied
        nodes = np.array([2, 3], dtype=np.int32)
        assert L.ym_graph_hold(h, nodes.ctypes.data_as(ip), 2, 1) == 0
        nodes = np.array([3, 0], dtype=np.int32)
        assert L.ym_graph_hold(h, nodes.ctypes.data_as(ip), 2, 0) == -1 and "node 0" in _capi.last_error()
        assert L.ym_graph_held(h, mask.ctypes.data_as(bp), 4) == 0 and mask.tolist() == [1, 0, 1, 1]
        nodes = np.array([3, 1], dtype=np.int32)
        assert L.ym_graph_hold(h, nodes.ctypes.data_as(ip), 2, 0) == 0
        assert L.ym_graph_held(h, mask.ctypes.data_as(bp), 4) == 0 and mask.tolist() == [1, 0, 1, 0]
        assert L.ym_graph_held(h, mask.ctypes.data_as(bp), 3) == -1 and "4 nodes" in _capi.last_error()
        assert L.ym_graph_add_nodes(h, xyt.ctypes.data_as(dp), 1) == 0  # a node is free when added
        mask = np.zeros(5, dtype=np.uint8)
        assert L.ym_graph_held(h, mask.ctypes.data_as(bp), 5) == 0 and mask.tolist() == [1, 0, 1, 0, 0]
    finally:
        L.ym_graph_destroy(h)


def test_a_closure_through_the_mapper_leaves_a_held_prior_alone():
    """The square loop of tests/test_gpu_posegraph.py behind a 4 x 4 grid of prior vertices, linked with identity * 1e-12 as
    splicing.map_to_graphslam links them and held through hold_vertices; the first live scan is spliced in.  The grid lies
    20 m from the loop, out of the loop search's reach."""
    from collections import namedtuple
    from yag_slam_amd.mapping import LoopClosingMapper
    from yag_slam_amd.models import LocalizedRangeScan
    from yag_slam_amd.posegraph import PoseGraphOptimizer
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

    def scan_at(x, y, t):
        return LocalizedRangeScan([1.0] * 5, -1, 1, 0.5, 0, 10, 5, x, y, t)

    class Recording(PoseGraphOptimizer):
        def compute(self, *args):
            self.before = self.nodes_xyt.copy()
            self.calls = getattr(self, "calls", 0) + 1
            return super().compute(*args)

    opt = Recording()
    mp = LoopClosingMapper(Seq(), Loop(), loop_search_dist=3.0, loop_search_min_chain_size=3, optimizer=opt)
    prior = [scan_at(-20.0 + 0.5 * (k % 4), -20.0 + 0.5 * (k // 4), 0.1 * k) for k in range(16)]
    for k, s in enumerate(prior):
        s.num = k
        mp.add_vertex(s)
    for k in range(16):
        if (k + 1) % 4:
            mp.link_scans(prior[k], prior[k + 1], np.identity(3) * 1e-12)
        if k + 4 < 16:
            mp.link_scans(prior[k], prior[k + 4], np.identity(3) * 1e-12)
    mp.hold_vertices(prior[:8] + list(range(8, 16)))
    assert opt.held.tolist() == list(range(16))

    def bits(s):
        p = s.corrected_pose
        return np.array([p.x, p.y, p.euler[-1]]).tobytes()
    had = [bits(s) for s in prior]
    closed_at = None
    for i in range(len(truth)):
        state["i"] = i
        s = scan_at(0.0, 0.0, 0.0)
        s.odom_pose = Transform(odom[i][0], odom[i][1], 0, odom[i][2])
        if i == 0:
            s.corrected_pose = Transform(odom[0][0], odom[0][1], 0, odom[0][2])
            mp.splice_first_scan(s, radius=100)
            continue
        _, closed = mp.process_scan(s)
        if closed:
            closed_at = i
            break
    assert closed_at is not None and closed_at >= 30, closed_at
    assert opt.calls == 1 and len(opt.nodes) == len(mp.scans) == 16 + closed_at + 1
    assert [bits(s) for s in prior] == had
    after = opt.nodes_xyt
    assert after[:16].tobytes() == opt.before[:16].tobytes()
    for s, row in zip(mp.scans[16:], after[16:]):
        p = s.corrected_pose
        assert (p.x, p.y) == (row[0], row[1]) and abs(float(ref.wrap(p.euler[-1] - row[2]))) < 1e-12
    rep = opt.last_report
    edges = np.array([(f, t) for f, t, _, _ in mp.constraints], dtype=np.int32)
    means = np.array([(m.x, m.y, m.euler[-1]) for _, _, m, _ in mp.constraints])
    infos = np.array([np.linalg.inv(np.array(c)) for _, _, _, c in mp.constraints])
    chi_before, chi_after = ref.chi2(opt.before, edges, means, infos), ref.chi2(after, edges, means, infos)
    print("closure at %d behind a held prior: chi2 %.4g -> %.4g, %d steps, %d cg iterations, band %d"
          % (closed_at, chi_before, chi_after, rep.lm_steps, rep.cg_iterations, rep.band))
    assert chi_after < chi_before and rep.chi2_final < rep.chi2_initial
    assert abs(rep.chi2_final - chi_after) <= 1e-9 * chi_after
    assert not np.array_equal(after[16:-1], opt.before[16:-1])
    assert all(s in mp.index.buckets[mp.index.key(s.corrected_pose)] for s in mp.scans)
