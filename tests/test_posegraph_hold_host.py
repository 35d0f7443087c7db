"""CPU-only checks of the pose-graph optimiser's held set: the yardstick tests/posegraph_hold_ref.py against
tests/posegraph_ref.py, the cases of tests/test_gpu_posegraph_hold.py (that they are the ones meant, and that the yardstick
itself stays inside what the device is held to), and the argument checks that need no device."""
import numpy as np
import pytest

from tests import posegraph_hold_ref as href
from tests import posegraph_ref as ref
from tests.test_posegraph_host import BAND_LAMBDA, case_seed

HOLD_WIDTHS = (1, 7, 16)
HOLD_SIZES = (6, 13, 40, 257)
HOLD_KINDS = ("first third", "every third", "last third", "all but one", "all but two")
CG_TOL = 1e-10


def held_set(g, kind):
    """the held set of a kind on a graph (node 0 is added by the yardstick and by the device), or None where there is none"""
    n = len(g["poses"])
    if kind == "first third":
        return list(range(n // 3))
    if kind == "every third":
        return list(range(0, n, 3))
    if kind == "last third":
        return list(range(n - n // 3, n))
    if kind == "all but one":
        return [i for i in range(n) if i != n // 2]
    linked = {tuple(sorted(p)) for p in g["edges"].tolist()}
    for a in range(1, n):  # all but two that share no edge: the first such pair, the second node from the far end
        for b in range(n - 1, a, -1):
            if (a, b) not in linked:
                return [i for i in range(n) if i not in (a, b)]
    return None


def hold_cases():
    """[(W, n, kind, graph, held)] of every case that exists"""
    out = []
    for W in HOLD_WIDTHS:
        for n in HOLD_SIZES:
            g = ref.banded(n, W, case_seed(W, n))
            for kind in HOLD_KINDS:
                held = held_set(g, kind)
                if held is not None:
                    out.append((W, n, kind, g, held))
    return out


@pytest.fixture(scope="module")
def cases():
    return hold_cases()


def test_only_node_0_held_is_the_old_yardstick_to_the_bit():
    for g, band in ((ref.ring(64, noise=0.02, seed=1), 3), (ref.banded(40, 7, 740), 7), (ref.grid(5, 5, noise=0.02, seed=3), 5)):
        n = len(g["poses"])
        slot, node_of_slot = href.slots(n, [0])
        assert np.array_equal(slot, np.arange(n)) and np.array_equal(node_of_slot, np.arange(n))
        assert href.auto_band(g, []) == ref.auto_band(g)
        for got, want in zip(href.damped_system(g, BAND_LAMBDA, band, [0]), ref.damped_system(g, BAND_LAMBDA, band)):
            assert got.tobytes() == want.tobytes()
        (p1, r1), (p0, r0) = href.optimize(g, []), ref.optimize(g)
        assert p1.tobytes() == p0.tobytes() and r1 == r0


def test_slots_and_the_band_in_slots():
    slot, node_of_slot = href.slots(7, [2, 3, 6])
    assert slot.tolist() == [0, 1, 0, 0, 2, 3, 0] and node_of_slot.tolist() == [0, 1, 4, 5]
    g = href.interleaved(12, 31)
    held = g["held"]
    assert len(g["poses"]) == 31 * 11 + 7 and len(held) == len(g["poses"]) - 12
    assert ref.auto_band(g) == 6 and href.auto_band(g, held) == 1
    A, M, b = href.damped_system(g, BAND_LAMBDA, 1, held)
    assert A.shape == (39, 39) and np.array_equal(A, M)
    np.linalg.cholesky(A)
    x, it, res = ref.pcg(A, M, b, CG_TOL, 50)
    print("interleaved(12, 31): %d iteration(s), residual %.3g" % (it, res))
    assert it == 1 and res <= 1e-15
    # a held neighbour gives a free node its diagonal block and gradient, nothing else: the free rows of the full system
    h, grad = ref.linear_system(g["poses"], g["edges"], g["means"], g["infos"])
    h = h.toarray()
    first = 3 * 6
    assert np.allclose(A[3:6, 3:6], (h + BAND_LAMBDA * np.diag(np.diag(h)))[first:first + 3, first:first + 3], rtol=1e-15, atol=0)
    assert np.array_equal(b[3:6], -grad[first:first + 3])
    # no edge between two free nodes, none at node 0: band 0; an edge at node 0 counts, as it does with nothing else held
    star = dict(g, edges=np.array([[1, 2], [5, 6], [36, 37]], dtype=np.int32), means=g["means"][:3], infos=g["infos"][:3])
    assert href.auto_band(star, held) == 0
    assert href.auto_band(dict(star, edges=np.array([[1, 2], [5, 6], [0, 37]], dtype=np.int32)), held) == 2


def test_hold_cases_are_the_ones_meant(cases):
    assert len(cases) >= 48
    seen = set()
    counts = []
    for W, n, kind, g, held in cases:
        seen.add((W, n, kind))
        A, M, b = href.damped_system(g, BAND_LAMBDA, href.auto_band(g, held), held)
        np.linalg.cholesky(M)  # positive definite (raises LinAlgError otherwise)
        np.linalg.cholesky(A)
        f = len(g["poses"]) - len(set(held) | {0})
        assert A.shape == (3 * f + 3, 3 * f + 3) and f >= 1
        if kind == "all but two":
            assert f == 2 and np.array_equal(A, M)  # (no block off the diagonal, whatever the band)
        x, it, res = ref.pcg(A, M, b, CG_TOL, 50)
        assert 1 <= it <= 13 and res <= CG_TOL, (W, n, kind, it, res)
        counts.append(it)
    print("%d cases; pcg iterations %d .. %d" % (len(cases), min(counts), max(counts)))
    for W in HOLD_WIDTHS:
        for n in HOLD_SIZES:
            for kind in HOLD_KINDS[:4]:
                assert (W, n, kind) in seen
    # far edges of index distance >= 17 come within 16 slots when every third node is held
    g = ref.banded(257, 1, case_seed(1, 257))
    assert ref.auto_band(g) == 1 and href.auto_band(g, held_set(g, "every third")) == 13


def test_the_prior_held_agrees_with_the_unheld_optimum():
    """The prior's edges carry 1e12: left free its vertices move by about 1e-11 m, so the two problems agree and the new
    yardstick is checked against the old one."""
    g = href.spliced(6, 6, 40)
    p0, r0 = ref.optimize(g)
    p1, r1 = href.optimize(g, g["prior"])
    d = p1 - p0
    d[:, 2] = ref.wrap(d[:, 2])
    moved = np.abs(p0[g["prior"]] - g["poses"][g["prior"]]).max()
    print("spliced(6, 6, 40): held against unheld %.3g, the unheld prior moved %.3g; steps %d / %d, chi2 %.6g / %.6g"
          % (np.abs(d).max(), moved, r1["lm_steps"], r0["lm_steps"], r1["chi2_final"], r0["chi2_final"]))
    assert np.abs(d).max() < 1e-9
    assert p1[g["prior"]].tobytes() == g["poses"][g["prior"]].tobytes()
    assert r1["status"] == 1 and r1["chi2_final"] < 0.5 * r1["chi2_initial"]


def e2e_graphs():
    """{name: (graph, held)} of the end-to-end cases of the device test.  The spliced graph's seed is the first of 5 + 1000 k
    at which no gain of the yardstick's own run comes within a factor 2 of the stop rule 1e-9 chi2 (5 and 1005: 1.87), as
    tests/test_posegraph_host.py chooses E2E_CASES; test_end_to_end_cases_stop_clear_of_the_rule holds it to that."""
    g = href.spliced(5, 5, 20, seed=2005)
    k = 7  # a grid-grid edge that gets a residual of 1e-5 m: a constant chi2 term of about 1e12 * 1e-10
    assert g["edges"][k].max() < 25
    means = g["means"].copy()
    means[k, 0] += 1e-5
    return {"ring64": (ref.ring(64, noise=0.02, seed=1), list(range(20))), "spliced": (dict(g, means=means), list(g["prior"]))}


def test_end_to_end_cases_stop_clear_of_the_rule():
    for name, (g, held) in e2e_graphs().items():
        history = []
        poses, rep = href.optimize(g, held, history=history)
        chi = [rep["chi2_initial"]] + history
        ratio = [(chi[i] - chi[i + 1]) / (1e-9 * chi[i]) for i in range(len(history))]
        print("%s: status %d after %d steps, chi2 %.6g -> %.6g, gains over the stop rule %s"
              % (name, rep["status"], rep["lm_steps"], chi[0], chi[-1], ["%.3g" % r for r in ratio]))
        assert rep["status"] == 1 and rep["lm_steps"] >= 3
        assert all(r < 0.5 or r > 2.0 for r in ratio), (name, ratio)
        assert poses[held].tobytes() == g["poses"][held].tobytes()
        if name == "spliced":  # the constant term: the held grid's one edge with a residual
            a, b = g["edges"][7]
            e = ref.residuals(g["poses"], g["edges"][7:8], g["means"][7:8])[0]
            const = float(e @ g["infos"][7] @ e)
            assert const > 10.0 and rep["chi2_final"] > const


def test_zero_step_cases_of_the_yardstick():
    g = ref.ring(8, noise=0.02, seed=4)
    poses, rep = href.optimize(g, range(8))
    assert rep["lm_steps"] == 0 and rep["chi2_final"] == rep["chi2_initial"] == ref.chi2(g["poses"], g["edges"], g["means"], g["infos"]) > 0
    assert poses.tobytes() == g["poses"].tobytes()


def test_hold_and_release_validate_without_a_device():
    from yag_slam_amd.posegraph import PoseGraphOptimizer
    opt = PoseGraphOptimizer()
    assert opt.held.tolist() == [0]
    for i in range(5):
        opt.add_node(float(i), 0.0, 0.0, i)
    assert opt.held.tolist() == [0]
    with pytest.raises(ValueError, match="out of range"):
        opt.hold([1, 5])
    with pytest.raises(ValueError, match="out of range"):
        opt.release([-1])
    with pytest.raises(ValueError, match="node 0"):
        opt.release([2, 0])
    assert opt.held.tolist() == [0]  # nothing of a refused call is applied
    with pytest.raises(ValueError, match="integers"):
        opt.hold([1.5])
    opt.hold([3, 1])
    opt.hold([3])
    opt.hold(np.array([1], dtype=np.int64))
    assert opt.held.tolist() == [0, 1, 3] and opt.held.dtype.kind == "i"
    opt.release([2])  # (free already)
    opt.release([1])
    opt.release([1])
    assert opt.held.tolist() == [0, 3]
    opt.hold([])
    opt.hold([0])
    assert opt.held.tolist() == [0, 3]
    opt.add_node(5.0, 0.0, 0.0, 5)
    opt.hold([5])  # a node added since, not flushed yet
    assert opt.held.tolist() == [0, 3, 5]


def test_holding_through_a_mapper_without_an_optimiser_raises(monkeypatch):
    from yag_slam_amd import splicing
    from yag_slam_amd.mapping import LoopClosingMapper
    from yag_slam_amd.posegraph import PoseGraphOptimizer
    from tests.test_segments_host import _Scan
    scans = [_Scan(i, 0.5 * i, 0.25 * i) for i in range(4)]
    monkeypatch.setattr(splicing, "map_to_graph", lambda *a, **k: (scans, [(0, 1), (1, 2), (2, 3)]))
    mp = LoopClosingMapper(None, None)
    with pytest.raises(ValueError, match="optimizer"):
        mp.hold_vertices([0])
    with pytest.raises(ValueError, match="optimizer"):
        splicing.map_to_graphslam(mp, None, 0.05, (0.0, 0.0), None, hold=True)
    assert mp.scans == []  # refused before anything was added

    class FourCalls:  # an optimizer with SPA2d's four calls and no hold
        nodes = ()

        def add_node(self, *a):
            pass

        def add_constraint(self, *a):
            pass

        def compute(self, *a):
            pass
    with pytest.raises(ValueError, match="optimizer"):
        LoopClosingMapper(None, None, optimizer=FourCalls()).hold_vertices([0])
    # with one: every vertex of the prior is held, by scan or by num; the default holds nothing
    opt = PoseGraphOptimizer()
    mp = LoopClosingMapper(None, None, optimizer=opt)
    assert splicing.map_to_graphslam(mp, None, 0.05, (0.0, 0.0), None, hold=True) is mp
    assert opt.held.tolist() == [0, 1, 2, 3] and mp.held_nums == {0, 1, 2, 3}
    opt2 = PoseGraphOptimizer()
    mp2 = LoopClosingMapper(None, None, optimizer=opt2)
    splicing.map_to_graphslam(mp2, None, 0.05, (0.0, 0.0), None)
    assert opt2.held.tolist() == [0] and mp2.held_nums == set()
    mp2.hold_vertices([scans[2], 3])
    assert opt2.held.tolist() == [0, 2, 3]


def test_the_header_documents_the_new_entries():
    import os
    text = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "yagmatch.h")).read()
    assert "int ym_graph_hold(ym_graph *g, const int32_t *nodes, int n, int hold" in text
    assert "int ym_graph_held(const ym_graph *g, uint8_t *mask, int n_nodes)" in text
