"""The band solver of the pose-graph optimiser (ym_k_posegraph.hpp: the block-banded Cholesky factor, the two substitutions,
the preconditioned conjugate gradients) against dense solves of tests/posegraph_ref.py, at every band width where a row
takes another number of loads, at node counts around the window, the prefetch depth and the block-Jacobi stride, with edges
stored in both directions and one edge twice.  `compute()` corrects its own errors (CG with a slightly wrong preconditioner
still converges), so the solve is observed through `solve_step` (ym_graph_solve): z = band(A, W)^-1 b alone, one iteration
at full band, and the rank bound with far edges.  The cases and the bounds are those of tests/test_posegraph_host.py, which
holds the yardstick itself to them on the CPU."""
import numpy as np
import pytest

from tests import posegraph_ref as ref
from tests.test_gpu_posegraph import _optimizer, _pose_diff
from tests.test_posegraph_host import BAND_LAMBDA, BAND_WIDTHS, CASES, E2E_CASES, ETA_BOUND, case_seed, far_applies

pytestmark = pytest.mark.gpu

CONVERGED, PIVOT = 1, 2  # ym_graph_solve's flags
CG_TOL = 1e-10


@pytest.fixture(scope="module")
def systems():
    """(graph, A, M, b) by (W, n, far), made when first asked for and never modified"""
    made = {}

    def get(W, n, far):
        if (W, n, far) not in made:
            g = ref.banded(n, W, case_seed(W, n), far=far)
            made[W, n, far] = (g,) + ref.damped_system(g, BAND_LAMBDA, W)
        return made[W, n, far]
    return get


@pytest.fixture(scope="module")
def handles(systems):
    """one optimiser a case"""
    made = {}

    def get(W, n, far):
        if (W, n, far) not in made:
            made[W, n, far] = _optimizer(systems(W, n, far)[0])
        return made[W, n, far]
    yield get
    for opt in made.values():
        opt.close()


def _sizes(W):
    return [n for w, n in CASES if w == W]


@pytest.mark.parametrize("W", BAND_WIDTHS)
def test_preconditioner_alone(systems, handles, W):
    """max_cg_iters = 0: z is the factor and both substitutions applied to b, nothing else.  A handful of roundings an entry
    apart from LAPACK (reciprocal square roots for divisions, another order in the trailing update): 32 times its error; a
    wrong block, slot or row gives 1e-3 or more."""
    worst = 0.0
    for n in _sizes(W):
        g, A, M, b = systems(W, n, 2)
        delta, z, band, iters, res, flags = handles(W, n, 2).solve_step(BAND_LAMBDA, band=W, max_cg_iters=0)
        eta = ref.backward_error(M, z, b)
        worst = max(worst, eta)
        print("W %d n %d: eta %.3g" % (W, n, eta))
        assert band == W and iters == 0 and not flags & PIVOT
        assert eta <= ETA_BOUND, (W, n, eta)
        assert not z[0].any() and not delta.any()
        assert z.tobytes() != np.zeros_like(z).tobytes()
    print("W %d: worst eta of z %.3g (bound %.3g)" % (W, worst, ETA_BOUND))


@pytest.mark.parametrize("n", [2, 511, 512, 513])
def test_preconditioner_alone_block_jacobi(n):
    """band 0 factors and applies by node, 512 threads striding over the nodes"""
    g = ref.banded(n, 1, n)
    A, M, b = ref.damped_system(g, BAND_LAMBDA, 0)
    opt = _optimizer(g)
    delta, z, band, iters, res, flags = opt.solve_step(BAND_LAMBDA, band=0, max_cg_iters=0)
    eta = ref.backward_error(M, z, b)
    print("W 0 n %d: eta %.3g (bound %.3g)" % (n, eta, ETA_BOUND))
    assert band == 0 and iters == 0 and not flags & PIVOT
    assert eta <= ETA_BOUND
    assert not z[0].any() and not delta.any() and z[1:].any()
    opt.close()


@pytest.mark.parametrize("W", BAND_WIDTHS)
def test_full_band_converges_in_one_iteration(systems, handles, W):
    """Without far edges band(A, W) = A: the preconditioner is the inverse, and an error of the factor or a substitution above
    1e-10 relative costs a second iteration.  The yardstick's residual after one is <= 6.4e-16; 1e-12 is three orders above
    it and two inside the stop."""
    worst = 0.0
    for n in _sizes(W):
        g, A, M, b = systems(W, n, 0)
        assert np.array_equal(A, M)
        delta, z, band, iters, res, flags = handles(W, n, 0).solve_step(BAND_LAMBDA, band=W, cg_tol=CG_TOL, max_cg_iters=50)
        eta = ref.backward_error(A, delta, b)
        worst = max(worst, eta)
        print("W %d n %d: %d iteration(s), residual %.3g, eta %.3g" % (W, n, iters, res, eta))
        assert band == W and flags == CONVERGED, (W, n, flags)
        assert iters == 1, (W, n, iters)
        assert res <= 1e-12, (W, n, res)
        assert eta <= ETA_BOUND, (W, n, eta)
        assert not delta[0].any()
    print("W %d: worst eta of delta at full band %.3g (bound %.3g)" % (W, worst, ETA_BOUND))


@pytest.mark.parametrize("W", BAND_WIDTHS)
def test_far_edges_cost_what_their_rank_allows(systems, handles, W):
    """Two edges beyond the band: A - M has rank <= 12, and the device needs no more iterations than the same recurrence
    with a dense solve (one more for rounding at the stop).  The residual is recomputed from delta: the second term is the
    drift of the recursively updated one, 1e-16 to 1e-15 here."""
    for n in _sizes(W):
        if not far_applies(W, n):
            continue
        g, A, M, b = systems(W, n, 2)
        _, want_iters, _ = ref.pcg(A, M, b, CG_TOL, 50)
        opt = handles(W, n, 2)
        delta, z, band, iters, res, flags = opt.solve_step(BAND_LAMBDA, band=W, cg_tol=CG_TOL, max_cg_iters=50)
        Al, dl, bl = (np.asarray(v, dtype=np.longdouble) for v in (A, delta.ravel(), b))
        nb = float(np.sqrt((bl * bl).sum()))
        true_res = float(np.sqrt(((Al @ dl - bl) ** 2).sum())) / nb
        drift = 64 * 2.0 ** -53 * float(np.abs(np.linalg.eigvalsh(A)).max()) * float(np.linalg.norm(delta)) / nb
        print("W %d n %d: %d iterations (yardstick %d), residual %.3g reported, %.3g recomputed (drift term %.3g)"
              % (W, n, iters, want_iters, res, true_res, drift))
        assert band == W and flags == CONVERGED, (W, n, flags)
        assert iters <= want_iters + 1, (W, n, iters, want_iters)
        assert true_res <= CG_TOL + drift, (W, n, true_res)
        assert not delta[0].any()
        # the automatic band: the header's rule, which is W wherever the far edges are longer than 16
        auto = opt.solve_step(BAND_LAMBDA, band=-1, cg_tol=CG_TOL, max_cg_iters=0)[2]
        assert auto == ref.auto_band(g), (W, n, auto)
        if n > 20:
            assert auto == W, (W, n, auto)


def test_two_fresh_handles_solve_to_identical_bytes(systems):
    g = systems(16, 257, 2)[0]
    runs = []
    for _ in range(2):
        opt = _optimizer(g)
        _, z0, _, _, _, _ = opt.solve_step(BAND_LAMBDA, band=16, max_cg_iters=0)
        delta, z, _, iters, res, _ = opt.solve_step(BAND_LAMBDA, band=16, cg_tol=CG_TOL, max_cg_iters=50)
        runs.append((z0.tobytes(), delta.tobytes(), z.tobytes(), iters, res))
        opt.close()
    assert runs[0] == runs[1]
    assert np.frombuffer(runs[0][1]).any()


def test_solve_step_leaves_the_poses_and_a_compute_alone(systems):
    """the hook between two computes changes neither the poses nor what the second compute returns"""
    g = systems(7, 40, 2)[0]
    a, b = _optimizer(g), _optimizer(g)
    before = a.nodes_xyt.copy()
    chi2 = a.chi2()
    a.solve_step(BAND_LAMBDA, band=7, cg_tol=CG_TOL, max_cg_iters=50)
    a.solve_step(BAND_LAMBDA, band=3, max_cg_iters=0)
    assert a.nodes_xyt.tobytes() == before.tobytes() and a.chi2() == chi2
    rep_a, rep_b = a.compute(100, 1.0e-4, True, 1.0e-9, 50), b.compute(100, 1.0e-4, True, 1.0e-9, 50)
    assert a.nodes_xyt.tobytes() == b.nodes_xyt.tobytes()
    assert (rep_a.lm_steps, rep_a.cg_iterations, rep_a.chi2_final) == (rep_b.lm_steps, rep_b.cg_iterations, rep_b.chi2_final)
    # no constraint, one node: zeros
    from yag_slam_amd.posegraph import PoseGraphOptimizer
    one = PoseGraphOptimizer()
    one.add_node(1.0, 2.0, 0.0, 0)
    one.add_node(2.0, 2.0, 0.0, 1)
    delta, z, band, iters, res, flags = one.solve_step(BAND_LAMBDA)
    assert delta.shape == (2, 3) and not delta.any() and not z.any() and (band, iters, res, flags) == (0, 0, 0.0, 0)
    # a right-hand side of zero (the poses satisfy the one constraint exactly): zeros, not what the buffers held
    one.add_constraint(0, 1, 1.0, 0.0, 0.0, np.eye(3))
    delta, z, band, iters, res, flags = one.solve_step(BAND_LAMBDA, band=1, max_cg_iters=5)
    assert not delta.any() and not z.any() and (band, iters, res, flags) == (1, 0, 0.0, CONVERGED)
    for opt in (a, b, one):
        opt.close()


@pytest.fixture(scope="module")
def e2e_wanted():
    """the yardstick's answer of every end-to-end case, computed once"""
    out = {}
    for n, W, far, seed in E2E_CASES:
        g = ref.banded(n, W, seed, far=far)
        poses, rep = ref.optimize(g)
        out[n, W, far] = dict(g, want=poses, want_report=rep, band=W)
    g = ref.grid(5, 5, noise=0.02, seed=3)
    poses, rep = ref.optimize(g)
    out["grid5"] = dict(g, want=poses, want_report=rep, band=5)
    return out


@pytest.mark.parametrize("case", [c[:3] for c in E2E_CASES] + ["grid5"], ids=str)
def test_end_to_end_at_every_load_count(e2e_wanted, case):
    """the reference's call with the automatic band; the tolerances are test_agreement_with_the_yardstick's"""
    g = e2e_wanted[case]
    opt = _optimizer(g)
    rep = opt.compute(100, 1.0e-4, True, 1.0e-9, 50)
    want_chi2 = g["want_report"]["chi2_final"]
    err = _pose_diff(opt.nodes_xyt, g["want"])
    print("%s: pose difference %.3g, chi2 %.12g against %.12g, steps %d / %d, cg %d, band %d"
          % (case, err, rep.chi2_final, want_chi2, rep.lm_steps, g["want_report"]["lm_steps"], rep.cg_iterations, rep.band))
    assert rep.band == g["band"]
    assert err <= 1e-9
    assert abs(rep.chi2_final - want_chi2) <= 1e-9 * want_chi2
    assert rep.status == 1 and rep.lm_steps == g["want_report"]["lm_steps"]
    if case != "grid5" and case[2] == 0:
        assert rep.cg_iterations == rep.lm_steps
    opt.close()


@pytest.mark.parametrize("n_nodes,n_edges", [(256, 255), (257, 255), (256, 256), (257, 256), (256, 257), (257, 257), (256, 513), (257, 513)])
def test_reductions_at_block_edges(n_nodes, n_edges):
    """chi2's partial sums and the assembly at 256 lanes a block: one edge or node less, exactly full, one more, two blocks
    and one.  The first n_edges edges of a banded graph: its chain first ((257, 255) leaves the last node without an edge)."""
    g = ref.banded(n_nodes, 3, 7 * n_nodes + n_edges, far=0)
    assert len(g["edges"]) >= n_edges
    g = dict(g, edges=g["edges"][:n_edges], means=g["means"][:n_edges], infos=g["infos"][:n_edges])
    opt = _optimizer(g)
    want_chi2 = ref.chi2(g["poses"], g["edges"], g["means"], g["infos"])
    h, grad = ref.linear_system(g["poses"], g["edges"], g["means"], g["infos"])
    h, grad = h.toarray(), grad.reshape(-1, 3)
    assert abs(opt.chi2() - want_chi2) <= 1e-9 * want_chi2
    chi2, diag, got_grad = opt.linearise()
    assert abs(chi2 - want_chi2) <= 1e-9 * want_chi2
    for i in range(n_nodes):
        want = h[3 * i:3 * i + 3, 3 * i:3 * i + 3]
        assert np.abs(diag[i] - want).max() <= 1e-9 * np.abs(want).max(), i
        assert np.abs(got_grad[i] - grad[i]).max() <= 1e-9 * np.abs(grad[i]).max(), i
    opt.close()


INDEFINITE = [[1.0, 2.0, 0.0], [2.0, 1.0, 0.0], [0.0, 0.0, 1.0]]  # a positive diagonal, eigenvalues 3, -1, 1


def _failing(kind):
    """a graph whose damped system is not positive definite.  indefinite: the last node's only edge has the information
    INDEFINITE, so its diagonal block is R^T L R (the other edges' information is hundreds of times larger: chi2 stays
    positive, the run reaches its first solve); isolated: the last node has no edge, its block is zero"""
    from yag_slam_amd.posegraph import PoseGraphOptimizer
    g = ref.banded(6, 3, 11, far=0)
    opt = PoseGraphOptimizer()
    for i, p in enumerate(g["poses"]):
        opt.add_node(*p, i)
    last = 0
    for (a, b), mean, info in zip(g["edges"].tolist(), g["means"], g["infos"]):
        if 5 in (a, b):
            if kind == "isolated" or last:
                continue
            last, info = 1, np.array(INDEFINITE)
        opt.add_constraint(a, b, *mean, info)
    return opt


@pytest.mark.parametrize("kind", ["indefinite", "isolated"])
@pytest.mark.parametrize("band", [0, 3])
def test_a_system_that_is_not_positive_definite_is_refused(kind, band):
    from yag_slam_amd._capi import YmError
    opt = _failing(kind)
    opt.band = band
    before = opt.nodes_xyt.copy()
    chi2 = opt.chi2()
    assert chi2 > 0.0
    with pytest.raises(YmError, match="not positive definite"):
        opt.compute(100, 1.0e-4, True, 1.0e-9, 50)
    assert opt.nodes_xyt.tobytes() == before.tobytes()
    # the handle still works, and holds what it held
    assert opt.chi2() == chi2
    assert opt.solve_step(BAND_LAMBDA, max_cg_iters=0)[5] & PIVOT
    with pytest.raises(YmError, match="not positive definite"):
        opt.compute(100, 1.0e-4, False, 1.0e-9, 5)
    assert opt.nodes_xyt.tobytes() == before.tobytes() and opt.chi2() == chi2
    opt.close()


def test_band_range_and_zero_steps(systems):
    from yag_slam_amd._capi import YmError
    g = systems(2, 12, 2)[0]
    opt = _optimizer(g)
    before = opt.nodes_xyt.copy()
    for band in (17, -2):
        opt.band = band
        with pytest.raises(YmError, match=r"band %d: -1 \(automatic\) or 0 \.\. 16" % band):
            opt.compute(100, 1.0e-4, True, 1.0e-9, 50)
        with pytest.raises(YmError, match=r"band %d: -1 \(automatic\) or 0 \.\. 16" % band):
            opt.solve_step(BAND_LAMBDA)
    with pytest.raises(YmError, match="cg_tol > 0"):
        opt.solve_step(BAND_LAMBDA, band=2, max_cg_iters=-1)
    assert opt.nodes_xyt.tobytes() == before.tobytes()
    opt.band = -1
    rep = opt.compute(0, 1.0e-4, True, 1.0e-9, 50)
    assert (rep.status, rep.lm_steps, rep.accepted, rep.cg_iterations) == (0, 0, 0, 0) and rep.chi2_final == rep.chi2_initial == opt.chi2()
    assert opt.nodes_xyt.tobytes() == before.tobytes()
    opt.close()
