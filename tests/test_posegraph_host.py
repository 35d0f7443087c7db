"""CPU-only checks of the pose-graph optimiser: the yardstick (tests/posegraph_ref.py) checks itself, and
`yag_slam_amd.posegraph.PoseGraphOptimizer` validates its arguments and refuses to compute without a device."""
import numpy as np
import pytest

from tests import posegraph_ref as ref

# Exact recovery runs from lambda0 = 1e-8, not the reference call's 1e-4.  The stop rule chi2 <= 1e-18 chi2_0 bounds the pose
# error only by sqrt(1e-18 chi2_0 / mu), mu the smallest eigenvalue of H: 2e-7 for the drifted 64-ring (chi2_0 = 6.7e3,
# mu = 0.16).  How far below that bound the loop ends is decided by the last step's contraction, which for a damped step is
# about lambda * max diag(H) / mu (diag(H) up to 2e4 here): with lambda still 4e-7 after eight halvings from 1e-4 the
# yardstick itself stops 1.6e-9 from the truth, with 1e-8 the steps are Gauss-Newton's and it stops 5e-13 from it.
RECOVERY_LAMBDA = 1e-8


def test_yardstick_jacobians_match_finite_differences():
    g = ref.ring(16, noise=0.05, seed=3)
    poses, edges, means = g["poses"], g["edges"], g["means"]
    ja, jb = ref.jacobians(poses, edges)
    h = 1e-6
    for m in (0, 5, len(edges) - 1):
        a, b = edges[m]
        for node, jac in ((a, ja[m]), (b, jb[m])):
            for k in range(3):
                hi, lo = poses.copy(), poses.copy()
                hi[node, k] += h
                lo[node, k] -= h
                fd = (ref.residuals(hi, edges[m:m + 1], means[m:m + 1])[0] - ref.residuals(lo, edges[m:m + 1], means[m:m + 1])[0]) / (2 * h)
                # central differences of sin / cos times distances of a few metres: h^2 / 6 * |d| ~ 1e-11, rounding 1e-16 / h ~ 1e-10
                assert np.allclose(fd, jac[:, k], rtol=0, atol=1e-8), (m, node, k)


def test_yardstick_residual_wraps_and_information_counts():
    poses = np.array([[0.0, 0.0, 3.1], [1.0, 0.0, -3.1]])
    edges = np.array([[0, 1]], dtype=np.int32)
    e = ref.residuals(poses, edges, np.zeros((1, 3)))
    assert abs(e[0, 2] - (2 * np.pi - 6.2)) < 1e-15
    assert float(ref.wrap(np.pi)) == np.pi and float(ref.wrap(-np.pi)) == np.pi
    info = np.array([[[2.0, 0.5, 0], [0.5, 3.0, 0], [0, 0, 4.0]]])
    assert abs(ref.chi2(poses, edges, np.zeros((1, 3)), info) - float(e[0] @ info[0] @ e[0])) < 1e-12


def test_yardstick_recovers_the_noise_free_ring():
    g = ref.ring(64, noise=0.0, seed=1)
    assert np.abs(g["poses"] - g["truth"]).max() > 0.5  # the start has drifted
    poses, rep = ref.optimize(g, lam=RECOVERY_LAMBDA)
    d = poses - g["truth"]
    d[:, 2] = ref.wrap(d[:, 2])
    assert np.abs(d).max() < 1e-11, np.abs(d).max()
    assert rep["chi2_final"] <= 1e-18 * rep["chi2_initial"] and rep["status"] == 2


def test_yardstick_gradient_vanishes_at_the_noisy_answer():
    g = ref.ring(600, noise=0.02, seed=2)
    poses, rep = ref.optimize(g)
    assert rep["status"] == 1 and rep["chi2_final"] < 1e-2 * rep["chi2_initial"]
    _, g0 = ref.linear_system(g["poses"], g["edges"], g["means"], g["infos"])
    _, g1 = ref.linear_system(poses, g["edges"], g["means"], g["infos"])
    # the free nodes' gradient: seven orders below the start's (the last accepted step gained <= 1e-9 chi2)
    assert np.abs(g1[3:]).max() < 1e-7 * np.abs(g0[3:]).max()


def test_optimizer_validates_arguments_without_a_device():
    from yag_slam_amd.posegraph import PoseGraphOptimizer, SPA2d
    assert SPA2d is PoseGraphOptimizer
    opt = PoseGraphOptimizer()
    eye = [[1.0, 0, 0], [0, 1.0, 0], [0, 0, 1.0]]
    opt.add_node(0.0, 0.0, 0.0, 0)
    with pytest.raises(ValueError, match="next node is 1"):
        opt.add_node(1.0, 0.0, 0.0, 5)
    with pytest.raises(ValueError, match="not finite"):
        opt.add_node(float("nan"), 0.0, 0.0, 1)
    opt.add_node(1.0, 0.5, 0.25, 1)
    with pytest.raises(ValueError, match="out of range"):
        opt.add_constraint(0, 2, 1.0, 0.0, 0.0, eye)
    with pytest.raises(ValueError, match="itself"):
        opt.add_constraint(1, 1, 1.0, 0.0, 0.0, eye)
    with pytest.raises(ValueError, match="3 x 3"):
        opt.add_constraint(0, 1, 1.0, 0.0, 0.0, [1.0, 1.0, 1.0])
    with pytest.raises(ValueError, match="not finite"):
        opt.add_constraint(0, 1, float("inf"), 0.0, 0.0, eye)
    with pytest.raises(ValueError, match="positive diagonal"):
        opt.add_constraint(0, 1, 1.0, 0.0, 0.0, [[1.0, 0, 0], [0, 0.0, 0], [0, 0, 1.0]])
    opt.add_constraint(0, 1, 1.0, 0.0, 0.0, np.eye(3))
    assert opt.n_constraints == 1
    # the node sequence before any compute: the poses as added
    nodes = opt.nodes
    assert len(nodes) == 2 and (nodes[1].x, nodes[1].y, nodes[1].yaw) == (1.0, 0.5, 0.25)
    assert [n.x for n in nodes] == [0.0, 1.0] and len(nodes[:1]) == 1 and nodes[:1][0].x == 0.0
    assert opt.nodes_xyt.shape == (2, 3)


def test_compute_without_a_device_raises():
    from yag_slam_amd import _capi
    from yag_slam_amd.posegraph import PoseGraphOptimizer
    if _capi.lib().ym_device_count() > 0:
        pytest.skip("a GPU is present")
    opt = PoseGraphOptimizer()
    opt.add_node(0.0, 0.0, 0.0, 0)
    opt.add_node(1.0, 0.0, 0.0, 1)
    opt.add_constraint(0, 1, 1.0, 0.0, 0.0, np.eye(3))
    with pytest.raises(_capi.YmError, match="no HIP device"):
        opt.compute(100, 1.0e-4, True, 1.0e-9, 50)
    with pytest.raises(_capi.YmError, match="no HIP device"):
        opt.chi2()


def test_opt_struct_layouts_match_the_header():
    import ctypes as C
    from yag_slam_amd import _capi
    assert C.sizeof(_capi.YmOptParams) == 4 * 4 + 2 * 8
    assert C.sizeof(_capi.YmOptReport) == 3 * 8 + 5 * 4 + 4


# ---- the cases of tests/test_gpu_posegraph_band.py: that they are the ones meant, and that the yardstick itself stays inside
# every condition the device is held to
BAND_WIDTHS = (1, 2, 6, 7, 13, 14, 16)  # the row of 9 (W + 1) values crosses 64 at W = 7 and 128 at W = 14
BAND_LAMBDA = 1e-4
CASES = [(W, n) for W in BAND_WIDTHS for n in sorted({2, 3, 5, 6, 7, 12, 13, W + 1, W + 2, 40, 257})]
# The worst backward error of LAPACK's banded Cholesky (scipy.linalg.solveh_banded) over CASES, as measured by
# test_band_cases_reference_backward_error: 9.81e-17, 0.88 * 2^-53.
ETA_REF = 9.9e-17
ETA_BOUND = 32.0 * max(ETA_REF, 2.0 ** -53)
# The end-to-end cases (n, W, far, seed).  The seed is 100 W + n unless a gain of the yardstick's run came within a factor 2
# of the stop rule 1e-9 chi2 (test_end_to_end_cases_stop_clear_of_the_rule): then the next of 100 W + n + 1000 k that does not.
E2E_CASES = [(40, 1, 2, 140), (40, 1, 0, 1140), (40, 7, 2, 740), (40, 7, 0, 740), (40, 14, 2, 1440), (40, 14, 0, 1440),
             (40, 16, 2, 1640), (40, 16, 0, 1640), (257, 14, 2, 2657), (257, 14, 0, 2657)]


def case_seed(W, n):
    return 100 * W + n


def far_applies(W, n):
    return n > W + 2


@pytest.fixture(scope="module")
def band_systems():
    """(graph, A, M, b) of every case with far = 2, computed once"""
    out = {}
    for W, n in CASES:
        g = ref.banded(n, W, case_seed(W, n))
        out[W, n] = (g,) + ref.damped_system(g, BAND_LAMBDA, W)
    return out


def _distances(g):
    e = g["edges"].astype(int)
    return np.abs(e[:, 0] - e[:, 1]), e[:, 0] > e[:, 1], (e == 0).any(axis=1)


def test_band_cases_are_the_ones_meant(band_systems):
    reversed_far = 0
    for (W, n), (g, A, M, b) in band_systems.items():
        d, rev, at0 = _distances(g)
        have = {tuple(sorted(p)) for p in g["edges"].tolist()}
        assert all((i, i + 1) in have for i in range(n - 1)) and all((i, i + W) in have for i in range(n - W))
        assert (d <= W).sum() >= n - 1
        if n >= 3:  # the transposing branch of the assembly runs on a block that reaches the band
            assert (rev & (d <= W) & ~at0).any(), (W, n)
        if n > 3:   # one pair twice, clear of node 0
            pairs = [tuple(sorted(p)) for p in g["edges"].tolist()]
            twice = [p for p in set(pairs) if pairs.count(p) == 2]
            assert len(twice) == 1 and twice[0][0] != 0 and twice[0][1] - twice[0][0] <= W, (W, n)
        assert (d > W).sum() == (2 if far_applies(W, n) else 0), (W, n)
        reversed_far += int((rev & (d > W)).sum())
        if n > 20:  # the far edges are out of the device's reach too: band -1 picks W
            assert ref.auto_band(g) == W, (W, n)
        # with far = 0 the band holds the whole system
        g0 = ref.banded(n, W, case_seed(W, n), far=0)
        A0, M0, _ = ref.damped_system(g0, BAND_LAMBDA, W)
        assert np.array_equal(A0, M0), (W, n)
        assert np.array_equal(A[:3], np.eye(3, 3 * n)) and np.array_equal(A, A.T) and not b[:3].any()
    assert reversed_far >= 1


def test_band_cases_reference_backward_error(band_systems):
    import scipy.linalg as sla
    worst = 0.0
    for (W, n), (g, A, M, b) in band_systems.items():
        np.linalg.cholesky(M)  # positive definite (raises LinAlgError otherwise)
        np.linalg.cholesky(A)
        u = 3 * W + 2
        ab = np.zeros((u + 1, 3 * n))
        for k in range(min(u, 3 * n - 1) + 1):
            ab[u - k, k:] = np.diag(M, k)
        z = sla.solveh_banded(ab, b)
        worst = max(worst, ref.backward_error(M, z, b))
    print("ETA_REF: worst backward error of solveh_banded over %d cases %.3g (%.2f * 2^-53)" % (len(CASES), worst, worst * 2.0 ** 53))
    assert worst <= ETA_REF


def test_band_cases_pcg_counts(band_systems):
    counts = {}
    for (W, n), (g, A, M, b) in band_systems.items():
        g0 = ref.banded(n, W, case_seed(W, n), far=0)
        A0, M0, b0 = ref.damped_system(g0, BAND_LAMBDA, W)
        x0, it0, res0 = ref.pcg(A0, M0, b0, 1e-10, 50)
        assert it0 == 1 and res0 <= 1e-15, (W, n, it0, res0)
        x, it, res = ref.pcg(A, M, b, 1e-10, 50)
        # A - M has rank <= 6 a far edge, so M^-1 A has at most 6 far + 1 distinct eigenvalues
        assert it <= 13 and res <= 1e-10, (W, n, it, res)
        assert ref.backward_error(A, x, b) <= 1e-10
        if not far_applies(W, n):
            assert it == 1
        counts[W, n] = it
    print("pcg iterations with two far edges: " + ", ".join("W%d n%d: %d" % (W, n, it) for (W, n), it in counts.items() if far_applies(W, n)))


def _gains_over_stop(g):
    history = []
    _, rep = ref.optimize(g, history=history)
    chi = [rep["chi2_initial"]] + history
    return rep, [(chi[i] - chi[i + 1]) / (1e-9 * chi[i]) for i in range(len(history))]


def test_end_to_end_cases_stop_clear_of_the_rule():
    graphs = [("banded %d / %d far %d" % (n, W, far), ref.banded(n, W, seed, far=far)) for n, W, far, seed in E2E_CASES]
    graphs.append(("grid5", ref.grid(5, 5, noise=0.02, seed=3)))
    for name, g in graphs:
        rep, ratio = _gains_over_stop(g)
        print("%s: status %d after %d steps, gains over the stop rule %s" % (name, rep["status"], rep["lm_steps"], ["%.3g" % r for r in ratio]))
        assert rep["status"] == 1 and 4 <= rep["lm_steps"] <= 10
        # no accepted step (the last, which stops the run, or an earlier one, which does not) within a factor 2 of the rule
        assert all(r < 0.5 or r > 2.0 for r in ratio), (name, ratio)
        assert ratio[-1] < 0.5
