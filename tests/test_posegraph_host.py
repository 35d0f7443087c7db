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
