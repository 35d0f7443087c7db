"""The yardstick of tests/test_gpu_yag_ties.py, checked where no GPU is needed.

1. The numpy restatement of the "yagpy" rounding rule (tests/yag_ties_ref.py, rule_sums) against sum volumes the REFERENCE's own
   score_world_points_on_grid produced (tests/golden/*.npz: coarse_sums, fine_sums), with numpy's trig as the reference takes it: bit for
   bit.  That ties the yardstick to the reference, not to the kernels it is going to judge.
2. The aiming routine against a simulated device: numpy's cos and sin moved by up to an ulp, as a deterministic function of the operand
   (what a device's libm is).  On every configuration the GPU tests use, the rounds of the attack must fill every band those tests
   require -- the check that their conditions can be met by the inputs alone."""
import numpy as np
import pytest

from tests import yag_ties_ref as R
from tests.util import PlainScan, load_case

SUM_CASES = ["sums_cfg2", "sums_dirty_rot", "sums_far", "sums_loop", "sums_near_threshold"]
SUM_SMALL = ["small_pen0_fine1", "small_pen1_fine1", "small_dirty_rot"]


@pytest.mark.parametrize("name", SUM_CASES + SUM_SMALL)
def test_rule_as_written_gives_the_reference_made_sum_volumes(name):
    from oracle import oracle as orc
    c = load_case(name)
    z, q = c["z"], c["query"]
    res = c["cfg"].get("resolution", 0.01)
    # the grid: the CPU oracle's (held to the reference's own grids in tests/test_oracle_golden.py); where the fixture carries the
    # reference's grid itself, that one
    o = orc.Oracle(c["cfg"], "yagpy")
    o.match_scan(q, c["base"], c["penalty"], c["do_fine"])
    grid, _ = o.grid_u8()
    G = int(z["grid_size"])
    assert grid.shape == (G, G)
    if "grid_nz_val" in z.files:
        ref_grid = np.zeros((G, G), dtype=np.uint8)
        ref_grid[z["grid_nz_y"], z["grid_nz_x"]] = (100 * z["grid_nz_val"]).astype(np.int64)
        assert np.array_equal(grid, ref_grid)
        grid = ref_grid
    ox, oy = (float(z["q_pose"][i]) - 0.5 * (G - 1) * res for i in (0, 1))  # scan_matching.py:188-189 of the reference
    ok = ~((q.ranges > q.range_threshold) | np.isnan(q.ranges))
    ang = q.min_angle + np.arange(len(q.ranges)) * q.angle_increment
    pts = np.stack([q.ranges * np.cos(ang), q.ranges * np.sin(ang)], axis=1)[ok]
    checked = 0
    for pass_ in ("coarse", "fine"):
        if pass_ + "_sums" not in z.files:
            continue
        tv = z[pass_ + "_tvals"]
        f = R.make_frame(z[pass_ + "_xvals"], z[pass_ + "_yvals"], tv, np.stack([np.cos(tv), np.sin(tv)], axis=1), pts, ox, oy, res, G, G)
        assert np.array_equal(R.rule_sums(f, grid), z[pass_ + "_sums"].astype(np.int64)), pass_
        # the same through a window that holds only the cells the readings reach: what the device keeps
        ys, xs = np.nonzero(grid)
        x0, y0 = max(0, xs.min() - 3), max(0, ys.min() - 3)
        assert np.array_equal(R.rule_sums(f, grid[y0:ys.max() + 4, x0:xs.max() + 4], (x0, y0)), z[pass_ + "_sums"].astype(np.int64)), pass_
        checked += 1
    assert checked >= 1


# ---- a simulated device ------------------------------------------------------------------------------------------------
def _nudge(values, operand):
    """values moved by -1, 0 or +1 ulp, decided by the operand's bits alone (a libm is a function)"""
    bits = np.asarray(operand, dtype=np.float64).view(np.uint64)
    pick = ((bits * np.uint64(0x9E3779B97F4A7C15)) >> np.uint64(62)).astype(np.int64)  # 0 .. 3
    out = np.where(pick == 0, np.nextafter(values, -np.inf), np.where(pick == 3, np.nextafter(values, np.inf), values))
    return out


def sim_cos(x):
    return _nudge(np.cos(x), x)


def sim_sin(x):
    return _nudge(np.sin(x), np.asarray(x) + 0.0)


class SimDevice:
    """the reference's match_scan geometry with the nudged trig: frames of both passes, the oracle's grid and coarse result"""

    def __init__(self, case):
        from oracle import oracle as orc
        self.cfg = R.case_config(case)
        self.problem = R.case_problem(case)
        self.orc = orc.Oracle(self.cfg, "yagpy")
        self.orc_module = orc
        self.rounds = 0

    def scan(self, ranges, pose):
        return PlainScan(ranges, R.MIN_ANGLE, R.ANGLE_INCREMENT, 0.05, 6.0, pose)

    def measure(self, role, ranges):
        self.rounds += 1
        cfg, res = self.cfg, self.cfg["resolution"]
        pose = self.problem["queries"][role][1]
        base = [self.scan(r, p) for r, p in self.problem["base"]]
        ro = self.orc.match_scan(self.scan(ranges, pose), base, True, False)  # (the coarse pass alone: its mean is the fine pass's centre)
        grid, _ = self.orc.grid_u8()
        G = int(cfg["search_size"] / res + 1 + 2 * cfg["range_threshold"] / res)
        assert grid.shape == (G, G)
        ox, oy = pose[0] - 0.5 * (G - 1) * res, pose[1] - 0.5 * (G - 1) * res
        ang = (0.0 + R.MIN_ANGLE) + np.arange(len(ranges)) * R.ANGLE_INCREMENT
        pts = np.stack([ranges * sim_cos(ang), ranges * sim_sin(ang)], axis=1)
        lat = int(np.floor(cfg["search_size"] / (2 * res) + 1e-6)) + 1
        frames = []
        for centre, sxy, step, st, stt in ((pose, cfg["search_size"] * 0.5, res * 2, 0.349 * 0.5, 0.0349),
                                           (tuple(ro["pose"]), res * 2, res, 0.0349 * 0.5, 0.00349)):
            xv = np.arange(-sxy + centre[0], sxy + centre[0], step)
            yv = np.arange(-sxy + centre[1], sxy + centre[1], step)
            tv = np.arange(-st + centre[2], st + centre[2], stt)
            frames.append(R.make_frame(xv, yv, tv, np.stack([sim_cos(tv), sim_sin(tv)], axis=1), pts, ox, oy, res, G, G, roi_w=G,
                                       win_origin=0, win_w=G, lat_nx=lat, lat_ny=lat, lat_nt=len(tv) + 1, step_cells=2))
        return frames[0], frames[1], grid, (0, 0)


@pytest.mark.parametrize("case", sorted(R.CHAIN_CASES))
def test_aimed_readings_fill_every_band_on_a_simulated_device(case):
    dev = SimDevice(case)
    aimed = R.attack_chain_case(dev.measure, dev.problem)
    assert dev.rounds == 3  # every query once, with its readings as they come.  No retries.
    spec = R.CHAIN_CASES[case]
    far = abs(spec["shift"][0]) > 1000
    # ---- the regular query: accepted pairs only
    f0, _, _, _ = dev.measure("regular", aimed["regular"])
    counts, facts = R.band_counts(f0)
    assert R.proof_claim_holds(facts)
    dec = R.expected_decision(f0, facts)
    assert dec["regular"] and dec["failed"] == 0, dec
    for axis in ("x", "y"):
        assert counts[(axis, "inside_regular")] >= R.NEED, (axis, counts)
        assert counts[(axis, "just_outside")] >= R.NEED, (axis, counts)
        assert counts[(axis, "inside_irregular")] == 0
        if far:
            assert counts[(axis, "beyond_2m40")] >= R.NEED, (axis, counts)
    assert dec["checked"] >= 4 * R.NEED
    # ---- the fine query: its fine pass meets operands whose product and quotient round apart, where the bytes differ
    _, f1, grid, origin = dev.measure("fine", aimed["fine"])
    both, differ = R.rint_div_count(f1, grid, origin)
    if R.rint_div_reachable(spec):
        assert both >= R.NEED, (both, differ)
    else:
        assert differ == 0 or far, (both, differ)
    # ---- the irregular query: ties that fall differently along the axis
    g0, _, _, _ = dev.measure("irregular", aimed["irregular"])
    counts, facts = R.band_counts(g0)
    assert R.proof_claim_holds(facts)
    dec = R.expected_decision(g0, facts)
    assert not dec["regular"] and dec["failed"] >= 2 * R.NEED, dec
    for axis in ("x", "y"):
        assert counts[(axis, "inside_irregular")] >= R.NEED, (axis, counts)
