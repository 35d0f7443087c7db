"""INTEGRATION.md section 1 as a test: the REFERENCE's own `GraphSlam` (yag_slam/graph_slam.py of yag-slam) drives this
package's scan and pose classes -- process_scan, loop-closure bookkeeping, run_opt, serialize / binarize / unbinarize --
without a line of yag-slam changed.  The run is recorded in tests/golden/graphslam_run.{json,bin} by
tests/golden/make_golden_graphslam.py, which imports the reference (tests/refstubs.py); the matcher is a stand-in (no GPU
there), everything else in the run is the reference's code on yag_slam_amd objects.  The test checks the recording against
this package's scans, poses and map-file reader; tests/test_oracle_golden.py's opt-in regeneration test runs the
reference again and requires the same bytes."""
import json
import math
import os
from collections import namedtuple

import numpy as np
import pytest

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
N_SCANS = 40

Result = namedtuple("Result", "response covariance best_pose meta")


class StandInMatcher(object):
    """the plugin surface GraphSlam uses: .config + match_scan(...) -> response, covariance, best_pose"""

    def __init__(self, truth, loop=False):
        from yag_slam_amd.config import make_config
        self.config = make_config(None, loop=loop)
        self.truth = truth
        self.calls = []

    def match_scan(self, query, base_scans, penalty=True, do_fine=False):
        from yag_slam_amd.transform import Transform
        self.calls.append((query.num, [b.num for b in base_scans], penalty, do_fine))
        t = self.truth[query.num]
        return Result(0.9, [[0.01, 0, 0], [0, 0.01, 0], [0, 0, 0.001]], Transform(t[0], t[1], 0.0, t[2]), {})


def _scans(n):
    from yag_slam_amd.models import LocalizedRangeScan
    from yag_slam_amd.transform import Transform
    rng = np.random.default_rng(3)
    truth, scans = [], []
    for i in range(n):
        a = 2 * math.pi * i / 24.0          # two laps of a 1.5 m circle: the second lap revisits the first
        truth.append((1.5 * math.cos(a), 1.5 * math.sin(a), a + math.pi / 2))
        s = LocalizedRangeScan(rng.uniform(0.5, 9.0, 31), -1.3, 1.3, 2.6 / 30, 0.05, 30.0, 12.0, *truth[0])
        s.odom_pose = Transform(truth[i][0] + rng.normal(0, 0.01), truth[i][1] + rng.normal(0, 0.01), 0.0, truth[i][2])
        scans.append(s)
    return truth, scans


def test_reference_graphslam_runs_on_this_packages_objects():
    import zlib

    import msgpack
    from yag_slam_amd import mapfile
    with open(os.path.join(GOLDEN, "graphslam_run.json")) as f:
        rec = json.load(f)
    with open(os.path.join(GOLDEN, "graphslam_run.bin"), "rb") as f:
        blob = f.read()
    n = N_SCANS
    assert rec["n_scans"] == n
    truth, scans = _scans(n)  # the inputs of the recorded run, built again from this package's classes
    seq_calls = [(q, b, p, f) for q, b, p, f in rec["seq_calls"]]
    loop_calls = [(q, b, p, f) for q, b, p, f in rec["loop_calls"]]
    closed = rec["closed"]
    # the reference's call pattern reached the plugin: sequential match with penalty + fine on the running chain
    assert seq_calls[0] == (1, [0], True, True)
    assert all(len(c[1]) <= 5 for c in seq_calls if c[2])
    assert closed and min(closed) >= 24, closed              # second lap closes against the first
    assert any(c[2:] == (False, False) for c in loop_calls)  # coarse loop stage (graph_slam.py:220)
    assert any(c[2:] == (False, True) for c in seq_calls)    # fine stage on the moved copy (graph_slam.py:233-236)
    assert rec["opt_computes"] == len(closed) and rec["opt_nodes"] == n
    # run_opt rebuilt every pose through tiny_tf.tf.Transform
    assert rec["corrected_pose_classes"] == ["yag_slam_amd.transform.Transform"]
    for p, t in zip(rec["corrected_poses"], truth):
        assert abs(p[0] - t[0]) < 1e-12 and abs(p[2] - t[2]) < 1e-12
    # ---- the reference serialised this package's scans / poses / config, and read them back
    d = msgpack.unpackb(zlib.decompress(blob))
    assert d["scans"][3]["___name"] == "LocalizedRangeScan" and d["scans"][3]["corrected_pose"]["___name"] == "Transform"
    assert d["seq_matcher_config"]["___name"] == "ScanMatcherConfig" and d["seq_matcher_config"]["search_size"] == 0.5
    back = rec["unbinarized"]                                # the reference's reader (its own scan class)
    assert back["vertices"] == n and back["edges"] == rec["edges"]
    for r, p, s, q in zip(back["ranges"], back["corrected_poses"], scans, rec["corrected_poses"]):
        assert np.array_equal(np.asarray(r), s.ranges)
        assert abs(p[0] - q[0]) < 1e-12
        dth = p[2] - q[2]                                    # a quaternion keeps the heading modulo 2 pi
        assert abs(math.sin(dth)) < 1e-12 and math.cos(dth) > 0
    # ---- and this package's map-file reader agrees with the reference's on the same bytes
    mine = mapfile.loads(blob, matcher_factory=lambda cfg, loop: StandInMatcher(truth, loop))
    assert len(mine.scans) == n and len(mine.constraints) == rec["edges"]
    assert [s.num for s in mine.running_scans] == rec["running_scans"]
    for a, s, q, num in zip(mine.scans, scans, rec["corrected_poses"], rec["nums"]):
        assert np.array_equal(a.ranges, s.ranges) and a.num == num
        assert abs(a.corrected_pose.x - q[0]) < 1e-12 and abs(a.odom_pose.y - s.odom_pose.y) < 1e-12


def test_transform_speaks_tiny_tfs_constructor_and_attributes():
    from yag_slam_amd.transform import Transform
    t = Transform(1.0, 2.0, 0.0, 0.7)
    q = Transform(t.x, t.y, t.z, t.qx, t.qy, t.qz, t.qw)      # serde's cls(*[x, y, z, qx, qy, qz, qw])
    assert abs(q.euler[-1] - 0.7) < 1e-15 and (q.x, q.y) == (1.0, 2.0)
    k = Transform(x=1.0, y=2.0, z=0.0, qx=0.0, qy=0.0, qz=t.qz, qw=t.qw)
    assert abs(k.euler[-1] - 0.7) < 1e-15
    with pytest.raises(TypeError):
        Transform(0, 0, 0, 1, 2)
