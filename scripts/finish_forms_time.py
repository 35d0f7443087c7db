"""Ad-hoc workload for kernel traces (development aid): the finish-stage and score kernels that bench.py's headline,
quick_time.py and stress_time.py never launch.  Batches of 256 chains finish in finish_kernel<1024>; with the region
correlate's scoring left to the score stage (debug option 21 = 2) and with the direct correlate (option 14 = 1) they pass
through score_kernel.  Single matches on the 47 x 47 x 21 lattice take fine_kernel<true>."""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from tests.util import cfg2_scans  # noqa: E402
from tests.test_gpu_parity import _mk_native  # noqa: E402
from yag_slam_amd.scan_matching import ScanMatcher  # noqa: E402

q, base = cfg2_scans()
nq, nb = _mk_native(q), [_mk_native(b) for b in base]
chains = [nb[i % 4:] if i % 2 else nb[:len(nb) - i % 5] for i in range(256)]
for option, value in ((None, None), (21, 2), (14, 1)):
    m = ScanMatcher()
    if option is not None:
        m.debug_option(option, value)
    for _ in range(12):
        per, best = m.match_scan_batch(nq, chains, True, True)
    print("batch of 256, option %s = %s: best %d, response %.6f" % (option, value, best, per[best].response))
    m.close()
m = ScanMatcher(dict(search_size=0.92))
assert m.coarse_dims() == (47, 47, 21)
for _ in range(60):
    r = m.match_scan(nq, nb, True, True)
print("single match on 47 x 47 x 21: response %.6f" % r.response)
m.close()
