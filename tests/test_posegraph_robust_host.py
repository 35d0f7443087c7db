"""CPU-only checks of the pose-graph optimiser's robust kernels and switchable constraints: the
yardstick tests/posegraph_robust_ref.py against tests/posegraph_ref.py and against itself, the cases of
tests/test_gpu_posegraph_robust.py (that they are the ones meant, and that the yardstick itself shows what the device is held
to), the header's prototypes, and the argument checks that need no device."""
import functools
import os
import shutil
import subprocess

import numpy as np
import pytest

from tests import posegraph_hold_ref as href
from tests import posegraph_ref as ref
from tests import posegraph_robust_ref as rr

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# ---- the linearisation cases of the device test: graphs cut to an exact number of edges
EDGE_COUNTS = (1, 255, 256, 257, 600)  # the block edges of the 256-lane kernels and their partial sums
HUBER_K, LIN_C = 1.5, 2.0


def lin_graph(family, count):
    """`count` edges of a seeded graph with noise 0.02, the first of a seeded order of all its edges (chain, skip and closing
    edges mixed; nodes that lose every edge keep their pose and get a zero block), every third edge with a kind in rotation
    and one in ten disabled (posegraph_robust_ref.with_settings)"""
    g = ref.ring(400, noise=0.02, seed=11) if family == "ring" else ref.banded(200, 7, 12, noise=0.02)
    assert len(g["edges"]) >= count
    pick = np.random.default_rng(5).permutation(len(g["edges"]))[:count]
    g = dict(g, edges=g["edges"][pick], means=g["means"][pick], infos=g["infos"][pick])
    return rr.with_settings(g, huber_k=HUBER_K, c=LIN_C)


# ---- the end-to-end cases of the device test.  EXTRA closures (the long-range edges ring() appends), a share of them replaced by
# constraints to a wrong place, the robust kernel on the closures only.  The seed of the replacement is, per ring and share, the
# first of 0, 1, 2, ... at which both kinds pass test_end_to_end_cases_decide_clear_of_rounding and
# test_the_yardstick_shows_what_robust_kernels_are_for (the 600-ring at 10 %: the first at which the plain run converges as well).
EXTRA = 100
E2E_C = 5.0
E2E_RINGS = {40: 1, 600: 2}  # nodes: the ring's seed
E2E_SEEDS = {(40, 0.01): 9, (40, 0.03): 1, (40, 0.10): 0, (600, 0.01): 52, (600, 0.03): 220, (600, 0.10): 116}
E2E_KINDS = ("cauchy", "geman_mcclure")
# one case with some nodes held (where they start: the run converges linearly, against the pull of the held poses; ring, share
# and held set are the first of those tried that pass test_end_to_end_cases_decide_clear_of_rounding)
HELD_CASE = (40, 0.10, "cauchy", (1, 2, 3))


@functools.lru_cache(maxsize=None)
def e2e_cases():
    """{(n, share): dict(graph, closures, wrong, plain=(poses, report), robust={kind: (graph, poses, report, decisions)})} and
    under the key "held" the held case: (graph, held, poses, report, decisions).  Computed once a process and never modified."""
    out = {}
    for (n, share), seed in E2E_SEEDS.items():
        base = ref.ring(n, noise=0.02, seed=E2E_RINGS[n], extra=EXTRA)
        g, closures, wrong = rr.with_wrong_closures(base, EXTRA, share, seed)
        robust = {}
        for kind in E2E_KINDS:
            gr, decisions = rr.robust_on(g, closures, kind, E2E_C), []
            poses, rep = rr.optimize(gr, decisions=decisions)
            robust[kind] = (gr, poses, rep, decisions)
        out[n, share] = dict(graph=g, closures=closures, wrong=wrong, plain=rr.optimize(g), robust=robust)
    n, share, kind, held = HELD_CASE
    gr, decisions = out[n, share]["robust"][kind][0], []
    poses, rep = rr.optimize(gr, held, decisions=decisions)
    out["held"] = (gr, held, poses, rep, decisions)
    return out


def clear_of_rounding(decisions, rep):
    """Whether no decision of a run of the yardstick could go the other way on the device.  The issue's rule: no keep / reject
    decision closer than 1e-6 relative.  A run that stops by the gain rule cannot meet that to the letter -- its last kept step
    gains at most 1e-9 F by that very rule, and the steps before it approach that -- so the rule is applied where a decision
    that went the other way would send the run elsewhere, and the rest is held to what protects it:
    - while F is more than 1e-6 F_final above F_final (the descent), every step's |F_trial - F| is at least 1e-6 F;
    - after that every step is kept, a step that does not end the run gains more than twice the stop rule's 1e-9 F, and the
      one that ends it less than half of that (the convention of tests/test_posegraph_host.py) but at least 1e-11 F: F is a
      sum of at most 1000 positive terms of a handful of roundings each, so two evaluations differ by at most about
      1e3 * 2^-53 = 1e-13 F, a hundred times less."""
    if rep["status"] != 1:
        return False
    final = rep["chi2_final"]
    for k, (before, trial) in enumerate(decisions):
        margin, last = abs(before - trial) / before, k == len(decisions) - 1
        if last:
            ok = trial < before and 1e-11 <= margin < 0.5e-9
        elif before - final > 1e-6 * final:
            ok = margin >= 1e-6
        else:
            ok = trial < before and margin > 2e-9
        if not ok:
            return False
    return True


# ---- the yardstick against itself and against the plain one
def test_rho_and_w_as_the_table_states_them():
    s = np.array([0.0, 0.5, 2.25, 2.26, 9.0, 1e4])
    assert np.array_equal(rr.rho(rr.NONE, 7.0, s), s) and np.array_equal(rr.weight(rr.NONE, 7.0, s), np.ones(6))
    k = 1.5
    assert np.allclose(rr.rho(rr.HUBER, k, s), [0.0, 0.5, 2.25, 2 * k * np.sqrt(2.26) - k * k, 2 * k * 3 - k * k, 2 * k * 100 - k * k], rtol=1e-15)
    assert np.allclose(rr.weight(rr.HUBER, k, s), [1, 1, 1, k / np.sqrt(2.26), k / 3, k / 100], rtol=1e-15)
    c = 2.0
    assert np.allclose(rr.rho(rr.CAUCHY, c, s), 4 * np.log1p(s / 4), rtol=1e-15)
    assert np.allclose(rr.weight(rr.CAUCHY, c, s), 1 / (1 + s / 4), rtol=1e-15)
    assert np.allclose(rr.rho(rr.GEMAN_MCCLURE, c, s), 4 * s / (4 + s), rtol=1e-15)
    assert np.allclose(rr.weight(rr.GEMAN_MCCLURE, c, s), (4 / (4 + s)) ** 2, rtol=1e-15)
    # a kind per element, and huber(1e150) is the plain square to the bit
    assert np.array_equal(rr.rho([rr.NONE, rr.HUBER], [1.0, 1e150], [3.0, 1e30]), [3.0, 1e30])
    assert np.array_equal(rr.weight(rr.HUBER, 1e150, s), np.ones(6))


def test_w_is_the_derivative_of_rho():
    """central differences of rho: the step h = 1e-5 s gives a truncation error of h^2 rho''' / 6 (relative 1e-10 and less for
    these kernels) and a rounding error of 2^-53 rho / h, about 1e-11 relative; huber's kink at k^2 is kept 1 % away"""
    s = np.concatenate([np.geomspace(1e-3, 1e5, 81), [2.2, 2.3]])
    for kind, p in ((rr.NONE, 1.0), (rr.HUBER, 1.5), (rr.CAUCHY, 2.0), (rr.GEMAN_MCCLURE, 2.0), (rr.CAUCHY, 30.0), (rr.GEMAN_MCCLURE, 0.1)):
        h = 1e-5 * s
        fd = (rr.rho(kind, p, s + h) - rr.rho(kind, p, s - h)) / (2 * h)
        w = rr.weight(kind, p, s)
        assert np.abs(fd - w).max() <= 1e-8 and np.all(np.abs(fd - w) <= 1e-6 * w + 1e-12), (kind, p)
    assert (np.abs(s - 2.25) > 0.02).all()


def test_a_plain_graph_is_the_old_yardstick_to_the_bit():
    for g, held in ((ref.ring(64, noise=0.02, seed=1), ()), (ref.banded(40, 7, 740), ()), (ref.ring(64, noise=0.02, seed=1), tuple(range(20)))):
        h1, g1 = rr.linear_system(g["poses"], g)
        h0, g0 = ref.linear_system(g["poses"], g["edges"], g["means"], g["infos"])
        assert h1.toarray().tobytes() == h0.toarray().tobytes() and g1.tobytes() == g0.tobytes()
        assert rr.cost(g["poses"], g) == rr.chi2(g["poses"], g)
        assert abs(rr.cost(g["poses"], g) - ref.chi2(g["poses"], g["edges"], g["means"], g["infos"])) <= 1e-13 * rr.cost(g["poses"], g)
        everywhere = dict(g, kinds=np.full(len(g["edges"]), rr.HUBER), params=np.full(len(g["edges"]), 1e150))
        (p1, r1), (p2, r2), (p0, r0) = rr.optimize(g, held), rr.optimize(everywhere, held), href.optimize(g, held)
        assert p1.tobytes() == p2.tobytes() and r1 == r2
        # (F is summed an edge at a time, posegraph_ref's chi2 in one einsum: the same steps, chi2 to rounding)
        assert np.abs(p1 - p0).max() <= 1e-12 and r1["lm_steps"] == r0["lm_steps"]
        assert abs(r1["chi2_final"] - r0["chi2_final"]) <= 1e-12 * r0["chi2_final"]


def test_the_weighted_system_is_the_gradient_of_the_cost():
    """g = sum w J^T L e is half the gradient of F = sum rho(e^T L e): central differences over every coordinate of three
    nodes.  h = 1e-6: truncation h^2 F''' / 6 and rounding 2^-53 F / h are both about 1e-9 of F's scale."""
    g = lin_graph("banded", 257)
    _, grad = rr.linear_system(g["poses"], g)
    scale = np.abs(grad).max()
    for node in (1, 57, 150):
        for k in range(3):
            hi, lo = g["poses"].copy(), g["poses"].copy()
            hi[node, k] += 1e-6
            lo[node, k] -= 1e-6
            fd = (rr.cost(hi, g) - rr.cost(lo, g)) / 2e-6
            assert abs(fd - 2.0 * grad[3 * node + k]) <= 1e-6 * scale, (node, k)


def test_disabled_edges_are_as_if_never_added():
    g = lin_graph("ring", 600)
    on = g["enabled"]
    cut = dict(g, edges=g["edges"][on], means=g["means"][on], infos=g["infos"][on], kinds=g["kinds"][on], params=g["params"][on],
               enabled=np.ones(int(on.sum()), dtype=bool))
    assert abs(rr.cost(g["poses"], g) - rr.cost(g["poses"], cut)) <= 1e-13 * rr.cost(g["poses"], g)
    assert abs(rr.chi2(g["poses"], g) - rr.chi2(g["poses"], cut)) <= 1e-13 * rr.chi2(g["poses"], g)
    (h1, g1), (h0, g0) = rr.linear_system(g["poses"], g), rr.linear_system(g["poses"], cut)
    assert np.abs(h1.toarray() - h0.toarray()).max() <= 1e-12 * np.abs(h0.toarray()).max() and np.abs(g1 - g0).max() <= 1e-12 * np.abs(g0).max()
    s, w = rr.edge_terms(g["poses"], g)
    assert (w[~on] == 0).all() and (s[~on] > 0).all() and (w[on] > 0).all()


# ---- the cases of the device test
def test_linearisation_cases_are_the_ones_meant():
    for family in ("ring", "banded"):
        for count in EDGE_COUNTS:
            g = lin_graph(family, count)
            assert len(g["edges"]) == count
            kinds, params, enabled = rr.settings(g)
            assert (kinds[::3] != 0).all() and (np.delete(kinds, np.arange(0, count, 3)) == 0).all()
            assert int((~enabled).sum()) == (count + 4) // 10
            s, w = rr.edge_terms(g["poses"], g)
            hub = (kinds == rr.HUBER) & enabled
            if count >= 255:  # (one edge is on one side; from 255 on both branches of Huber occur)
                assert {rr.HUBER, rr.CAUCHY, rr.GEMAN_MCCLURE} <= set(kinds.tolist())
                assert (s[hub] <= HUBER_K ** 2).any() and (s[hub] > HUBER_K ** 2).any(), (family, count)
                assert ((kinds != 0) & ~enabled).any()  # a robust edge that is disabled
                assert rr.cost(g["poses"], g) < 0.9 * rr.chi2(g["poses"], g)
    # the one-edge graphs between them: huber's inlier branch on the ring, its outlier branch on the banded graph
    sides = [rr.edge_terms(g["poses"], g)[0][0] <= HUBER_K ** 2 for g in (lin_graph("ring", 1), lin_graph("banded", 1))]
    assert sorted(sides) == [False, True], sides


def test_end_to_end_cases_are_the_ones_meant():
    cases = e2e_cases()
    for (n, share), seed in E2E_SEEDS.items():
        c = cases[n, share]
        g, closures, wrong = c["graph"], c["closures"], c["wrong"]
        assert len(g["poses"]) == n and len(closures) == EXTRA and len(wrong) == round(share * EXTRA) >= 1
        assert (np.abs(g["edges"][closures, 0].astype(int) - g["edges"][closures, 1]) > 20).all()
        # a wrong closure contradicts the truth by metres; a right one by its noise
        s_truth, _ = rr.edge_terms(g["truth"], g)
        right = np.setdiff1d(closures, wrong)
        assert s_truth[wrong].min() > 1e3 and s_truth[right].max() < 40
        for kind in E2E_KINDS:
            kinds, params, enabled = rr.settings(c["robust"][kind][0])
            assert (kinds[closures] == rr.KIND_OF[kind]).all() and (np.delete(kinds, closures) == 0).all() and enabled.all()
    gr, held, poses, rep, _ = cases["held"]
    assert poses[list(held)].tobytes() == gr["poses"][list(held)].tobytes() and 0 not in held


def test_end_to_end_cases_decide_clear_of_rounding():
    cases = e2e_cases()
    runs = [("%d / %g %s" % (n, share, kind), cases[n, share]["robust"][kind][2:]) for (n, share) in E2E_SEEDS for kind in E2E_KINDS]
    runs.append(("held", cases["held"][3:]))
    for name, (rep, decisions) in runs:
        margins = ["%.2g" % (abs(a - b) / a) for a, b in decisions]
        print("%s: status %d, %d of %d steps kept, F %.6g -> %.6g, |F_trial - F| / F %s"
              % (name, rep["status"], rep["accepted"], rep["lm_steps"], rep["chi2_initial"], rep["chi2_final"], margins))
        assert len(decisions) == rep["lm_steps"] >= 4
        assert clear_of_rounding(decisions, rep), name


def test_the_yardstick_shows_what_robust_kernels_are_for():
    cases = e2e_cases()
    for (n, share) in E2E_SEEDS:
        c = cases[n, share]
        g, closures, wrong = c["graph"], c["closures"], c["wrong"]
        right = np.setdiff1d(closures, wrong)
        plain_err = rr.pose_error(c["plain"][0], g["truth"])
        for kind in E2E_KINDS:
            gr, poses, rep, _ = c["robust"][kind]
            err = rr.pose_error(poses, g["truth"])
            _, w = rr.edge_terms(poses, gr)
            print("%d / %g %s: error against truth plain %.3g, robust %.3g (%.0f times); w of wrong closures <= %.2g, of right ones >= %.2g"
                  % (n, share, kind, plain_err, err, plain_err / err, w[wrong].max(), w[right].min()))
            assert plain_err >= 10.0 * err
            assert w[wrong].max() < w[right].min()


def test_disabling_the_wrong_closures_is_the_graph_without_them():
    c = e2e_cases()[40, 0.10]
    g, wrong = c["graph"], c["wrong"]
    keep = np.setdiff1d(np.arange(len(g["edges"])), wrong)
    cut = dict(g, edges=g["edges"][keep], means=g["means"][keep], infos=g["infos"][keep])
    enabled = np.ones(len(g["edges"]), dtype=bool)
    enabled[wrong] = False
    (p1, r1), (p0, r0) = rr.optimize(dict(g, enabled=enabled)), ref.optimize(cut)
    assert np.abs(p1 - p0).max() <= 1e-9 and r1["lm_steps"] == r0["lm_steps"]


# ---- the interface without a device
PROTOS = """
int (*p_set_robust)(ym_graph *, const int32_t *, int, int, double) = ym_graph_set_robust;
int (*p_enable)(ym_graph *, const int32_t *, int, int) = ym_graph_enable;
int (*p_edge_terms)(ym_graph *, double *, double *) = ym_graph_edge_terms;
int (*p_cost)(ym_graph *, double *) = ym_graph_cost;
"""
FUNCS = ("ym_graph_set_robust", "ym_graph_enable", "ym_graph_edge_terms", "ym_graph_cost")


def test_the_prototypes_compile_from_the_header(tmp_path):
    import ctypes as C
    from yag_slam_amd import _capi
    L = _capi.lib()
    for f in FUNCS:
        assert f in _capi.EXPORTS and hasattr(L, f), f
    vp, ip, dp = C.c_void_p, C.POINTER(C.c_int32), C.POINTER(C.c_double)
    assert list(L.ym_graph_set_robust.argtypes) == [vp, ip, C.c_int, C.c_int, C.c_double]
    assert list(L.ym_graph_enable.argtypes) == [vp, ip, C.c_int, C.c_int]
    assert list(L.ym_graph_edge_terms.argtypes) == [vp, dp, dp] and list(L.ym_graph_cost.argtypes) == [vp, dp]
    cc = shutil.which("cc") or shutil.which("gcc") or shutil.which("clang")
    assert cc, "no C compiler to read the header with"
    src = tmp_path / "protos.c"
    src.write_text('#include <stdio.h>\n#include "yagmatch.h"\n%s\nint main(void) { printf("%%d %%d %%d %%d\\n", YM_ROBUST_NONE, YM_ROBUST_HUBER, '
                   'YM_ROBUST_CAUCHY, YM_ROBUST_GEMAN_MCCLURE); return 0; }\n' % PROTOS)
    obj = str(tmp_path / "protos.o")
    subprocess.run([cc, "-Wall", "-Werror", "-I", os.path.join(REPO, "include"), "-c", "-o", obj, str(src)], check=True, capture_output=True)
    stub = tmp_path / "stubs.c"  # (the entries are only named, never called: the program links against empty stand-ins)
    stub.write_text("".join("int %s(void) { return 0; }\n" % f for f in FUNCS))
    exe = str(tmp_path / "protos")
    subprocess.run([cc, "-o", exe, obj, str(stub)], check=True, capture_output=True)
    assert subprocess.run([exe], check=True, capture_output=True, text=True).stdout.split() == ["0", "1", "2", "3"]
    from yag_slam_amd.posegraph import ROBUST_KINDS
    assert ROBUST_KINDS == {"huber": 1, "cauchy": 2, "geman_mcclure": 3} == rr.KIND_OF


def _two_nodes():
    from yag_slam_amd.posegraph import PoseGraphOptimizer
    opt = PoseGraphOptimizer()
    opt.add_node(0.0, 0.0, 0.0, 0)
    opt.add_node(1.0, 0.0, 0.0, 1)
    return opt


def test_robust_arguments_are_refused_without_a_device():
    opt = _two_nodes()
    eye = np.eye(3)
    assert opt.add_constraint(0, 1, 1.0, 0.0, 0.0, eye) == 0
    for bad, match in ((("tukey", 1.0), "kind"), ((1, 1.0), "kind"), (("huber", 0.0), "positive"), (("cauchy", -2.0), "positive"),
                       (("cauchy", float("nan")), "positive"), (("geman_mcclure", float("inf")), "positive"), (("huber", "k"), "number"),
                       ("huber", "kind, parameter"), (("huber",), "kind, parameter"), (5.0, "kind, parameter")):
        with pytest.raises(ValueError, match=match):
            opt.add_constraint(0, 1, 1.0, 0.0, 0.0, eye, robust=bad)
        with pytest.raises(ValueError, match=match):
            opt.set_robust([0], bad)
    assert opt.n_constraints == 1 and opt._h is None  # nothing of a refused call is kept, the library was not touched
    assert opt.add_constraint(1, 0, -1.0, 0.0, 0.0, eye, robust=("cauchy", 2.0)) == 1
    assert opt.add_constraint(0, 1, 1.0, 0.0, 0.0, eye, ("huber", 1.5)) == 2
    for call in (opt.enable, opt.disable, lambda e: opt.set_robust(e, ("huber", 1.0)), lambda e: opt.set_robust(e, None)):
        with pytest.raises(ValueError, match="out of range"):
            call([0, 3])
        with pytest.raises(ValueError, match="out of range"):
            call([-1])
        with pytest.raises(ValueError, match="integers"):
            call([0.5])
        call([])
    opt.set_robust([0, 2], ("geman_mcclure", 3.0))
    opt.set_robust(np.array([1]), None)
    opt.enable([2])
    assert opt._h is None


def test_the_mapper_passes_the_keyword_only_when_set():
    from yag_slam_amd.mapping import LoopClosingMapper
    from tests.test_segments_host import _Scan

    class FourCalls:  # SPA2d's four calls, as the reference makes them: no keyword, nothing returned
        def __init__(self):
            self.nodes, self.edges = [], []

        def add_node(self, x, y, yaw, num):
            self.nodes.append(num)

        def add_constraint(self, a, b, x, y, yaw, info):
            self.edges.append((a, b))

        def compute(self, *a):
            pass

    with pytest.raises(ValueError, match="kind"):
        LoopClosingMapper(None, None, robust_closures=("tukey", 1.0))
    with pytest.raises(ValueError, match="positive"):
        LoopClosingMapper(None, None, robust_closures=("cauchy", 0.0))
    for kw in ({}, {"robust_closures": None}):
        opt = FourCalls()
        mp = LoopClosingMapper(None, None, optimizer=opt, **kw)
        scans = [_Scan(i, 0.5 * i, 0.0) for i in range(3)]
        for s in scans:
            mp.add_vertex(s)
        eye = np.identity(3).tolist()
        assert mp.link_scans(scans[0], scans[1], eye) and mp.last_edge == 0
        assert mp.link_to_closest_scan_in_chain(scans[2], scans[:2], eye) and mp.last_edge == 1
        assert not mp.link_scans(scans[1], scans[0], eye) and mp.last_edge == 1
        assert opt.edges == [(0, 1), (1, 2)] and mp.robust_closures is None
        with pytest.raises(ValueError, match="edge_terms"):
            mp.closure_weights()
        with pytest.raises(TypeError):
            mp.drop_closures()  # max_weight is required
    # an optimiser that takes the keyword gets it for the edge that asks for it, and its index is kept
    from yag_slam_amd.posegraph import PoseGraphOptimizer
    opt = PoseGraphOptimizer()
    mp = LoopClosingMapper(None, None, optimizer=opt, robust_closures=("cauchy", 2.0))
    scans = [_Scan(i, 0.5 * i, 0.0) for i in range(3)]
    for s in scans:
        mp.add_vertex(s)
    mp.link_scans(scans[0], scans[1], np.identity(3).tolist())
    mp.link_scans(scans[0], scans[2], np.identity(3).tolist(), robust=mp.robust_closures)
    assert mp.last_edge == 1 and [op[0] for op in opt._new_ops] == ["robust"] and opt._new_ops[0][1].tolist() == [1]
