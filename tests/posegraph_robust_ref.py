"""Test-side yardstick of the pose-graph optimiser's robust kernels and switchable constraints:
tests/posegraph_ref.py with a kind, a parameter and an enabled flag on every edge.  With s = e^T L e an edge costs rho(s) and
its blocks and gradient are weighted by w = rho'(s) taken at the poses of the linearisation; the objective F = sum rho takes
chi2's place in every rule of the Levenberg-Marquardt loop.  Held nodes as in tests/posegraph_hold_ref.py.

A graph is posegraph_ref's dict with, optionally, kinds (M,) int, params (M,) and enabled (M,) bool; without them every edge
is plain and enabled, and everything here is posegraph_ref's (posegraph_hold_ref's) to the bit: the weights are 1.0."""
import numpy as np
import scipy.sparse as sp
import scipy.sparse.linalg as spla

from tests import posegraph_hold_ref as href
from tests import posegraph_ref as ref

NONE, HUBER, CAUCHY, GEMAN_MCCLURE = 0, 1, 2, 3
KIND_OF = {"huber": HUBER, "cauchy": CAUCHY, "geman_mcclure": GEMAN_MCCLURE}


def rho(kind, p, s):
    """rho(s) of an enabled edge, elementwise"""
    kind, p, s = np.broadcast_arrays(np.asarray(kind), np.asarray(p, dtype=np.float64), np.asarray(s, dtype=np.float64))
    p2 = p * p
    out = np.array(s, dtype=np.float64)
    h = kind == HUBER
    out[h] = np.where(s[h] <= p2[h], s[h], 2.0 * p[h] * np.sqrt(s[h]) - p2[h])
    c = kind == CAUCHY
    out[c] = p2[c] * np.log1p(s[c] / p2[c])
    g = kind == GEMAN_MCCLURE
    out[g] = p2[g] * s[g] / (p2[g] + s[g])
    return out


def weight(kind, p, s):
    """w(s) = rho'(s) of an enabled edge, elementwise"""
    kind, p, s = np.broadcast_arrays(np.asarray(kind), np.asarray(p, dtype=np.float64), np.asarray(s, dtype=np.float64))
    p2 = p * p
    out = np.ones(s.shape)
    h = kind == HUBER
    with np.errstate(divide="ignore"):
        out[h] = np.where(s[h] <= p2[h], 1.0, p[h] / np.sqrt(s[h]))
    c = kind == CAUCHY
    out[c] = 1.0 / (1.0 + s[c] / p2[c])
    g = kind == GEMAN_MCCLURE
    out[g] = (p2[g] / (p2[g] + s[g])) ** 2
    return out


def settings(graph):
    """(kinds, params, enabled) of a graph, the defaults where it names none"""
    m = len(graph["edges"])
    return (np.asarray(graph.get("kinds", np.zeros(m, dtype=int))), np.asarray(graph.get("params", np.ones(m)), dtype=np.float64),
            np.asarray(graph.get("enabled", np.ones(m, dtype=bool)), dtype=bool))


def edge_terms(poses, graph):
    """(s, w) of every edge at `poses`: s = e^T L e (of a disabled edge too), w = rho'(s), 0 for a disabled edge"""
    kinds, params, enabled = settings(graph)
    e = ref.residuals(poses, graph["edges"], graph["means"])
    s = np.einsum("mi,mij,mj->m", e, graph["infos"], e)
    return s, np.where(enabled, weight(kinds, params, s), 0.0)


def cost(poses, graph):
    """F = sum rho over the enabled edges"""
    kinds, params, enabled = settings(graph)
    s, _ = edge_terms(poses, graph)
    return float(np.where(enabled, rho(kinds, params, s), 0.0).sum())


def chi2(poses, graph):
    """the plain sum of s over the enabled edges"""
    s, _ = edge_terms(poses, graph)
    return float(s[settings(graph)[2]].sum())


def linear_system(poses, graph):
    """H = sum w J^T L J as a (3N, 3N) CSR matrix and g = sum w J^T L e, node 0 included: posegraph_ref's system with every
    information matrix scaled by its edge's weight"""
    _, w = edge_terms(poses, graph)
    return ref.linear_system(poses, graph["edges"], graph["means"], w[:, None, None] * graph["infos"])


def optimize(graph, held=(), iters=100, lam=1e-4, history=None, decisions=None):
    """posegraph_hold_ref.optimize with F in place of chi2, rule for rule: keep the step if F falls, lambda halved or doubled,
    the gain stop, the 1e-18 stop, the lambda limit.  history takes F after every kept step; decisions takes (F before, F of the
    trial) of every step, kept or not.  Returns (poses, report dict) with F in chi2_initial and chi2_final."""
    edges = graph["edges"]
    poses = np.array(graph["poses"], dtype=np.float64)
    n = len(poses)
    cur = cost(poses, graph) if len(edges) else 0.0
    first = cur
    rep = dict(chi2_initial=cur, lm_steps=0, accepted=0, status=0)
    slot, node_of_slot = href.slots(n, held) if n else (np.zeros(0, dtype=int), np.zeros(1, dtype=int))
    free = node_of_slot[1:]
    if n < 2 or len(edges) == 0 or not (slot[edges] != 0).any():
        rep.update(chi2_final=cur, lambda_final=lam)
        return poses, rep
    idx = href._dofs(node_of_slot)
    only_node_0 = len(free) == n - 1
    system = None
    for _ in range(iters):
        if cur <= 1e-18 * first:
            rep["status"] = 2
            break
        if system is None:
            system = linear_system(poses, graph)
        h, g = system
        a = (h + lam * sp.diags(h.diagonal())).tocsc()
        a = a[3:, 3:] if only_node_0 else a[idx][:, idx]  # (the same matrix; the slice keeps posegraph_ref's bits)
        delta = np.zeros((n, 3))
        delta[free] = spla.spsolve(a.tocsc(), -g[idx]).reshape(-1, 3)
        trial = poses + delta
        trial[free, 2] = ref.wrap(trial[free, 2])
        new = cost(trial, graph)
        rep["lm_steps"] += 1
        if decisions is not None:
            decisions.append((cur, new))
        if new < cur:
            gain, before = cur - new, cur
            poses, cur, system = trial, new, None
            rep["accepted"] += 1
            lam = max(lam / 2.0, 1e-12)
            if history is not None:
                history.append(cur)
            if gain <= 1e-9 * before:
                rep["status"] = 1
                break
        else:
            lam *= 2.0
            if lam > 1e10:
                rep["status"] = 3
                break
    if rep["status"] == 0 and cur <= 1e-18 * first:
        rep["status"] = 2
    rep.update(chi2_final=cur, lambda_final=lam)
    return poses, rep


def with_settings(graph, huber_k=1.5, c=2.0):
    """`graph` with every third edge given a kind in rotation (huber, cauchy, geman_mcclure: edges 0, 3, 6, ...) and one edge in
    ten disabled (edges 5, 15, 25, ...; never edge 0, so the one-edge graph keeps its edge)"""
    m = len(graph["edges"])
    kinds, params = np.zeros(m, dtype=int), np.ones(m)
    for k, e in enumerate(range(0, m, 3)):
        kinds[e] = (HUBER, CAUCHY, GEMAN_MCCLURE)[k % 3]
        params[e] = huber_k if kinds[e] == HUBER else c
    enabled = np.ones(m, dtype=bool)
    enabled[5::10] = False
    return dict(graph, kinds=kinds, params=params, enabled=enabled)


def closures_of(graph, extra):
    """the indices of the `extra` long-range edges posegraph_ref.ring appends last"""
    m = len(graph["edges"])
    return np.arange(m - extra, m)


def with_wrong_closures(graph, extra, share, seed):
    """ring(..., extra=extra) with a share of its closures (at least one) replaced by constraints to a wrong place: the edge
    a -> b keeps its nodes and information and gets the noise-free mean of a -> b', b' a seeded node at least a quarter of the
    ring from b.  Returns (graph, closures, wrong): the indices of all closures and of the replaced ones."""
    rng = np.random.default_rng(seed)
    closures = closures_of(graph, extra)
    n = len(graph["poses"])
    count = max(1, int(round(share * extra)))
    wrong = np.sort(rng.choice(closures, size=count, replace=False))
    means = graph["means"].copy()
    for e in wrong:
        a, b = (int(v) for v in graph["edges"][e])
        while True:
            other = int(rng.integers(0, n))
            if min(abs(other - b), n - abs(other - b)) >= n // 4 and other != a:
                break
        means[e] = ref.relative(graph["truth"][a], graph["truth"][other])
    return dict(graph, means=means), closures, wrong


def robust_on(graph, edges, kind, p):
    """`graph` with the kind and parameter on `edges`, every other edge plain"""
    m = len(graph["edges"])
    kinds, params = np.zeros(m, dtype=int), np.ones(m)
    kinds[edges] = KIND_OF[kind]
    params[edges] = p
    return dict(graph, kinds=kinds, params=params)


def pose_error(poses, truth):
    """the largest |x|, |y| or wrapped |theta| difference"""
    d = np.array(poses) - np.array(truth)
    d[:, 2] = ref.wrap(d[:, 2])
    return float(np.abs(d).max())
