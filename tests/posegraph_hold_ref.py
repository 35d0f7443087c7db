"""Test-side yardstick of the pose-graph optimiser's held set ("Held nodes"): tests/posegraph_ref.py
with any set of nodes held.  Every node is held or free, node 0 always held.  Solve order: slot 0 stands for the held nodes
(identity row, right-hand side zero), the free nodes take the slots 1 .. F in index order; the band lives in slots.  H, g and
diag H are summed over all edges, so a free node keeps the diagonal block and gradient of its edges to held nodes, and an
edge between two held nodes only adds to chi2.  With held = {0} everything here is posegraph_ref's, to the bit."""
import math

import numpy as np
import scipy.sparse as sp
import scipy.sparse.linalg as spla

from tests import posegraph_ref as ref


def held_mask(n, held):
    """(n,) bool: the nodes of `held`, and node 0"""
    mask = np.zeros(n, dtype=bool)
    mask[np.asarray(sorted(set(int(v) for v in held) | {0}), dtype=int)] = True
    return mask


def slots(n, held):
    """(slot (n,), node_of_slot (F + 1,)): slot 0 for a held node, 1 .. F for the free ones in index order; node_of_slot[0] = 0"""
    mask = held_mask(n, held)
    free = np.flatnonzero(~mask)
    slot = np.zeros(n, dtype=int)
    slot[free] = 1 + np.arange(len(free))
    return slot, np.concatenate([[0], free]).astype(int)


def auto_band(graph, held, widest=16):
    """the band of band -1: the largest |slot(a) - slot(b)| <= widest among the edges whose ends are free or node 0, 0 without
    one.  An edge at node 0 has no block in the band; it counts because posegraph_ref.auto_band counts it, and with only node
    0 held the two must agree.  An edge at any other held node does not count."""
    slot, _ = slots(len(graph["poses"]), held)
    a, b = graph["edges"][:, 0].astype(int), graph["edges"][:, 1].astype(int)
    sa, sb = slot[a], slot[b]
    d = np.abs(sa - sb)[((sa != 0) | (a == 0)) & ((sb != 0) | (b == 0))]
    d = d[d <= widest]
    return int(d.max()) if len(d) else 0


def _dofs(node_of_slot):
    """the rows of the full system behind the slots 1 .. F"""
    return (3 * node_of_slot[1:, None] + np.arange(3)[None, :]).ravel()


def damped_system(graph, lam, band, held):
    """dense (A, M, b) of one step in solve order, 3 (F + 1) rows: A = H + lam diag(H) over the free nodes with the identity
    in slot 0, M the blocks of A with |slot - slot'| <= band, b = -g of the free nodes with slot 0's entries zero"""
    h, g = ref.linear_system(graph["poses"], graph["edges"], graph["means"], graph["infos"])
    h = h.toarray()
    h = (h + h.T) / 2.0  # (as posegraph_ref.damped_system: the device keeps one off-diagonal block an edge and transposes it)
    full = h + lam * np.diag(np.diag(h))
    _, node_of_slot = slots(len(graph["poses"]), held)
    idx = _dofs(node_of_slot)
    a = np.zeros((3 + len(idx), 3 + len(idx)))
    a[:3, :3] = np.eye(3)
    a[3:, 3:] = full[np.ix_(idx, idx)]
    s = np.arange(len(a)) // 3
    m = np.where(np.abs(s[:, None] - s[None, :]) <= band, a, 0.0)
    b = np.concatenate([np.zeros(3), -g[idx]])
    return a, m, b


def to_solve_order(rows, held):
    """(N, 3) by node -> (F + 1, 3) by slot (slot 0: zeros)"""
    _, node_of_slot = slots(len(rows), held)
    out = np.array(rows)[node_of_slot]
    out[0] = 0.0
    return out


def optimize(graph, held, iters=100, lam=1e-4, history=None):
    """posegraph_ref.optimize over the free nodes: the sparse direct solve of the reduced system, delta = 0 and no wrap for a
    held node.  No edge with a free end: zero steps.  Returns (poses, report dict)."""
    edges, means, infos = graph["edges"], graph["means"], graph["infos"]
    poses = np.array(graph["poses"], dtype=np.float64)
    n = len(poses)
    cur = ref.chi2(poses, edges, means, infos) if len(edges) else 0.0
    first = cur
    rep = dict(chi2_initial=cur, lm_steps=0, accepted=0, status=0)
    slot, node_of_slot = slots(n, held) if n else (np.zeros(0, dtype=int), np.zeros(1, dtype=int))
    free = node_of_slot[1:]
    if n < 2 or len(edges) == 0 or not (slot[edges] != 0).any():
        rep.update(chi2_final=cur, lambda_final=lam)
        return poses, rep
    idx = _dofs(node_of_slot)
    only_node_0 = len(free) == n - 1
    system = None
    for _ in range(iters):
        if cur <= 1e-18 * first:
            rep["status"] = 2
            break
        if system is None:
            system = ref.linear_system(poses, edges, means, infos)
        h, g = system
        a = (h + lam * sp.diags(h.diagonal())).tocsc()
        a = a[3:, 3:] if only_node_0 else a[idx][:, idx]  # (the same matrix; the slice keeps posegraph_ref's bits)
        delta = np.zeros((n, 3))
        delta[free] = spla.spsolve(a.tocsc(), -g[idx]).reshape(-1, 3)
        trial = poses + delta
        trial[free, 2] = ref.wrap(trial[free, 2])
        new = ref.chi2(trial, edges, means, infos)
        rep["lm_steps"] += 1
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


PRIOR_INFO = 1e12  # the information of a prior map's edges: splicing.map_to_graphslam links with covariance identity * 1e-12


def spliced(rows, cols, chain, seed=0, noise=0.02, links=3, stride=None):
    """A prior map with a robot's trajectory spliced in.  Nodes 0 .. rows cols - 1: posegraph_ref.grid(rows, cols), whose edges
    get the information PRIOR_INFO * identity and the means of the grid's own poses, so the prior is at rest as given.  Then
    `chain` robot nodes on a diagonal sweep over the grid with the ring's links (i -> i + 1, then i - 3 -> i for i = 3, 5,
    ...), dead-reckoned with drift from their first pose, and `links` links grid node -> chain node, evenly along the chain,
    each from the grid node nearest to the chain node's true position.  Returns the graph with `prior`, the grid's nodes."""
    rng = np.random.default_rng(seed)
    g = ref.grid(rows, cols, noise=0.0, seed=seed)
    n0, e0 = rows * cols, len(g["edges"])
    prior_means = np.array([ref.relative(g["poses"][a], g["poses"][b]) for a, b in g["edges"]])
    t = np.arange(chain) / max(chain - 1, 1)
    span_x, span_y = 0.5 * (cols - 1), 0.5 * (rows - 1)
    cx, cy = span_x * t, span_y * (0.5 - 0.5 * np.cos(math.pi * t))
    head = np.arctan2(np.gradient(cy), np.gradient(cx)) if chain > 1 else np.zeros(1)
    truth = np.stack([cx, cy, ref.wrap(head)], axis=1)
    pairs = [(i, i + 1) for i in range(chain - 1)] + [(i - 3, i) for i in range(3, chain, 2)]
    c = ref._finish(truth, pairs, noise, rng, chain_drift=(0.002, 0.001, 0.004)) if chain > 1 else None
    at = sorted(set(int(round(v)) for v in np.linspace(0, chain - 1, links)))
    lk_pairs, lk_means = [], []
    for i in at:
        near = int(np.argmin(np.hypot(g["truth"][:, 0] - truth[i, 0], g["truth"][:, 1] - truth[i, 1])))
        lk_pairs.append((near, n0 + i))
        lk_means.append(ref.relative(g["truth"][near], truth[i]) + noise * rng.standard_normal(3) * np.array([1.0, 1.0, 0.3]))
    m = rng.standard_normal((len(at), 3, 3))
    lk_infos = 50.0 * np.einsum("mij,mkj->mik", m, m) + np.diag([400.0, 400.0, 900.0])
    edges = np.concatenate([g["edges"], c["edges"] + n0, np.array(lk_pairs, dtype=np.int32)]).astype(np.int32)
    means = np.concatenate([prior_means, c["means"], np.array(lk_means)])
    infos = np.concatenate([np.tile(PRIOR_INFO * np.eye(3), (e0, 1, 1)), c["infos"], lk_infos])
    poses = np.concatenate([g["poses"], c["poses"]])
    return dict(poses=poses, edges=edges, means=means, infos=infos, truth=np.concatenate([g["truth"], truth]),
                prior=np.arange(n0))


def interleaved(free, gap, seed=0, noise=0.02):
    """`free` free nodes at the indices 6 + gap k with gap - 1 held nodes between consecutive ones, N = gap (free - 1) + 7
    nodes on posegraph_ref.banded's spiral.  Edges: 0 -> the first free node (6 apart: the only edge within 16 indices but
    longer than 1), each free node -> the next, the held node before each free node -> it, and one between two held nodes
    (1 -> 2).  By index the band would be 6; in slots it is 1 and no edge lies beyond it.  Returns the graph with `held`."""
    rng = np.random.default_rng(seed)
    n = gap * (free - 1) + 7
    i = np.arange(n)
    rad, ang = 5.0 + 0.05 * i, 0.15 * i
    truth = np.stack([rad * np.cos(ang), rad * np.sin(ang), ref.wrap(ang + math.pi / 2)], axis=1)
    at = [6 + gap * k for k in range(free)]
    pairs = [(0, at[0])] + [(a, b) for a, b in zip(at, at[1:])] + [(a - 1, a) for a in at] + [(1, 2)]
    g = ref._finish(truth, pairs, noise, rng, jitter=(0.05, 0.05, 0.02))
    g["held"] = np.array([v for v in range(n) if v not in at])
    return g
