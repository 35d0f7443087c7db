"""numpy yardstick of the places search (include/yagmatch.h, ym_locator_locate_places).

`places` is the contract itself: the greedy rule on the exhaustive score volume of tests/locate_ref.py.  `branch_and_bound`
restates the device's search in plain numpy (CPU tests only): one round per place, each the branch and bound of
tests/locate_ref.py with top_k = 1, an empty threshold, and the exclusion rules -- a leaf near a pick never survives, a node
whose clipped square is wholly near one pick is dropped unscored, and the probe gives both the key score 0.  It must return
what `places` returns."""
import numpy as np

from tests import locate_ref as R


def near_mask(shape, pick, sep_cells2, sep_headings, circular):
    """bool [n_angles][H][W]: the hypotheses near the pick (k, cx, cy) -- BOTH within sep_cells2 and within sep_headings"""
    n_angles, H, W = shape
    k, cx, cy = pick
    dk = np.abs(np.arange(n_angles) - k)
    if circular:
        dk = np.minimum(dk, n_angles - dk)
    d2 = (np.arange(W)[None, :] - cx) ** 2 + (np.arange(H)[:, None] - cy) ** 2
    return (dk <= sep_headings)[:, None, None] & (d2 <= sep_cells2)[None, :, :]


def places(S, n_places, sep_cells2, sep_headings, circular, s_min=0):
    """[(score, index)] in place order: place 1 the best hypothesis with score >= s_min (ties by ascending index), place i + 1
    the best one near none of places 1 .. i; ends after n_places entries or when none is left"""
    n_angles, H, W = S.shape
    free = S >= s_min
    out = []
    while len(out) < n_places:
        best = R.top_k(np.where(free, S, -1), 1, max(s_min, 0))
        if not best:
            break
        out.append(best[0])
        free &= ~near_mask(S.shape, R.decode(best[0][1], W, H), sep_cells2, sep_headings, circular)
    return out


def greedy_over_top(S, top, n_places, sep_cells2, sep_headings, circular):
    """what thinning the `top` best does (MapLocator.locate(min_separation=...) with top = 64): the greedy rule on that list alone"""
    n_angles, H, W = S.shape
    kept = []
    for score, index in R.top_k(S, top):
        k, cx, cy = R.decode(index, W, H)
        if not any(near_mask(S.shape, R.decode(i, W, H), sep_cells2, sep_headings, circular)[k, cy, cx] for _, i in kept):
            kept.append((score, index))
    return kept[:n_places]


def _excluded(k, Y, X, side, W, H, picks, n_angles, sep_cells2, sep_headings, circular):
    """is the node's square, clipped to the map, wholly near one pick?  (side 1: the leaf test)"""
    x1, y1 = min(X + side, W) - 1, min(Y + side, H) - 1
    for pk, px, py in picks:
        dk = abs(k - pk)
        if circular:
            dk = min(dk, n_angles - dk)
        dx, dy = max(abs(X - px), abs(x1 - px)), max(abs(Y - py), abs(y1 - py))
        if dk <= sep_headings and dx * dx + dy * dy <= sep_cells2:
            return True
    return False


def _bounds(pyr, j, offs, nodes):
    """B of the nodes [(k, Y, X)] of level j"""
    B = np.zeros(len(nodes), dtype=np.int64)
    for k in set(n[0] for n in nodes):
        sel = [i for i, n in enumerate(nodes) if n[0] == k]
        B[sel] = R.node_bounds(pyr[j], j, offs[k], [nodes[i][2] for i in sel], [nodes[i][1] for i in sel])
    return B


def _round(g, pyr, offs, picks, sep, s_min, L, max_nodes, stats):
    """one search with top_k = 1 and `picks` excluded: (score, index) or None"""
    H, W = g.shape
    n_angles = offs.shape[0]
    side = 1 << L
    sep_cells2, sep_headings, circular = sep

    def excluded(n, j):
        return _excluded(n[0], n[1], n[2], 1 << j, W, H, picks, n_angles, sep_cells2, sep_headings, circular)

    tops = [(k, Y, X) for k in range(n_angles) for Y in range(0, H, side) for X in range(0, W, side)]
    cells = [min(side, W - X) * min(side, H - Y) for (_, Y, X) in tops]
    assert max(cells) <= max_nodes
    best, tau, t0, scored = None, -1, 0, 0
    while t0 < len(tops):
        t1, used = t0, 0
        while t1 < len(tops) and used + cells[t1] <= max_nodes:
            used += cells[t1]
            t1 += 1
        stats["chunks"] += 1
        front = tops[t0:t1]
        probe = front if L > 0 else []
        for j in range(L, -1, -1):
            if not probe:
                break
            stats["probe_nodes"] += len(probe)
            scored += len(probe)
            B = _bounds(pyr, j, offs, probe)
            B[[i for i, n in enumerate(probe) if excluded(n, j)]] = 0  # the probe's zeroed leaves and nodes
            order = np.lexsort((np.arange(len(probe)), -B))
            if j == 0:
                tau = max(tau, int(B[order[0]]))
                break
            h = 1 << (j - 1)
            probe = [(probe[i][0], probe[i][1] + dy, probe[i][2] + dx) for i in order[:64] for dy in (0, h) for dx in (0, h)
                     if probe[i][1] + dy < H and probe[i][2] + dx < W]
        if best is not None:
            tau = max(tau, best[0])
        thr = max(tau, s_min)
        for j in range(L, -1, -1):
            assert len(front) <= max_nodes
            stats["nodes"] += len(front)
            scored += len(front)
            out = [n for n in front if excluded(n, j)]
            stats["excluded_leaves" if j == 0 else "excluded_nodes"] += len(out)
            front = [n for n in front if not excluded(n, j)]
            B = _bounds(pyr, j, offs, front)
            keep = [(n, int(b)) for n, b in zip(front, B) if b >= thr]  # pruned only on strictly less
            if j == 0:
                for (k, y, x), b in keep:
                    cand = (b, (k * H + y) * W + x)
                    if best is None or (-cand[0], cand[1]) < (-best[0], best[1]):
                        best = cand
            else:
                h = 1 << (j - 1)
                front = [(k, y + dy, x + dx) for (k, y, x), _ in keep for dy in (0, h) for dx in (0, h) if y + dy < H and x + dx < W]
        t0 = t1
    stats["round_nodes"].append(scored)
    return best


def branch_and_bound(g8, offs, n_places, sep_cells2, sep_headings, circular, s_min=0, levels=None, max_nodes=1 << 25):
    """The places search as the device runs it.  Returns ([(score, index)], stats) with stats = dict(rounds, chunks, nodes,
    probe_nodes, excluded_leaves, excluded_nodes, round_nodes)."""
    g = np.asarray(g8).astype(np.int64)
    H, W = g.shape
    L = R.default_levels(W, H) if levels is None else levels
    pyr = [R.pyramid_level(g, j) for j in range(L + 1)]
    stats = dict(rounds=0, chunks=0, nodes=0, probe_nodes=0, excluded_leaves=0, excluded_nodes=0, round_nodes=[])
    found, picks = [], []
    while len(found) < n_places:
        stats["rounds"] += 1
        best = _round(g, pyr, offs, picks, (sep_cells2, sep_headings, circular), s_min, L, max_nodes, stats)
        if best is None:
            break
        found.append(best)
        picks.append(R.decode(best[1], W, H))
    return found, stats
