"""numpy yardstick of the map locator (include/yagmatch.h, ym_locator_*).

From the point set the search used, the caller's (cos, sin) table and the byte grid: the integer offsets, the exhaustive
score volume S[k][cy][cx] (shifted copies of the zero-padded map added up), the ordered top-K, the pyramid levels by direct
sliding maximum, and a plain branch and bound of the same contract (CPU tests only: it mirrors the chunking, the
threshold carried across chunks and the tie rule, and must return what the exhaustive evaluation returns)."""
import math

import numpy as np


def offsets(points, dir_cs, res):
    """int64 [n_angles][nq][2] = (dx, dy): r = (P.x c - P.y s, P.y c + P.x s), d = rint(r / res)"""
    p = np.asarray(points, dtype=np.float64).reshape(-1, 2)
    cs = np.asarray(dir_cs, dtype=np.float64).reshape(-1, 2)
    c, s = cs[:, 0][:, None], cs[:, 1][:, None]
    px, py = p[:, 0][None, :], p[:, 1][None, :]
    rx = px * c - py * s
    ry = py * c + px * s
    return np.stack([np.rint(rx / res), np.rint(ry / res)], axis=2).astype(np.int64)


def s_min_of(min_response, nq):
    return int(math.ceil(min_response * 100.0 * float(nq)))


def score_volume(g8, offs):
    """S[k][cy][cx] = sum_l g8[cy + dy_l][cx + dx_l], reads outside the map counting 0"""
    g = np.asarray(g8).astype(np.int64)
    H, W = g.shape
    S = np.zeros((offs.shape[0], H, W), dtype=np.int64)
    for k in range(offs.shape[0]):
        uniq, cnt = np.unique(offs[k], axis=0, return_counts=True)
        for (dx, dy), n in zip(uniq, cnt):
            x0, x1 = max(0, -dx), min(W, W - dx)
            y0, y1 = max(0, -dy), min(H, H - dy)
            if x0 < x1 and y0 < y1:
                S[k, y0:y1, x0:x1] += n * g[y0 + dy:y1 + dy, x0 + dx:x1 + dx]
    return S


def top_k(S, k, s_min=0):
    """[(score, index)] of the k best with score >= s_min: score descending, then index = (k H + cy) W + cx ascending"""
    flat = S.reshape(-1)
    idx = np.flatnonzero(flat >= s_min)
    order = np.lexsort((idx, -flat[idx]))[:k]
    return [(int(flat[idx[i]]), int(idx[i])) for i in order]


def pyramid_level(g8, j):
    """M_j with its low-side margin m = 2^j - 1: out[y + m][x + m] = max g8 over [x, x + 2^j) x [y, y + 2^j), 0 outside the map,
    for x in [-m, W), y in [-m, H)"""
    g = np.asarray(g8).astype(np.int64)
    H, W = g.shape
    m = (1 << j) - 1
    pad = np.zeros((H + 2 * m, W + 2 * m), dtype=np.int64)
    pad[m:m + H, m:m + W] = g
    out = np.zeros((H + m, W + m), dtype=np.int64)
    for dy in range(m + 1):
        for dx in range(m + 1):
            np.maximum(out, pad[dy:dy + H + m, dx:dx + W + m], out=out)
    return out


def node_bounds(level, j, offs_k, X, Y):
    """B of the nodes (X[i], Y[i]) of level j for one heading: sum_l M_j[Y + dy_l][X + dx_l] (0 outside what the level stores)"""
    m = (1 << j) - 1
    x = np.asarray(X)[:, None] + offs_k[None, :, 0] + m
    y = np.asarray(Y)[:, None] + offs_k[None, :, 1] + m
    ok = (x >= 0) & (x < level.shape[1]) & (y >= 0) & (y < level.shape[0])
    return np.where(ok, level[np.clip(y, 0, level.shape[0] - 1), np.clip(x, 0, level.shape[1] - 1)], 0).sum(axis=1)


def default_levels(W, H):
    L = 0
    while L < 6 and (4 << (L + 1)) <= min(W, H):
        L += 1
    return L


def branch_and_bound(g8, offs, k_top, s_min=0, levels=None, max_nodes=1 << 25):
    """The contract's search in plain numpy.  Returns ([(score, index)], stats) with stats = dict(chunks, nodes[9], survivors[9], probe_nodes)."""
    g = np.asarray(g8).astype(np.int64)
    H, W = g.shape
    L = default_levels(W, H) if levels is None else levels
    side = 1 << L
    pyr = [pyramid_level(g, j) for j in range(L + 1)]
    tops = [(k, Y, X) for k in range(offs.shape[0]) for Y in range(0, H, side) for X in range(0, W, side)]
    cells = [min(side, W - X) * min(side, H - Y) for (_, Y, X) in tops]
    assert max(cells) <= max_nodes, "one top-level node's expansion alone exceeds max_nodes"
    best = []  # (score, index), ordered
    stats = dict(chunks=0, nodes=[0] * 9, survivors=[0] * 9, probe_nodes=0)
    t0, tau = 0, -1
    while t0 < len(tops):
        t1, used = t0, 0
        while t1 < len(tops) and used + cells[t1] <= max_nodes:
            used += cells[t1]
            t1 += 1
        stats["chunks"] += 1
        front = tops[t0:t1]
        # the probe: a beam of the 64 best-bounded nodes followed down to level 0; the k_top-th best exact score it finds is a
        # threshold the final list cannot lie below (those k_top hypotheses exist), known before the exact pass starts
        probe = front if L > 0 else []
        for j in range(L, -1, -1):
            if not probe:
                break
            stats["probe_nodes"] += len(probe)
            B = np.zeros(len(probe), dtype=np.int64)
            for k in set(n[0] for n in probe):
                sel = [i for i, n in enumerate(probe) if n[0] == k]
                B[sel] = node_bounds(pyr[j], j, offs[k], [probe[i][2] for i in sel], [probe[i][1] for i in sel])
            order = np.lexsort((np.arange(len(probe)), -B))
            if j == 0:
                if len(probe) >= k_top:
                    tau = max(tau, int(B[order[k_top - 1]]))
                break
            h = 1 << (j - 1)
            probe = [(probe[i][0], probe[i][1] + dy, probe[i][2] + dx) for i in order[:64] for dy in (0, h) for dx in (0, h)
                     if probe[i][1] + dy < H and probe[i][2] + dx < W]
        if len(best) >= k_top:
            tau = max(tau, best[k_top - 1][0])
        thr = max(tau, s_min)
        for j in range(L, -1, -1):
            assert len(front) <= max_nodes
            stats["nodes"][j] += len(front)
            keep = []
            by_k = {}
            for (k, Y, X) in front:
                by_k.setdefault(k, []).append((Y, X))
            for k, yx in by_k.items():
                yx = np.array(yx)
                B = node_bounds(pyr[j], j, offs[k], yx[:, 1], yx[:, 0])
                keep += [(k, int(y), int(x), int(b)) for (y, x), b in zip(yx, B) if b >= thr]  # pruned only on strictly less
            stats["survivors"][j] += len(keep)
            if j == 0:
                best = sorted(best + [(b, (k * H + y) * W + x) for (k, y, x, b) in keep], key=lambda t: (-t[0], t[1]))[:k_top]
            else:
                h = 1 << (j - 1)
                front = [(k, y + dy, x + dx) for (k, y, x, _) in keep for dy in (0, h) for dx in (0, h) if y + dy < H and x + dx < W]
        t0 = t1
    return best, stats


# ---- the scenes the tests share ------------------------------------------------------------------------------------------
ROOM_RES = 0.1
ROOM_ORIGIN = (-0.75, -0.75)   # world position of cell (0, 0)
ROOM_SHAPE = (75, 95)          # H, W: the 8 m x 6 m room of synth.Scene() with 7.5 cells of margin
ROOM_TRUTH = (3.3, 2.7, 0.4)
ROOM_ANGLES = 36


def room_image(scene):
    """the walls and boxes of `scene` as an occupancy image at 0.1 m: 0 = occupied, 255 = free"""
    H, W = ROOM_SHAPE
    im = np.full((H, W), 255, dtype=np.uint8)
    for x0, y0, x1, y1 in scene.segs:
        n = int(math.hypot(x1 - x0, y1 - y0) / 0.02) + 2
        t = np.linspace(0.0, 1.0, n)
        cx = np.rint((x0 + t * (x1 - x0) - ROOM_ORIGIN[0]) / ROOM_RES).astype(int)
        cy = np.rint((y0 + t * (y1 - y0) - ROOM_ORIGIN[1]) / ROOM_RES).astype(int)
        im[cy, cx] = 0
    return im


def smear_grid(im, res, smear, occupied_value=0):
    """the float correlation grid of an occupancy image as ym_map_from_occupancy computes it: every occupied pixel is 1.0 and
    max-stamped with the matcher's float kernel (4 rint(smear / res) + 1 taps a side, exp(-0.5 d^2 / smear^2)), taps outside
    the image dropped.  For the CPU tests, where no device map can be read back."""
    half = (int(4 * np.rint(smear / res)) + 1) // 2
    H, W = im.shape
    out = np.zeros((H, W))
    occ = np.argwhere(im == occupied_value)
    for dy in range(-half, half + 1):
        for dx in range(-half, half + 1):
            v = math.exp(-0.5 * ((dx * res) ** 2 + (dy * res) ** 2) / (smear * smear))
            y, x = occ[:, 0] + dy, occ[:, 1] + dx
            ok = (y >= 0) & (y < H) & (x >= 0) & (x < W)
            np.maximum.at(out, (y[ok], x[ok]), v)
    out[occ[:, 0], occ[:, 1]] = 1.0
    return out


def byte_grid(cgrid):
    """what scoring reads: int(100 * cell)"""
    return (100 * np.asarray(cgrid, dtype=np.float64)).astype(np.int64)


def set_points(scans, stride=1):
    """The point set of a list of scans (objects with ranges, min_angle, angle_increment, range_threshold, corrected_pose): the
    readings the Python semantics keep (not NaN, not beyond range_threshold) at each scan's own pose, in scan then beam order,
    minus the mean scan position; every stride-th of them."""
    pts, xs, ys = [], [], []
    for q in scans:
        r = np.asarray(q.ranges, dtype=np.float64)
        p = q.corrected_pose
        ang = (p.euler[-1] + q.min_angle) + np.arange(r.shape[0]) * q.angle_increment
        ok = ~((r > q.range_threshold) | np.isnan(r))
        pts.append(np.stack([p.x + r * np.cos(ang), p.y + r * np.sin(ang)], axis=1)[ok])
        xs.append(float(p.x))
        ys.append(float(p.y))
    c = np.array([sum(xs) / float(len(xs)), sum(ys) / float(len(ys))])
    return (np.concatenate(pts) - c[None, :])[::stride]


def dir_table(n_angles):
    th = 2.0 * np.pi * np.arange(n_angles) / float(n_angles)
    return np.stack([np.cos(th), np.sin(th)], axis=1)


def random_grid(W=61, H=53, seed=5):
    """a float grid of random k / 100 values: pruning is weak on it"""
    return np.random.default_rng(seed).integers(0, 101, size=(H, W)) / 100.0


def corner_grid(W=45, H=38):
    """occupied cells only at the map's corners: the best hypotheses hang most of their points outside the map"""
    g = np.zeros((H, W))
    g[0, 0] = g[0, W - 1] = g[H - 1, 0] = g[H - 1, W - 1] = 1.0
    g[1, 0] = g[H - 1, W - 2] = 0.5
    return g


def room_labels(im, n_seeds=24, seed=21):
    """a label image of the room's free pixels: labels 0 and 1 .. K without gaps"""
    from yag_slam_amd.synth import seeded_partition
    lab = seeded_partition(im.shape[0], im.shape[1], n_seeds, seed) * (im == 255)
    _, inv = np.unique(lab, return_inverse=True)
    return inv.reshape(im.shape).astype(np.int32)


def decode(index, W, H):
    return index // (W * H), index % W, (index % (W * H)) // W  # k, cx, cy
