"""Test-side yardstick of the pose-graph optimiser: numpy + scipy, written from Konolige et al., "Efficient Sparse Pose
Adjustment for 2D Mapping" (2010) and DESIGN.md ("Pose-graph optimiser").  Residuals, chi2, the sparse H and g, the
Levenberg-Marquardt loop with a sparse direct solve, and the graphs the tests run on.

A graph is a dict: poses (N, 3), edges (M, 2) int, means (M, 3), infos (M, 3, 3), and truth (N, 3) where there is one."""
import math

import numpy as np
import scipy.sparse as sp
import scipy.sparse.linalg as spla

TWO_PI = 2.0 * math.pi


def wrap(t):
    """into (-pi, pi]"""
    return t - TWO_PI * np.ceil((t - math.pi) / TWO_PI)


def residuals(poses, edges, means):
    """(M, 3): e_xy = R(theta_a)^T (t_b - t_a) - z_xy, e_theta = wrap(theta_b - theta_a - z_theta)"""
    pa, pb = poses[edges[:, 0]], poses[edges[:, 1]]
    c, s = np.cos(pa[:, 2]), np.sin(pa[:, 2])
    dx, dy = pb[:, 0] - pa[:, 0], pb[:, 1] - pa[:, 1]
    return np.stack([c * dx + s * dy - means[:, 0], -s * dx + c * dy - means[:, 1],
                     wrap(pb[:, 2] - pa[:, 2] - means[:, 2])], axis=1)


def chi2(poses, edges, means, infos):
    e = residuals(poses, edges, means)
    return float(np.einsum("mi,mij,mj->", e, infos, e))


def jacobians(poses, edges):
    """(M, 3, 3) each: d e / d pose_a, d e / d pose_b"""
    pa, pb = poses[edges[:, 0]], poses[edges[:, 1]]
    c, s = np.cos(pa[:, 2]), np.sin(pa[:, 2])
    dx, dy = pb[:, 0] - pa[:, 0], pb[:, 1] - pa[:, 1]
    z, o = np.zeros_like(c), np.ones_like(c)
    ja = np.stack([np.stack([-c, -s, -s * dx + c * dy], 1), np.stack([s, -c, -c * dx - s * dy], 1), np.stack([z, z, -o], 1)], 1)
    jb = np.stack([np.stack([c, s, z], 1), np.stack([-s, c, z], 1), np.stack([z, z, o], 1)], 1)
    return ja, jb


def linear_system(poses, edges, means, infos):
    """H = J^T L J as a (3N, 3N) CSR matrix and g = J^T L e, node 0 included"""
    n = len(poses)
    e = residuals(poses, edges, means)
    ja, jb = jacobians(poses, edges)
    a, b = edges[:, 0], edges[:, 1]
    blocks = [(a, a, np.einsum("mki,mkl,mlj->mij", ja, infos, ja)), (a, b, np.einsum("mki,mkl,mlj->mij", ja, infos, jb)),
              (b, a, np.einsum("mki,mkl,mlj->mij", jb, infos, ja)), (b, b, np.einsum("mki,mkl,mlj->mij", jb, infos, jb))]
    rows, cols, vals = [], [], []
    ii, jj = np.meshgrid(np.arange(3), np.arange(3), indexing="ij")
    for r, c, v in blocks:
        rows.append((3 * r[:, None, None] + ii[None]).ravel())
        cols.append((3 * c[:, None, None] + jj[None]).ravel())
        vals.append(v.ravel())
    h = sp.coo_matrix((np.concatenate(vals), (np.concatenate(rows), np.concatenate(cols))), shape=(3 * n, 3 * n)).tocsr()
    g = np.zeros((n, 3))
    np.add.at(g, a, np.einsum("mki,mkl,ml->mi", ja, infos, e))
    np.add.at(g, b, np.einsum("mki,mkl,ml->mi", jb, infos, e))
    return h, g.ravel()


def optimize(graph, iters=100, lam=1e-4, history=None):
    """The Levenberg-Marquardt loop of DESIGN.md with exact solves.  Returns (poses, report dict)."""
    edges, means, infos = graph["edges"], graph["means"], graph["infos"]
    poses = np.array(graph["poses"], dtype=np.float64)
    cur = chi2(poses, edges, means, infos)
    first = cur
    rep = dict(chi2_initial=cur, lm_steps=0, accepted=0, status=0)
    if len(poses) < 2 or len(edges) == 0:
        rep.update(chi2_final=cur, lambda_final=lam)
        return poses, rep
    system = None
    for _ in range(iters):
        if cur <= 1e-18 * first:
            rep["status"] = 2
            break
        if system is None:
            system = linear_system(poses, edges, means, infos)
        h, g = system
        a = (h + lam * sp.diags(h.diagonal())).tocsc()[3:, 3:]
        delta = np.concatenate([np.zeros(3), spla.spsolve(a, -g[3:])]).reshape(-1, 3)
        trial = poses + delta
        trial[:, 2] = wrap(trial[:, 2])
        new = chi2(trial, edges, means, infos)
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


def relative(pa, pb):
    """pose b in the frame of pose a, the angle wrapped: the noise-free mean of an edge a -> b"""
    c, s = math.cos(pa[2]), math.sin(pa[2])
    dx, dy = pb[0] - pa[0], pb[1] - pa[1]
    return np.array([c * dx + s * dy, -s * dx + c * dy, float(wrap(pb[2] - pa[2]))])


def compose(p, z):
    c, s = math.cos(p[2]), math.sin(p[2])
    return np.array([p[0] + c * z[0] - s * z[1], p[1] + s * z[0] + c * z[1], float(wrap(p[2] + z[2]))])


def _finish(truth, pairs, noise, rng, chain_drift=None, jitter=None):
    """means, informations and start poses for the edges `pairs` over the ground truth `truth`.  chain_drift: the start is
    dead-reckoned through the edges i -> i + 1 (which must be the first n - 1 of `pairs`, in order) with that drift a step;
    jitter: the start is the truth plus jitter * N(0, 1), node 0 exact"""
    n = len(truth)
    edges = np.array(pairs, dtype=np.int32)
    means = np.array([relative(truth[a], truth[b]) for a, b in pairs])
    means = means + noise * rng.standard_normal(means.shape) * np.array([1.0, 1.0, 0.3])
    m = rng.standard_normal((len(pairs), 3, 3))
    infos = 50.0 * np.einsum("mij,mkj->mik", m, m) + np.diag([400.0, 400.0, 900.0])
    if chain_drift is not None:
        poses = np.zeros((n, 3))
        poses[0] = truth[0]
        for i in range(n - 1):
            assert tuple(pairs[i]) == (i, i + 1)
            poses[i + 1] = compose(poses[i], means[i] + np.array(chain_drift))
    else:
        poses = np.array(truth) + np.array(jitter) * rng.standard_normal((n, 3))
        poses[0] = truth[0]
        poses[:, 2] = wrap(poses[:, 2])
    return dict(poses=poses, edges=edges, means=means, infos=infos, truth=np.array(truth))


def ring(n, noise=0.0, seed=0, extra=0):
    """n nodes on 0.97 of a circle of radius 10 m, heading tangential.  Edges i -> i+1, then i-3 -> i for i = 3, 5, 7, ...,
    then the closing edges 2 -> n-1 and 0 -> n-2, then `extra` seeded long-range edges."""
    rng = np.random.default_rng(seed)
    ang = 0.97 * TWO_PI * np.arange(n) / n
    truth = np.stack([10.0 * np.cos(ang), 10.0 * np.sin(ang), wrap(ang + math.pi / 2)], axis=1)
    pairs = [(i, i + 1) for i in range(n - 1)] + [(i - 3, i) for i in range(3, n, 2)] + [(2, n - 1), (0, n - 2)]
    have = set(pairs)
    while extra > 0:
        a, b = (int(v) for v in rng.integers(0, n, 2))
        if abs(a - b) > 20 and (a, b) not in have and (b, a) not in have:
            pairs.append((a, b))
            have.add((a, b))
            extra -= 1
    return _finish(truth, pairs, noise, rng, chain_drift=(0.002, 0.001, 0.004))


def grid(rows, cols, noise=0.0, seed=0, spacing=0.5):
    """rows x cols nodes, row-major, with 4-neighbour edges (along the rows first, then between them): the shape of a prior
    map's pose graph.  The start is the truth plus N(0, 1) * (0.05, 0.05, 0.02), as a map's own poses are close already."""
    rng = np.random.default_rng(seed)
    n = rows * cols
    truth = np.array([[spacing * (i % cols), spacing * (i // cols), 0.3 * math.sin(0.7 * i)] for i in range(n)])
    pairs = [(i, i + 1) for i in range(n - 1) if (i + 1) % cols] + [(i, i + cols) for i in range(n - cols)]
    return _finish(truth, pairs, noise, rng, jitter=(0.05, 0.05, 0.02))


def banded(n, reach, seed, far=2, reverse=0.4, noise=0.02):
    """n nodes on a gentle spiral whose system has block band `reach`: edges i -> i+1, every i -> i+reach, and a seeded half
    of the pairs at the distances in between; then `far` seeded edges longer than `reach` when n > reach + 2 (longer than 16,
    the widest band of the device, where n allows it, so that the automatic band stays `reach`), then one seeded edge a second
    time when n > 3.  A seeded share `reverse` of all edges is stored as (b, a), with the mean of the reversed pair; from
    three nodes on at least one in-band edge clear of node 0 is (node 0 is held, its off-diagonal blocks are not assembled),
    and the repeated edge is clear of node 0 too.  The start is the truth plus N(0, 1) * (0.05, 0.05, 0.02)."""
    rng = np.random.default_rng(seed)
    i = np.arange(n)
    rad, ang = 5.0 + 0.05 * i, 0.15 * i
    truth = np.stack([rad * np.cos(ang), rad * np.sin(ang), wrap(ang + math.pi / 2)], axis=1)
    pairs = [(a, a + 1) for a in range(n - 1)] + [(a, a + reach) for a in range(n - reach) if reach > 1]
    pairs += [(a, a + d) for d in range(2, reach) for a in range(n - d) if rng.random() < 0.5]
    in_band = len(pairs)
    if n > reach + 2:
        least = 17 if n > 18 + far else reach + 1
        have = set()
        while len(have) < far:
            a, b = sorted(int(v) for v in rng.integers(0, n, 2))
            if b - a >= max(least, reach + 1) and (a, b) not in have:
                have.add((a, b))
                pairs.append((a, b))
    if n > 3:
        clear = [p for p in pairs[:in_band] if p[0] != 0]
        pairs.append(clear[int(rng.integers(0, len(clear)))])
    flip = rng.random(len(pairs)) < reverse
    clear = [k for k in range(in_band) if pairs[k][0] != 0]
    if clear and not flip[clear].any():
        flip[clear[int(rng.integers(0, len(clear)))]] = True
    pairs = [(b, a) if f else (a, b) for (a, b), f in zip(pairs, flip)]
    return _finish(truth, pairs, noise, rng, jitter=(0.05, 0.05, 0.02))


def auto_band(graph, widest=16):
    """the band the device picks for band -1: the largest |a - b| among the edges that are at most `widest` apart"""
    d = np.abs(graph["edges"][:, 0].astype(int) - graph["edges"][:, 1])
    d = d[d <= widest]
    return int(d.max()) if len(d) else 0


def damped_system(graph, lam, band):
    """dense (A, M, b) of one step: A = H + lam diag(H) with node 0's rows and columns replaced by the identity, M the
    blocks of A with |i - j| <= band, b = -g with node 0's entries zero"""
    h, g = linear_system(graph["poses"], graph["edges"], graph["means"], graph["infos"])
    h = h.toarray()
    h = (h + h.T) / 2.0  # (the two off-diagonal blocks of an edge are rounded apart; the device keeps one and transposes it)
    a = h + lam * np.diag(np.diag(h))
    a[:3, :] = 0.0
    a[:, :3] = 0.0
    a[:3, :3] = np.eye(3)
    node = np.arange(len(a)) // 3
    m = np.where(np.abs(node[:, None] - node[None, :]) <= band, a, 0.0)
    b = -g
    b[:3] = 0.0
    return a, m, b


def pcg(A, M, b, tol, cap):
    """The device's recurrence (ym_k_posegraph.hpp, pg_solve_kernel) with a dense solve for M: (x, iterations, |r| / |b| of
    the recursively updated r)."""
    import scipy.linalg as sla
    x, r = np.zeros_like(b), b.copy()
    bb = float(b @ b)
    if not bb > 0.0:
        return x, 0, 0.0
    fac = sla.cho_factor(M)
    z = sla.cho_solve(fac, r)
    p = z.copy()
    rz, rr, iters = float(r @ z), bb, 0
    for _ in range(cap):
        q = A @ p
        alpha = rz / float(p @ q)
        x = x + alpha * p
        r = r - alpha * q
        rr = float(r @ r)
        iters += 1
        if rr <= tol * tol * bb:
            break
        z = sla.cho_solve(fac, r)
        rz_new = float(r @ z)
        p = z + (rz_new / rz) * p
        rz = rz_new
    return x, iters, math.sqrt(rr / bb)


def backward_error(M, z, b):
    """|M z - b|_inf / (|M|_inf |z|_inf + |b|_inf) in np.longdouble: the normwise backward error of z as a solution of M z = b"""
    M, z, b = (np.asarray(v, dtype=np.longdouble) for v in (M, np.ravel(z), np.ravel(b)))
    res = np.abs(M @ z - b).max()
    return float(res / (np.abs(M).sum(axis=1).max() * np.abs(z).max() + np.abs(b).max()))
