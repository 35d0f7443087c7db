"""`match_scan_sets` restated in numpy from the statement of the call -- not imported from the reference and
not a copy of the device code: the filter walks its chain point by point, the grid is stamped point by point, every hypothesis'
cells are rounded on their own.  It returns what the fixtures of tests/golden/make_golden_scan_sets.py hold, plus the smallest
distance to a decision boundary it met: rounding ties (in cells) of the base readings and of every (hypothesis, point) pair of both
passes, and the two comparisons of the filter.  tests/test_scan_sets_host.py holds it against the fixtures the reference made;
tests/test_gpu_scan_sets.py holds the device against it on inputs no fixture has.
"""
import math

import numpy as np


def point_readings(ranges, pose, sensor):
    """every reading r <= the scan's threshold that is not NaN, at the scan's pose, in beam order"""
    r = np.asarray(ranges, dtype=np.float64)
    i = np.arange(len(r))
    with np.errstate(invalid="ignore"):
        ok = ~((r > sensor["range_threshold"]) | np.isnan(r))
    ang = pose[2] + sensor["min_angle"] + i[ok] * sensor["angle_increment"]
    return pose[0] + r[ok] * np.cos(ang), pose[1] + r[ok] * np.sin(ang)


def validate(px, py, vpx, vpy):
    """the valid-point filter: mask of the kept readings, and the smallest |d^2 - 0.04| and |ss| it decided on"""
    msd = 0.2 ** 2
    keep = np.zeros(len(px), dtype=bool)
    if len(px) == 0:
        return keep, math.inf, math.inf
    fx, fy = px[0], py[0]
    start = 1
    near_d, near_s = math.inf, math.inf
    for i in range(1, len(px)):
        cx, cy = px[i], py[i]
        d2 = (fx - cx) ** 2 + (fy - cy) ** 2
        near_d = min(near_d, abs(d2 - msd))
        if d2 > msd:
            a = vpy - fy
            b = fx - vpx
            c = fy * vpx - fx * vpy
            fx, fy = cx, cy
            ss = cx * a + cy * b + c
            near_s = min(near_s, abs(ss))
            if ss > 0.0:
                keep[start:i + 1] = True
            start = i + 1
    return keep, near_d, near_s


def smear_kernel(res, smear):
    size = int(4 * np.round(smear / res) + 1)
    half = int(size / 2)
    k = np.zeros((size, size))
    for i_ in range(size):
        for j_ in range(size):
            sq = ((i_ - half) * res) ** 2 + ((j_ - half) * res) ** 2
            k[i_, j_] = np.exp(-0.5 * sq / (smear ** 2))
    return k


def _tie(u):
    """distance of the values u to the nearest rounding tie, in cells"""
    if u.size == 0:
        return math.inf
    return float(np.min(np.abs(np.abs(u - np.floor(u)) - 0.5)))


def build_grid(cfg, G, ox, oy, base, view):
    """base: list of (ranges, pose, sensor).  Returns the float grid, the kept count per base scan and the tie distances."""
    res = cfg["resolution"]
    kern = smear_kernel(res, cfg["smear_deviation"])
    half = kern.shape[0] // 2
    grid = np.zeros((G, G))
    kept, tie, near_d, near_s = [], math.inf, math.inf, math.inf
    for ranges, pose, sensor in base:
        px, py = point_readings(ranges, pose, sensor)
        if len(px) == 0:  # (defined here: such a scan contributes nothing)
            kept.append(0)
            continue
        keep, nd, ns = validate(px, py, view[0], view[1])
        near_d, near_s = min(near_d, nd), min(near_s, ns)
        kept.append(int(keep.sum()))
        ux, uy = (px[keep] - ox) / res, (py[keep] - oy) / res
        tie = min(tie, _tie(ux), _tie(uy))
        gx, gy = np.round(ux).astype(np.int64), np.round(uy).astype(np.int64)
        for x, y in zip(gx, gy):
            if not (0 <= x < G and 0 <= y < G):
                continue
            x0, x1, y0, y1 = max(0, x - half), min(G, x + half + 1), max(0, y - half), min(G, y + half + 1)
            sub = kern[y0 - (y - half):y1 - (y - half), x0 - (x - half):x1 - (x - half)]
            grid[y0:y1, x0:x1] = np.maximum(grid[y0:y1, x0:x1], sub)
            grid[y, x] = 1.0
    return grid, kept, tie, near_d, near_s


def sums_pass(g8, G, ptsx, ptsy, cx, cy, ct, ox, oy, xy_s, xy_r, a_s, a_r, res):
    """the integer sums [nt][ny][nx] of one pass and its lattice, every (hypothesis, point) pair rounded on its own"""
    xv = np.arange(-xy_s + cx, xy_s + cx, xy_r)
    yv = np.arange(-xy_s + cy, xy_s + cy, xy_r)
    tv = np.arange(-a_s + ct, a_s + ct, a_r)
    out = np.zeros((len(tv), len(yv), len(xv)), dtype=np.int64)
    tie = math.inf
    for k, t in enumerate(tv):
        rx = ptsx * np.cos(t) - ptsy * np.sin(t)
        ry = ptsy * np.cos(t) + ptsx * np.sin(t)
        ux = ((xv[:, None] + rx[None, :]) - ox) / res      # [nx][points]
        uy = ((yv[:, None] + ry[None, :]) - oy) / res      # [ny][points]
        tie = min(tie, _tie(ux), _tie(uy))
        gx, gy = np.round(ux).astype(np.int64), np.round(uy).astype(np.int64)
        okx, oky = (gx >= 0) & (gx < G), (gy >= 0) & (gy < G)
        gxc, gyc = np.where(okx, gx, 0), np.where(oky, gy, 0)
        for iy in range(len(yv)):
            v = g8[gyc[iy][None, :], gxc]                  # [nx][points]
            v = np.where(okx & oky[iy][None, :], v, 0)
            out[k, iy, :] = v.sum(axis=1)
    return out, xv, yv, tv, tie


def best_pose(sums, xv, yv, tv, n_pts, cx, cy, ct, ox, oy, G, res, penalize):
    """find_best_pose's tuple from the integer sums: (response, x, y, t, xx, yy, xy, th)"""
    nx, ny, nt = len(xv), len(yv), len(tv)
    out = np.zeros((nx, ny, nt))
    sx_, sy_ = ox + G * res / 2, oy + G * res / 2
    for i in range(nx):
        for j in range(ny):
            for k in range(nt):
                pen = 1.0
                if penalize:
                    sd = (xv[i] - sx_) ** 2 + (yv[j] - sy_) ** 2
                    dp = 1.0 - 0.2 * sd / (0.5 * res)
                    sa = (tv[k] - ct) ** 2
                    ap = 1.0 - 0.2 * sa / (1.0 * res)
                    pen = dp * ap
                out[i, j, k] = float(sums[k, j, i]) / n_pts * pen / 100.0
    m = int(np.argmax(out))
    ii, jj, kk = m // (ny * nt), (m % (ny * nt)) // nt, (m % (ny * nt)) % nt
    response = out[ii, jj, kk]
    bx = by = bt = 0.0
    norm_ = 0.0
    for i, j, k in zip(*np.where(out >= response - 0.00000001)):
        bx += xv[i]
        by += yv[j]
        bt += tv[k]
        norm_ += 1.0
    bx, by, bt = bx / norm_, by / norm_, bt / norm_
    XX = YY = XY = TH = 0.0
    norm = 0.0
    for i in range(max(0, ii - 5), min(nx - 1, ii + 6)):
        for j in range(max(0, jj - 5), min(ny - 1, jj + 6)):
            r_ = out[i, j, kk]
            norm += r_
            XX += r_ * (xv[i] - bx) ** 2
            YY += r_ * (yv[j] - by) ** 2
            XY += (xv[i] - bx) * (yv[j] - by) * r_
    th_norm = 0.0
    for k in range(max(0, kk - 5), min(nt - 1, kk + 6)):
        r_ = out[ii, jj, k]
        th_norm += r_
        TH += r_ * (tv[k] - bt) ** 2
    with np.errstate(divide="ignore", invalid="ignore"):
        return [response, bx, by, bt, np.float64(XX) / norm / response, np.float64(YY) / norm / response,
                np.float64(XY) / norm / response, np.float64(TH) / th_norm]


def compose(a, b):
    """the planar pose a (+) b"""
    c, s = math.cos(a[2]), math.sin(a[2])
    return (a[0] + c * b[0] - s * b[1], a[1] + s * b[0] + c * b[1], a[2] + b[2])


def inverse(a):
    c, s = math.cos(a[2]), math.sin(a[2])
    return (-(c * a[0] + s * a[1]), -(-s * a[0] + c * a[1]), -a[2])


def match_scan_sets(cfg, queries, base, penalty=True, do_fine=True):
    """cfg: dict with resolution, smear_deviation, range_threshold, search_size, coarse_search_angle_offset,
    coarse_angle_resolution.  queries, base: lists of (ranges, pose, sensor).  Returns a dict."""
    res, search = cfg["resolution"], cfg["search_size"]
    G = int(search / res + 1 + 2 * cfg["range_threshold"] / res)
    xs = [float(q[1][0]) for q in queries]
    ys = [float(q[1][1]) for q in queries]
    cx, cy = sum(xs) / float(len(xs)), sum(ys) / float(len(ys))
    ox, oy = cx - 0.5 * (G - 1) * res, cy - 0.5 * (G - 1) * res
    view = (float(queries[-1][1][0]), float(queries[-1][1][1]))  # the LAST query scan's position
    grid, kept, tie_b, near_d, near_s = build_grid(cfg, G, ox, oy, base, view)
    g8 = (100 * grid).astype(np.int64)
    px, py = [], []
    for ranges, pose, sensor in queries:
        x, y = point_readings(ranges, pose, sensor)
        px.append(x)
        py.append(y)
    px, py = np.hstack(px), np.hstack(py)
    c0, s0 = np.cos(0), np.sin(0)
    lx, ly = (px * c0 - py * s0) + -cx, (py * c0 + px * s0) + -cy
    out = dict(G=G, centre=(cx, cy), origin=(ox, oy), view=view, kept=kept, grid=grid, g8=g8, pts=(lx, ly), n_points=len(lx))
    if len(lx) == 0:
        out["status"] = -1
        return out
    cs, cxv, cyv, ctv, tie_c = sums_pass(g8, G, lx, ly, cx, cy, 0.0, ox, oy, search * 0.5, res * 2,
                                         cfg["coarse_search_angle_offset"] * 0.5, cfg["coarse_angle_resolution"], res)
    coarse = best_pose(cs, cxv, cyv, ctv, len(lx), cx, cy, 0.0, ox, oy, G, res, penalty)
    fin, tie_f = coarse, math.inf
    out.update(coarse_sums=cs, coarse=coarse, coarse_dims=(len(cxv), len(cyv), len(ctv)))
    if do_fine:
        fs, fxv, fyv, ftv, tie_f = sums_pass(g8, G, lx, ly, coarse[1], coarse[2], coarse[3], ox, oy, res * 2, res, 0.0349 * 0.5,
                                             0.00349, res)
        fin = best_pose(fs, fxv, fyv, ftv, len(lx), coarse[1], coarse[2], coarse[3], ox, oy, G, res, penalty)
        th = fin[7]
        out.update(fine_sums=fs, fine_dims=(len(fxv), len(fyv), len(ftv)))
    else:
        th = 4 * cfg["coarse_angle_resolution"]
    cov = np.array([[coarse[4], coarse[6], 0], [coarse[6], coarse[5], 0], [0, 0, th]])
    corrected = (fin[1], fin[2], fin[3])
    diff = compose(inverse((cx, cy, 0.0)), corrected)
    out.update(status=0, final=fin, response=fin[0], covariance=cov, corrected_centre=corrected,
               poses=[compose(diff, tuple(float(v) for v in q[1])) for q in queries],
               tie=min(tie_b, tie_c, tie_f), near_d=near_d, near_s=near_s)
    return out
