"""The finish stage of one match, restated in plain numpy / math (test infrastructure).

From a coarse response volume to the answer a caller sees, by Karto's rules as SURVEY.md (Appendix A, steps 7, 9, 10) and
the comments of ym_k_finish.hpp state them: best response, the DoubleEqual(1e-6) tie set and its mean (x and y arithmetic,
heading atan2 of the mean sine and cosine of the normalised headings), ComputePositionalCovariance over the per-(x, y)
maxima, and -- when refining -- the fine responses from the fine pass's integer sums, the fine best and tie mean, and
ComputeAngularCovariance at the fine-lattice cell under the mean.  Every sum is a math.fsum (exactly rounded, so the
reference's own rounding does not depend on an order), and every threshold comparison reports how far it was from its
threshold: a case whose smallest distance is tiny is one where the last bits of a correct implementation may decide
differently, and must not be compared.
"""
import math

import numpy as np

KT_TOLERANCE = 1e-6
MAX_VARIANCE = 500.0
PENALTY_GAIN = 0.2
OCCUPIED = 100
MIN_MARGIN = 1e-9


def kt_round(v):
    """math::Round: half away from zero"""
    return math.floor(v + 0.5) if v >= 0.0 else math.ceil(v - 0.5)


def normalize_angle(a):
    while a < -math.pi:
        a += 2 * math.pi
    while a > math.pi:
        a -= 2 * math.pi
    return a


def normalize_angle_difference(minuend, subtrahend):
    while minuend - subtrahend < -math.pi:
        minuend += 2 * math.pi
    while minuend - subtrahend > math.pi:
        minuend -= 2 * math.pi
    return minuend


def lattice(off, step, angle_off, angle_res):
    """Karto's search lattice: n = Round(2 off / step) + 1 values -off + i step per axis, Round(2 angle_off / angle_res) + 1 angles"""
    n = int(kt_round(off * 2.0 / step) + 1)
    return dict(nx=n, ny=n, nt=int(kt_round(angle_off * 2.0 / angle_res) + 1), off=off, step=step, angle_off=angle_off,
                angle_res=angle_res)


def lattices(cfg, coarse_angle_off=None):
    """(coarse, fine) lattices of a matcher configuration"""
    r = float(cfg["resolution"])
    side = int(kt_round(cfg["search_size"] / r) + 1)
    coarse = lattice(0.5 * (side - 1) * r, 2 * r, cfg["coarse_search_angle_offset"] if coarse_angle_off is None else coarse_angle_off,
                     cfg["coarse_angle_resolution"])
    fine = lattice(r, r, 0.5 * cfg["coarse_angle_resolution"], cfg["fine_search_angle_resolution"])
    return coarse, fine


def grid_offset(cfg, pose):
    """world coordinates of the correlation grid's cell (0, 0): the query's cell is the centre of the region of interest"""
    r = float(cfg["resolution"])
    side = int(kt_round(cfg["search_size"] / r) + 1)
    roi = side + 2 * int(math.ceil(cfg["range_threshold"] / r))
    return pose[0] - 0.5 * (roi - 1) * r, pose[1] - 0.5 * (roi - 1) * r


def penalties(cfg):
    return dict(dist_var=float(cfg["distance_variance_penalty"]), ang_var=float(cfg["angle_variance_penalty"]),
                min_dist=float(cfg.get("minimum_distance_penalty", 0.5)), min_ang=float(cfg["minimum_angle_penalty"]))


def responses(sums, nq, lat, centre_theta, penalize, pen):
    """CorrelateScan's response of every hypothesis from its integer sum: sum / (nq * 100), times the distance and the angle
    penalty when penalising and the response is not DoubleEqual to zero.  sums: [nt][ny][nx]."""
    s = np.asarray(sums, dtype=np.float64)
    r = s / float(nq * OCCUPIED) if nq else np.zeros_like(s)
    if penalize:
        x = -lat["off"] + np.arange(lat["nx"]) * lat["step"]
        y = -lat["off"] + np.arange(lat["ny"]) * lat["step"]
        sq = (x * x)[None, :] + (y * y)[:, None]
        dp = np.maximum(1.0 - (PENALTY_GAIN * sq / pen["dist_var"]), pen["min_dist"])
        angle = (centre_theta - lat["angle_off"]) + np.arange(lat["nt"]) * lat["angle_res"]
        ap = np.maximum(1.0 - (PENALTY_GAIN * ((angle - centre_theta) * (angle - centre_theta)) / pen["ang_var"]), pen["min_ang"])
        r = np.where(np.abs(r) <= KT_TOLERANCE, r, r * (dp[None, :, :] * ap[:, None, None]))
    return r


class _Margin:
    """smallest distance of any comparison from its threshold"""

    def __init__(self):
        self.value = math.inf

    def see(self, distances):
        d = np.abs(np.asarray(distances, dtype=np.float64))
        if d.size:
            self.value = min(self.value, float(d.min()))


def _tie_mean(resp, lat, centre, margin):
    """best response and the mean pose of the hypotheses DoubleEqual to it; centre = (x, y, heading) of the lattice"""
    best = float(resp.max())
    d = np.abs(resp - best)
    margin.see(np.abs(d - KT_TOLERANCE))
    kk, jj, ii = np.nonzero(d <= KT_TOLERANCE)
    n = len(kk)
    if n == 0:
        return best, None, 0
    xs = [centre[0] + (-lat["off"] + int(i) * lat["step"]) for i in ii]
    ys = [centre[1] + (-lat["off"] + int(j) * lat["step"]) for j in jj]
    start = centre[2] - lat["angle_off"]
    head = {int(k): normalize_angle(start + int(k) * lat["angle_res"]) for k in set(kk.tolist())}
    sines = math.fsum(math.sin(head[int(k)]) for k in kk)
    cosines = math.fsum(math.cos(head[int(k)]) for k in kk)
    return best, (math.fsum(xs) / n, math.fsum(ys) / n, math.atan2(sines / n, cosines / n)), n


def _positional_covariance(probs, lat, centre, mean, best, margin):
    cov = np.eye(3)
    if best < KT_TOLERANCE:
        cov[0, 0] = cov[1, 1] = MAX_VARIANCE
        cov[2, 2] = 4 * (lat["angle_res"] * lat["angle_res"])
        return cov
    dx, dy = mean[0] - centre[0], mean[1] - centre[1]
    p = np.asarray(probs, dtype=np.float64).reshape(lat["ny"], lat["nx"])
    margin.see(p - (best - 0.1))
    jj, ii = np.nonzero(p >= (best - 0.1))
    w = [float(p[j, i]) for j, i in zip(jj, ii)]
    x = [(-lat["off"] + int(i) * lat["step"]) - dx for i in ii]
    y = [(-lat["off"] + int(j) * lat["step"]) - dy for j in jj]
    norm = math.fsum(w)
    if norm > KT_TOLERANCE:
        vxx = math.fsum(a * a * c for a, c in zip(x, w)) / norm
        vxy = math.fsum(a * b * c for a, b, c in zip(x, y, w)) / norm
        vyy = math.fsum(b * b * c for b, c in zip(y, w)) / norm
        vxx = max(vxx, 0.1 * (lat["step"] * lat["step"]))
        vyy = max(vyy, 0.1 * (lat["step"] * lat["step"]))
        mult = 1.0 / best
        cov[0, 0], cov[0, 1], cov[1, 0], cov[1, 1] = vxx * mult, vxy * mult, vxy * mult, vyy * mult
        cov[2, 2] = 4 * (lat["angle_res"] * lat["angle_res"])
    if abs(cov[0, 0]) <= KT_TOLERANCE:
        cov[0, 0] = MAX_VARIANCE
    if abs(cov[1, 1]) <= KT_TOLERANCE:
        cov[1, 1] = MAX_VARIANCE
    return cov


def _cell(w, off, scale, margin):
    """WorldToGrid of one coordinate; the distance of the rounding from its half-way point goes to the margin"""
    v = (w - off) * scale
    margin.see(abs(v) + 0.5 - math.floor(abs(v) + 0.5))
    margin.see(math.floor(abs(v) + 0.5) + 1.0 - (abs(v) + 0.5))
    return int(kt_round(v))


def finish_ref(resp, lat, pose, probs=None, fine=None):
    """resp [nt][ny][nx]: the coarse responses; lat: lattice() of the coarse pass; pose: the query's (x, y, heading);
    probs [ny][nx]: the search-space probabilities (default: the maximum of resp over the angles).
    fine: None (no refinement) or a dict of
        sums [nt_f][ny_f][nx_f] the fine pass's integer sums, nq the number of query readings, lat the fine lattice(),
        penalize, pen = penalties(cfg), grid_off = grid_offset(cfg, pose), scale = 1 / resolution.
    Returns a dict: response, pose, cov [3][3], status, coarse_best, coarse_mean, n_ties, fine_n_ties, margin."""
    resp = np.asarray(resp, dtype=np.float64).reshape(lat["nt"], lat["ny"], lat["nx"])
    margin = _Margin()
    status = 0
    best, mean, n_ties = _tie_mean(resp, lat, pose, margin)
    if mean is None:
        mean, status = (0.0, 0.0, 0.0), -5
    probs = resp.max(axis=0) if probs is None else probs
    cov = _positional_covariance(probs, lat, pose, mean, best, margin)
    out = dict(coarse_best=best, coarse_mean=mean, n_ties=n_ties, fine_n_ties=0)
    if fine is not None:
        fl, nq = fine["lat"], int(fine["nq"])
        sums = np.asarray(fine["sums"]).reshape(fl["nt"], fl["ny"], fl["nx"])
        centre = mean
        fresp = responses(sums, nq, fl, centre[2], fine["penalize"], fine["pen"])
        best, fmean, fn = _tie_mean(fresp, fl, centre, margin)
        if fmean is None:
            status = -5
        else:
            mean = fmean
        out["fine_n_ties"] = fn
        # ComputeAngularCovariance: every fine angle's response at the cell of the mean pose
        best_angle = normalize_angle_difference(mean[2], centre[2])
        (ox, oy), scale = fine["grid_off"], fine["scale"]
        gx, gy = _cell(mean[0], ox, scale, margin), _cell(mean[1], oy, scale, margin)
        hit_x = hit_y = -1
        for i in range(fl["nx"]):
            if _cell(centre[0] + (-fl["off"] + i * fl["step"]), ox, scale, margin) == gx:
                hit_x = i
        for j in range(fl["ny"]):
            if _cell(centre[1] + (-fl["off"] + j * fl["step"]), oy, scale, margin) == gy:
                hit_y = j
        if hit_x < 0 or hit_y < 0:
            raise ValueError("the mean pose's cell is no cell of the fine lattice: not computable from the fine sums")
        start = centre[2] - fl["angle_off"]
        rs, terms = [], []
        for k in range(fl["nt"]):
            angle = start + k * fl["angle_res"]
            r = float(sums[k, hit_y, hit_x]) / float(nq * OCCUPIED)
            margin.see(r - (best - 0.1))
            if r >= (best - 0.1):
                rs.append(r)
                terms.append(((angle - best_angle) * (angle - best_angle)) * r)
        norm, acc = math.fsum(rs), math.fsum(terms)
        if norm > KT_TOLERANCE:
            if acc < KT_TOLERANCE:
                acc = fl["angle_res"] * fl["angle_res"]
            acc /= norm
        else:
            acc = 1000 * (fl["angle_res"] * fl["angle_res"])
        cov[2, 2] = acc
    out.update(response=min(best, 1.0), pose=tuple(mean), cov=cov, status=status, margin=margin.value)
    return out


def assert_margin(ref):
    """a case may be compared only if no comparison of the reference came closer than MIN_MARGIN to its threshold"""
    assert ref["margin"] >= MIN_MARGIN, "a comparison lies %.3g from its threshold: the case is ill-posed" % ref["margin"]
