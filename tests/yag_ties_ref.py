"""The "yagpy" rounding rule restated in numpy, for the tests that attack the device's rounding proofs with aimed readings
(tests/test_yag_ties_host.py, tests/test_gpu_yag_ties.py).  Test infrastructure: a plain module.

The reference's Python matcher reads, for hypothesis (ix, iy, k) and point l,

    cell = (np.round(((xvals[ix] + r.x) - ox) / res), np.round(((yvals[iy] + r.y) - oy) / res)),   r = the point rotated by tvals[k],

tests the cell against the grid's bounds and adds int(100 * grid[cell]) (helpers.py:76-83, 134-153, 194-196 of the reference).  This
file is written from that statement, not from the kernels.  It starts from a *frame*: the axes, the (cos, sin) of every angle and the
point set one pass computed with -- on the device those come from ym_debug_yag_frame (ScanMatcher.debug_yag_frame), because the
device's cos, sin and points differ from libm's by up to an ulp; everything after them is IEEE add, subtract, multiply and divide, which
numpy's element-wise operations perform one rounding at a time exactly as the library's code does (it is built with -ffp-contract=off).

  (a) rule_sums        the integer sum volume of a pass, every (hypothesis, point) pair rounded on its own with a true division
  (b) lattice_facts    per (angle, point, axis): the distance of u(0) from a rounding tie, whether the cells form the lattice
                       c(0) + i * step along the axis, the guard of the lattice proof from its formula; expected_decision: what the
                       proof must decide for the item and how many pairs it must send to -- and lose in -- the exhaustive check
  (c) rint_div_facts   per (angle, point, position, axis) of a fine or map pass: do rint(d * fl(1 / res)) and rint(d / res) differ, and do
                       the two candidate cells hold different bytes
  (d) aim              new ranges that put chosen (point, angle, axis) pairs at chosen offsets from a rounding tie
"""
import numpy as np

E53 = 2.0 ** -53


def make_frame(xvals, yvals, tvals, trig, points, ox, oy, res, grid_w, grid_h, **more):
    """a frame from its parts (the host tests build theirs from numpy's trig; the GPU tests read the device's)"""
    f = dict(xvals=np.asarray(xvals, dtype=np.float64), yvals=np.asarray(yvals, dtype=np.float64), tvals=np.asarray(tvals, dtype=np.float64),
             trig=np.asarray(trig, dtype=np.float64).reshape(-1, 2), points=np.asarray(points, dtype=np.float64).reshape(-1, 2),
             ox=float(ox), oy=float(oy), res=float(res), grid_w=int(grid_w), grid_h=int(grid_h))
    f.update(nx=len(f["xvals"]), ny=len(f["yvals"]), nt=len(f["tvals"]), nq=len(f["points"]))
    f.update(more)
    return f


def rotated(frame):
    """helpers.py:76-78 _rotate_points with the frame's (cos, sin): rx, ry [nt][nq]"""
    c, s = frame["trig"][:, 0:1], frame["trig"][:, 1:2]
    px, py = frame["points"][None, :, 0], frame["points"][None, :, 1]
    return px * c - py * s, py * c + px * s


def axis_cells(vals, r, o, res):
    """np.round(((vals[i] + r) - o) / res) for every position i: [nt][n][nq] (float64, as the reference holds them)"""
    return np.round(((vals[None, :, None] + r[:, None, :]) - o) / res)


# ---------------------------------------------------------------------------------------------------------------- (a)
def rule_sums(frame, grid, origin=(0, 0)):
    """The sum volume [nt][ny][nx] (int64) of the rule as written.  `grid` [h][w] uint8 holds the cells x0 .. x0 + w, y0 .. y0 + h of the
    rule's grid_w x grid_h grid, origin = (x0, y0); cells of the grid outside `grid` are zero (the device window: DESIGN.md section 3)."""
    rx, ry = rotated(frame)
    cx = axis_cells(frame["xvals"], rx, frame["ox"], frame["res"])
    cy = axis_cells(frame["yvals"], ry, frame["oy"], frame["res"])
    g = np.asarray(grid)
    h, w = g.shape
    x0, y0 = origin
    # a zero border: every cell that counts for nothing -- outside the rule's grid, or inside it and outside `grid` -- reads it
    pad = np.zeros((h + 1, w + 1), dtype=np.int64)
    pad[:h, :w] = g

    def index(c, n_grid, o0, n_have):
        ci = np.where(np.isfinite(c), c, -1.0).astype(np.int64)  # int(gx): exact, the cells are integers
        ok = (ci >= 0) & (ci < n_grid) & (ci - o0 >= 0) & (ci - o0 < n_have)
        return np.where(ok, ci - o0, n_have)

    ix = index(cx, frame["grid_w"], x0, w)  # [nt][nx][nq]
    iy = index(cy, frame["grid_h"], y0, h)
    out = np.zeros((frame["nt"], frame["ny"], frame["nx"]), dtype=np.int64)
    for k in range(frame["nt"]):
        out[k] = pad[iy[k][:, None, :], ix[k][None, :, :]].sum(axis=-1)
    return out


# ---------------------------------------------------------------------------------------------------------------- (b)
def lattice_guard(frame):
    """The guard of the lattice proof from its formula (the comment above yag_lattice_kernel, ym_k_yagpy.hpp):
    guard = 8 (n + 8) e M / res + 2^-40 with e = 2^-53, n = max(nx, ny), M = |ox| + |oy| + 2 G res, G the matcher's grid side."""
    n = max(frame["nx"], frame["ny"])
    M = abs(frame["ox"]) + abs(frame["oy"]) + 2.0 * frame["roi_w"] * frame["res"]
    return 8.0 * (n + 8) * E53 * M / frame["res"] + 2.0 ** -40


def lattice_facts(frame, step_cells=None):
    """Per axis ("x", "y") a dict of [nt][nq] arrays: u0 = u(0), c0 = its cell, dist = |u0 - c0| (0.5 at a tie), tie = 0.5 - dist,
    regular = the cells of ALL positions form c0 + i * step_cells, fast = dist < 0.5 - guard (the proof accepts at once)."""
    step = frame["step_cells"] if step_cells is None else step_cells
    guard = lattice_guard(frame)
    rx, ry = rotated(frame)
    out = {"guard": guard}
    for name, vals, r, o in (("x", frame["xvals"], rx, frame["ox"]), ("y", frame["yvals"], ry, frame["oy"])):
        u = ((vals[None, :, None] + r[:, None, :]) - o) / frame["res"]
        c = np.round(u)
        want = c[:, 0:1, :] + (step * np.arange(len(vals), dtype=np.float64))[None, :, None]
        dist = np.abs(u[:, 0, :] - c[:, 0, :])
        out[name] = dict(u0=u[:, 0, :], c0=c[:, 0, :], dist=dist, tie=0.5 - dist, regular=np.all(c == want, axis=1),
                         fast=dist < 0.5 - guard)
    return out


def expected_decision(frame, facts=None):
    """What the lattice proof must decide for the frame's item (a chain call's coarse pass) and its exact counts:
    dict(regular, checked, failed) -- the item may take the production kernels' sums; (point, angle) pairs sent to the exhaustive
    check; pairs that lost it or that read outside the device window somewhere on the launch lattice.
    A pair inside the window is accepted at once when both axes are farther than the guard from a tie; otherwise it is checked
    position by position on the axes that are not, and fails if the lattice does not hold there.  An item is regular when no pair
    fails and its lattice fits the launch lattice.  (The proof's own claim -- an axis accepted at once IS regular -- is
    proof_claim_holds.)"""
    f = facts or lattice_facts(frame)
    fits = (0 < frame["nx"] <= frame["lat_nx"] and 0 < frame["ny"] <= frame["lat_ny"] and 0 < frame["nt"] <= frame["lat_nt"])
    if not fits:
        return dict(regular=False, checked=0, failed=0)
    w0, ww = frame["win_origin"], frame["win_w"]
    span_x, span_y = (frame["lat_nx"] - 1) * frame["step_cells"], (frame["lat_ny"] - 1) * frame["step_cells"]
    cx, cy = f["x"]["c0"], f["y"]["c0"]
    inside = (cx >= w0) & (cx + span_x < w0 + ww) & (cy >= w0) & (cy + span_y < w0 + ww)
    at_once = f["x"]["fast"] & f["y"]["fast"]
    checked = inside & ~at_once
    lost = checked & ~((f["x"]["fast"] | f["x"]["regular"]) & (f["y"]["fast"] | f["y"]["regular"]))
    failed = int(lost.sum()) + int((~inside).sum())
    return dict(regular=failed == 0, checked=int(checked.sum()), failed=failed)


def proof_claim_holds(facts):
    """the proof's claim: every (pair, axis) farther than the guard from a tie is regular along the whole axis"""
    return all(bool(np.all(facts[a]["regular"][facts[a]["fast"]])) for a in ("x", "y"))


def bands(facts, axis):
    """The three bands of the attack along `axis`, as boolean [nt][nq] arrays: inside the guard and regular (the exhaustive check
    accepts), inside the guard and irregular (the item falls back), outside the guard by less than the guard again (accepted at once)."""
    f, g = facts[axis], facts["guard"]
    inside = ~f["fast"]
    return dict(inside_regular=inside & f["regular"], inside_irregular=inside & ~f["regular"], just_outside=f["fast"] & (f["tie"] < 2.0 * g),
                beyond_2m40=inside & (f["tie"] > 2.0 ** -40))


# ---------------------------------------------------------------------------------------------------------------- (c)
def rint_div_facts(frame, grid=None, origin=(0, 0)):
    """Per axis a dict of [nt][n][nq] arrays for a pass whose cells go through yag_rint_div (the fine pass, every map and set pass):
    differ = rint(d * fl(1 / res)) != rint(d / res) for d = (vals[i] + r) - o; with `grid` also bytes_differ = the two candidate cells
    hold different bytes on at least one position of the other axis (so a hypothesis' sum depends on which one is read)."""
    res = frame["res"]
    rres = 1.0 / res
    rx, ry = rotated(frame)
    out = {}
    d, cq, cp = {}, {}, {}
    for name, vals, r, o in (("x", frame["xvals"], rx, frame["ox"]), ("y", frame["yvals"], ry, frame["oy"])):
        d[name] = (vals[None, :, None] + r[:, None, :]) - o
        cq[name] = np.round(d[name] / res)
        cp[name] = np.round(d[name] * rres)
        out[name] = dict(d=d[name], quotient=cq[name], product=cp[name], differ=cq[name] != cp[name])
    if grid is None:
        return out
    g = np.asarray(grid)
    h, w = g.shape
    x0, y0 = origin
    pad = np.zeros((h + 1, w + 1), dtype=np.int64)
    pad[:h, :w] = g

    def index(c, n_grid, o0, n_have):
        ci = c.astype(np.int64)
        ok = (ci >= 0) & (ci < n_grid) & (ci - o0 >= 0) & (ci - o0 < n_have)
        return np.where(ok, ci - o0, n_have)

    for name, other in (("x", "y"), ("y", "x")):
        bd = np.zeros(out[name]["differ"].shape, dtype=bool)
        for k, i, l in zip(*np.nonzero(out[name]["differ"])):
            if name == "x":
                a, b = index(cq["x"][k, i, l], frame["grid_w"], x0, w), index(cp["x"][k, i, l], frame["grid_w"], x0, w)
                rows = index(cq["y"][k, :, l], frame["grid_h"], y0, h)
                bd[k, i, l] = bool(np.any(pad[rows, a] != pad[rows, b]))
            else:
                a, b = index(cq["y"][k, i, l], frame["grid_h"], y0, h), index(cp["y"][k, i, l], frame["grid_h"], y0, h)
                cols = index(cq["x"][k, :, l], frame["grid_w"], x0, w)
                bd[k, i, l] = bool(np.any(pad[a, cols] != pad[b, cols]))
        out[name]["bytes_differ"] = bd
    return out


def differing_operands(tie_cell, res, reach=6):
    """the doubles d within `reach` ulps of the tie (tie_cell + 0.5) res for which rint(d * fl(1 / res)) != rint(d / res)"""
    centre = (tie_cell + 0.5) * res
    cand = [centre]
    lo = hi = centre
    for _ in range(reach):
        lo, hi = np.nextafter(lo, -np.inf), np.nextafter(hi, np.inf)
        cand += [lo, hi]
    cand = np.array(sorted(cand))
    return cand[np.round(cand * (1.0 / res)) != np.round(cand / res)]


# ---------------------------------------------------------------------------------------------------------------- (d)
def beam_lines(frame, ranges, base=None):
    """A point as a function of its beam's range: point = base + range * direction.  Chain calls: base 0 (sensor-frame points); map and
    set calls: base = the scan's position minus the set's centre.  The direction is taken from the frame's own points, so it is the
    device's (cos, sin) of the beam angle to an ulp."""
    pts = frame["points"]
    base = np.zeros_like(pts) if base is None else np.asarray(base, dtype=np.float64).reshape(-1, 2)
    rho = np.asarray(ranges, dtype=np.float64)
    return base, (pts - base) / rho[:, None]


def _axis_value(frame, axis, position, k, px, py):
    """d = (vals[position] + r) - o of the rule for points (px, py) at angle k along `axis`, the operations in the rule's order"""
    c, s = frame["trig"][k, 0], frame["trig"][k, 1]
    if axis == "x":
        return (frame["xvals"][position] + (px * c - py * s)) - frame["ox"]
    return (frame["yvals"][position] + (py * c + px * s)) - frame["oy"]


def aim(frame, ranges, targets, base=None, span=256):
    """New ranges for the beams the targets name.  A target is a dict(point, angle, axis ("x" / "y"), and
        either  offset: the signed distance in CELLS from a rounding tie that u = d / res shall have (tie_cell: which tie, default
                the one nearest to where the beam's point lies now; position: which position of the axis, default 0),
        or      d: the exact value (vals[position] + r) - o shall take).
    u is linear in the range with slope (direction . axis) / res: one Newton step from the frame's reading, two more on the simulated
    arithmetic, then the best of the +-`span` neighbouring doubles of the range.  Returns (new ranges, predicted u per target); what is
    achieved has to be read back from the next frame -- the device's beam direction is known here to an ulp, not exactly."""
    rho = np.array(ranges, dtype=np.float64)
    base_, dirs = beam_lines(frame, rho, base)
    res = frame["res"]
    predicted = []
    for t in targets:
        l, k, axis, pos = t["point"], t["angle"], t["axis"], t.get("position", 0)
        c, s = frame["trig"][k, 0], frame["trig"][k, 1]
        slope = (dirs[l, 0] * c - dirs[l, 1] * s) if axis == "x" else (dirs[l, 1] * c + dirs[l, 0] * s)
        value = lambda r_: _axis_value(frame, axis, pos, k, base_[l, 0] + r_ * dirs[l, 0], base_[l, 1] + r_ * dirs[l, 1])
        now = value(rho[l])
        if "d" in t:
            want_d, want_u = float(t["d"]), None
        else:
            tie = t.get("tie_cell")
            if tie is None:
                tie = np.round(now / res - 0.5)  # the tie nearest to where the point lies: between this cell number and the next
            want_u = (float(tie) + 0.5) + float(t["offset"])
            want_d = want_u * res
        r_new = rho[l]
        for _ in range(3):
            r_new = r_new + (want_d - value(r_new)) / slope
        cand = r_new + np.spacing(r_new) * np.arange(-span, span + 1)
        got = value(cand)
        err = np.abs(got - want_d) if want_u is None else np.abs(got / res - want_u)
        best = int(np.argmin(err))
        rho[l] = cand[best]
        predicted.append(float(got[best]) / res)
    return rho, np.array(predicted)


def u_grain(frame, axis, k, l):
    """the spacing, in cells, of the values u(0) of pair (angle k, point l) can take along `axis`: an ulp of u itself or, where that is
    more, an ulp of the world coordinate over the cell size (far from the origin that is hundreds of ulps of u)"""
    c, s = frame["trig"][k, 0], frame["trig"][k, 1]
    px, py = frame["points"][l]
    if axis == "x":
        x = frame["xvals"][0] + (px * c - py * s)
        d = x - frame["ox"]
    else:
        x = frame["yvals"][0] + (py * c + px * s)
        d = x - frame["oy"]
    return max(np.spacing(abs(d / frame["res"])), np.spacing(abs(x)) / frame["res"], np.spacing(abs(d)) / frame["res"])


# ------------------------------------------------------------------------------------------------- the attack's plans
# What both test files share: which beams are aimed where.  The plans choose, the restatement above judges what was achieved.
MIN_SLOPE = 0.35  # a beam is aimed along an axis only where a metre of range moves the point at least this far along it


def _slopes(frame, ranges, base, k):
    """d(point . axis)/d(range) of every beam at angle k: (along x, along y)"""
    _, dirs = beam_lines(frame, ranges, base)
    c, s = frame["trig"][k, 0], frame["trig"][k, 1]
    return dirs[:, 0] * c - dirs[:, 1] * s, dirs[:, 1] * c + dirs[:, 0] * s


def plan_lattice(frame, ranges, wanted, beams, seed, base=None):
    """Targets that fill the bands of the lattice attack on a chain call's coarse frame.  wanted: {(axis, band): pairs to aim}, band one
    of "inside_regular" (0.3 .. 0.7 guards from the tie), "just_outside" (1.2 .. 1.8 guards), "tie" (-1 .. 1 grains of u: where the
    irregular pairs live).  beams: the beams that may be moved; each is used once, at one angle, for the entry that lacks most."""
    rng = np.random.default_rng(seed)
    guard = lattice_guard(frame)
    left = dict(wanted)
    targets = []
    for n, l in enumerate(beams):
        if not any(left.values()):
            break
        k = n % frame["nt"]
        sx, sy = _slopes(frame, ranges, base, k)
        ok = {"x": abs(sx[l]) >= MIN_SLOPE, "y": abs(sy[l]) >= MIN_SLOPE}
        choice = [e for e in left if left[e] > 0 and ok[e[0]]]
        if not choice:
            continue
        axis, band = max(choice, key=lambda e: left[e])
        sign = 1.0 if rng.random() < 0.5 else -1.0
        if band == "inside_regular":
            off = sign * guard * rng.uniform(0.3, 0.7)
        elif band == "just_outside":
            off = sign * guard * rng.uniform(1.2, 1.8)
        else:
            off = float(rng.integers(-1, 2)) * u_grain(frame, axis, k, l)
        targets.append(dict(point=int(l), angle=int(k), axis=axis, offset=float(off), band=band))
        left[(axis, band)] -= 1
    return targets


def plan_rint_div(frame, ranges, beams, grid, origin=(0, 0), base=None, per_beam_ties=2, max_positions=None):
    """Targets that put (vals[i] + r) - o of a fine or map pass on doubles where rint(d * fl(1 / res)) and rint(d / res) differ and
    the two cells they name hold different bytes (the slopes of the smear, not its plateaus or the empty cells): for every beam the
    candidate -- over the angles, both axes, the positions and the ties next to where its point lies -- that moves the range least."""
    g = np.asarray(grid)
    h, w = g.shape
    x0, y0 = origin
    res = frame["res"]
    rho = np.asarray(ranges, dtype=np.float64)
    base_, dirs = beam_lines(frame, rho, base)
    cache = {}
    targets = []
    for l in beams:
        best = None
        for k in range(frame["nt"]):
            c, s = frame["trig"][k, 0], frame["trig"][k, 1]
            px, py = frame["points"][l]
            rx, ry = px * c - py * s, py * c + px * s
            slope = {"x": dirs[l, 0] * c - dirs[l, 1] * s, "y": dirs[l, 1] * c + dirs[l, 0] * s}
            for axis in ("x", "y"):
                if abs(slope[axis]) < MIN_SLOPE:
                    continue
                vals, r, o = (frame["xvals"], rx, frame["ox"]) if axis == "x" else (frame["yvals"], ry, frame["oy"])
                ovals, orr, oo = (frame["yvals"], ry, frame["oy"]) if axis == "x" else (frame["xvals"], rx, frame["ox"])
                others = np.round(((ovals + orr) - oo) / res).astype(np.int64)  # the cells of the other axis, every position
                for i in range(len(vals) if max_positions is None else min(len(vals), max_positions)):
                    d_now = (vals[i] + r) - o
                    n0 = np.round(d_now / res - 0.5)
                    for n in n0 + np.arange(per_beam_ties) * (1.0 if d_now / res >= n0 + 0.5 else -1.0):
                        key = (float(n))
                        if key not in cache:
                            cache[key] = differing_operands(n, res)
                        if not len(cache[key]):
                            continue
                        a = int(n)  # the two cells: a and a + 1
                        if axis == "x":
                            yy = others - y0
                            yy = yy[(yy >= 0) & (yy < h)]
                            slopey = 0 <= a - x0 and a + 1 - x0 < w and len(yy) and bool(np.any(g[yy, a - x0] != g[yy, a + 1 - x0]))
                        else:
                            xx = others - x0
                            xx = xx[(xx >= 0) & (xx < w)]
                            slopey = 0 <= a - y0 and a + 1 - y0 < h and len(xx) and bool(np.any(g[a - y0, xx] != g[a + 1 - y0, xx]))
                        if not slopey:
                            continue
                        d = cache[key][np.argmin(np.abs(cache[key] - d_now))]
                        move = abs((d - d_now) / slope[axis])
                        if best is None or move < best[0]:
                            best = (move, dict(point=int(l), angle=int(k), axis=axis, position=int(i), d=float(d)))
        if best is not None:
            targets.append(best[1])
    return targets


# ------------------------------------------------------------------------------------------------- the attacked problems
# A small room seen by a 360-beam sensor; three base scans and three queries at one prior pose: "regular" carries the pairs
# that must be accepted (by the exhaustive check, or at once just outside the guard); "irregular" the pairs aimed at the ties
# themselves, where many are genuinely irregular; "fine" the fine pass's attack.
# cells: the coarse search in cells (50: the default lattice, 26 x 26 launched; 80: the loop lattice, 41 x 41, the gather correlate's).
N_BEAMS = 360
MIN_ANGLE = -2.35619449
ANGLE_INCREMENT = 2.0 * 2.35619449 / (N_BEAMS - 1)
NEED = 20  # pairs a band must hold
CHAIN_CASES = {
    "res01_default_near": dict(res=0.01, cells=50, shift=(0.0, 0.0)),
    "res01_default_far_pm": dict(res=0.01, cells=50, shift=(9876.5, -10234.25)),
    "res05_loop_near": dict(res=0.05, cells=80, shift=(0.0, 0.0)),
    "res05_loop_far_mp": dict(res=0.05, cells=80, shift=(-10021.3, 9950.7)),
    "res005_default_near": dict(res=0.005, cells=50, shift=(0.0, 0.0)),
    "res005_loop_far_mm": dict(res=0.005, cells=80, shift=(-9990.1, -10007.9)),
    "res25_control": dict(res=0.25, cells=24, shift=(0.0, 0.0)),
}


def case_config(case):
    c = CHAIN_CASES[case] if isinstance(case, str) else case
    return dict(resolution=c["res"], search_size=c["cells"] * c["res"], smear_deviation=2 * c["res"], range_threshold=6.0)


def case_problem(case):
    """-> dict(base=[(ranges, pose)], queries={role: (ranges, pose)}): clean readings of a 4 m x 3 m room
    (yag_slam_amd.synth.Scene), every beam a point, the poses reported `shift` away from where the room is scanned"""
    from yag_slam_amd import synth
    c = CHAIN_CASES[case] if isinstance(case, str) else case
    sx, sy = c["shift"]
    scene = synth.Scene(width=4.0, height=3.0, n_boxes=3, seed=77)
    cast = lambda p, i: scene.scan_ranges(p, index=500 + i, sigma=0.004, n_beams=N_BEAMS, min_angle=MIN_ANGLE, inc=ANGLE_INCREMENT)
    there = lambda p: (p[0] + sx, p[1] + sy, p[2])
    base_poses = [(1.6, 1.4, 0.20), (1.7, 1.45, 0.25), (1.8, 1.5, 0.30)]
    prior = (1.9, 1.5, 0.33)
    truth = {"regular": (1.9 + 0.6 * c["res"] * 3, 1.5 - 0.4 * c["res"] * 3, 0.345), "irregular": (1.9 - 0.5 * c["res"] * 3, 1.5 + 0.7 * c["res"] * 3, 0.32),
             "fine": (1.9 + 0.3 * c["res"] * 3, 1.5 + 0.5 * c["res"] * 3, 0.338)}
    return dict(base=[(cast(p, i), there(p)) for i, p in enumerate(base_poses)],
                queries={n: (cast(t, 10 + j), there(prior)) for j, (n, t) in enumerate(sorted(truth.items()))})


def lattice_wanted(role, per_band=40, per_tie=175):
    if role == "regular":
        return {(a, b): per_band for a in ("x", "y") for b in ("inside_regular", "just_outside")}
    return {(a, "tie"): per_tie for a in ("x", "y")}


def lattice_beams(role, nq):
    """the regular query moves every other beam, the irregular one all of them"""
    return list(range(0, nq, 2)) if role == "regular" else list(range(nq))


def fine_beams(nq):
    """the fine query moves every other beam: the rest hold its coarse result, the fine pass's centre, in place"""
    return list(range(1, nq, 2))


def band_counts(frame0):
    """{(axis, band): pairs} of a coarse chain frame, with the facts they were counted on"""
    facts = lattice_facts(frame0)
    out = {}
    for axis in ("x", "y"):
        for name, mask in bands(facts, axis).items():
            out[(axis, name)] = int(mask.sum())
    return out, facts


def rint_div_count(frame, grid, origin=(0, 0)):
    """positions (angle, position, point, axis) of a pass where product and quotient round differently AND the cells differ"""
    f = rint_div_facts(frame, grid, origin)
    return sum(int((f[a]["differ"] & f[a]["bytes_differ"]).sum()) for a in ("x", "y")), sum(int(f[a]["differ"].sum()) for a in ("x", "y"))


def attack_chain_case(measure, problem, seed=0):
    """The rounds of one case.  measure(role, ranges) -> (coarse frame, fine frame, grid bytes, grid origin) runs the query `role` with
    these ranges (on the device, or on a simulated one) and reads back what it computed with.  Every query is measured once with its
    readings as they come and aimed from those frames: "regular" and "irregular" at the ties of the coarse pass, "fine" at the operands of
    the fine pass.  (A tie of the fine pass is a tie of the coarse pass too -- the fine lattice sits on a coarse position -- so the fine
    pass's attack has a query of its own: it makes its item irregular.)  No round is repeated: what the aimed readings achieve is for
    the caller to measure.  -> {role: ranges}"""
    out = {}
    for role in ("regular", "irregular", "fine"):
        ranges = np.array(problem["queries"][role][0], dtype=np.float64)
        f0, f1, grid, origin = measure(role, ranges)
        assert f0["nq"] == len(ranges), "every beam must be a point: the plans pair beams with points"
        if role == "fine":
            ranges, _ = aim(f1, ranges, plan_rint_div(f1, ranges, fine_beams(f1["nq"]), grid, origin))
        else:
            ranges, _ = aim(f0, ranges, plan_lattice(f0, ranges, lattice_wanted(role), lattice_beams(role, f0["nq"]), seed))
        out[role] = ranges
    return out


def rint_div_reachable(spec):
    """Can aimed readings put the operands of yag_rint_div where product and quotient round apart?  Not where the cell size has an exact
    reciprocal (a power of two: the two are one number).  And not kilometres from the origin: there d = (x + r) - o is a difference
    of coordinates whose ulp is 2^-39 m, a thousand ulps of d itself, so d moves on a grid a thousand times coarser than the few ulps
    around a tie where the two roundings part; no choice of ranges puts it there."""
    exact_reciprocal = np.frexp(spec["res"])[0] == 0.5
    return not exact_reciprocal and abs(spec["shift"][0]) < 1000 and abs(spec["shift"][1]) < 1000


# ------------------------------------------------------------------------------------------------- maps and scan sets
# yag_map_kernel rounds every cell of both passes through yag_rint_div.  A smaller room (2.4 m x 2 m: at 1 cm it fills a map of 280 x
# 240 cells); one query scan per set, so a point is (pose + range * direction) - pose and the plans' base is zero.
MAP_CASES = {
    "res01_near": dict(res=0.01, cells=50, shift=(0.0, 0.0), map_wh=(280, 240), margin=0.2),
    "res05_near": dict(res=0.05, cells=50, shift=(0.0, 0.0), map_wh=(200, 200), margin=1.7),
    "res01_far_pm": dict(res=0.01, cells=50, shift=(9876.5, -10234.25), map_wh=(280, 240), margin=0.2),
}  # margin: metres of map to the left of and below the room


def map_problem(case):
    """-> dict(base=[(ranges, pose)], queries=[(ranges, pose)] (two of them), room_corner=(x, y) of the map's cell (0, 0), to a cell)"""
    from yag_slam_amd import synth
    c = MAP_CASES[case] if isinstance(case, str) else case
    sx, sy = c["shift"]
    scene = synth.Scene(width=2.4, height=2.0, n_boxes=2, seed=78)
    cast = lambda p, i: scene.scan_ranges(p, index=700 + i, sigma=0.004, n_beams=N_BEAMS, min_angle=MIN_ANGLE, inc=ANGLE_INCREMENT)
    there = lambda p: (p[0] + sx, p[1] + sy, p[2])
    base_poses = [(1.1, 0.95, 0.20), (1.2, 1.0, 0.25), (1.3, 1.05, 0.30)]
    q_poses = [(1.25, 1.02, 0.27), (1.18, 0.97, 0.22)]
    truth = lambda p: (p[0] + 1.3 * c["res"], p[1] - 0.8 * c["res"], p[2] + 0.004)
    return dict(base=[(cast(p, i), there(p)) for i, p in enumerate(base_poses)],
                queries=[(cast(truth(p), 20 + i), there(p)) for i, p in enumerate(q_poses)],
                room_corner=(sx - c["margin"], sy - c["margin"]))


def map_search(case):
    """the coarse pass against the map: 40 positions of one cell of the matcher's own size per axis, ten angles"""
    c = MAP_CASES[case] if isinstance(case, str) else case
    return dict(xy_search=20 * c["res"], xy_step=c["res"], angle_search=0.05, angle_step=0.01, grid_resolution=c["res"])


def aim_coarse_pass(f0, ranges, grid, origin=(0, 0)):
    """first round of a map or set item: its even beams at the coarse pass's operands (the first six positions of an axis: enough, and
    the plan stays quick).  The coarse frame does not depend on the ranges, so these stay where they land."""
    return aim(f0, ranges, plan_rint_div(f0, ranges, list(range(0, f0["nq"], 2)), grid, origin, max_positions=6))[0]


def aim_fine_pass(f1, ranges, grid, origin=(0, 0)):
    """second round: the odd beams at the fine pass's operands, once the coarse pass has run on the readings of the first round (its
    result is the fine pass's centre; the moves of this round are a small fraction of a cell and leave it where it is)"""
    return aim(f1, ranges, plan_rint_div(f1, ranges, list(range(1, f1["nq"], 2)), grid, origin))[0]
