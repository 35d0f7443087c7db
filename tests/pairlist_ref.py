"""The region correlate's pair-list contract ("The pair-list contract") restated in plain numpy, float64.

bin_kernel (yag_slam_amd/csrc/ym_k_region.hpp) sorts the (reading, angle) pairs of a query into bins (region, angle) of 16-bit entries
= the LDS offset of the pair's patch once the region is staged.  This file says what those lists must hold, from the query's points
and angle table alone: the lookup cell of every pair, its region, bin and entry, the padded sizes, the four clauses that decide
whether a part's list "fits", the tight boxes; and the way back from an entry to its window cell.  Nothing here imports the package
or touches a device; tests/test_pairlist_host.py pins it to the oracle, tests/test_gpu_pair_lists.py compares the device with it.
"""
import math

import numpy as np

RG_W = 64               # class bytes a region owns along x
RG_PITCH = 100          # LDS bytes per staged class row
RG_FLUSH = 652          # patches per set of 16-bit sums
RG_MAX_REGIONS = 96     # regions with work a correlate block can list
RG_MAX_ENTRIES = 28672
RG_MAX_BINS = 8192
RG_LAST_POS = 65532     # positions in a query's entry array are 16-bit in the correlate
HEIGHTS = (80, 100, 128)  # class rows per region the library uses
CLAUSES = ("padded total > entries_pstride", "pos0 + total > 65532", "an angle's total > ng * 652", "regions with work > 96")


def kt_round_int(v):
    """(int)math::Round(v), half away from zero (ym_k_common.hpp, kt_round_int)"""
    v = np.asarray(v, dtype=np.float64)
    r = np.floor(np.abs(v) + 0.5).astype(np.int64)
    return np.where(v < 0.0, -r, r)


def rotate(ql, ctrig):
    """the rotated points [nt][nq] of GridIndexLookup::ComputeOffsets: ox = c x - s y, oy = s x + c y"""
    x, y = ql[None, :, 0], ql[None, :, 1]
    c, s = ctrig[:, None, 0], ctrig[:, None, 1]
    return c * x - s * y, s * x + c * y


def lookup_cells_karto(ql, ctrig, off_x, off_y, scale):
    """lookup_cell_sem, Karto: kt_round_int(((c x - s y) + off_x - off_x) * scale) -> [nt][nq][2] (x, y)"""
    ox, oy = rotate(np.asarray(ql, dtype=np.float64).reshape(-1, 2), np.asarray(ctrig, dtype=np.float64).reshape(-1, 2))
    gx = kt_round_int(((ox + off_x) - off_x) * scale)
    gy = kt_round_int(((oy + off_y) - off_y) * scale)
    return np.stack([gx, gy], axis=-1)


def lookup_cells_yagpy(ql, ctrig, off_x, off_y, ylat, res, origin):
    """lookup_cell_sem, "yagpy": rint(((ylat + (c x - s y)) - off) / res) - origin (half to even), the cell hypothesis (0, 0) reads"""
    ox, oy = rotate(np.asarray(ql, dtype=np.float64).reshape(-1, 2), np.asarray(ctrig, dtype=np.float64).reshape(-1, 2))
    gx = np.rint(((ylat[0] + ox) - off_x) / res).astype(np.int64) - origin
    gy = np.rint(((ylat[1] + oy) - off_y) / res).astype(np.int64) - origin
    return np.stack([gx, gy], axis=-1)


def encode(X, Y, rg_h, rg_cls, nrx, nry):
    """region_entry for window cells (X, Y): -> valid, region, entry, er, ex.  The division by the region height is a division."""
    X, Y = np.asarray(X, dtype=np.int64), np.asarray(Y, dtype=np.int64)
    xc, yc = X >> 1, Y >> 1
    cls = (X & 1) | ((Y & 1) << 1)
    rx, ry = xc // RG_W, yc // rg_h
    valid = (X >= 0) & (Y >= 0) & (yc < 4096) & (rx < nrx) & (ry < nry)
    er, ex = yc - ry * rg_h, xc - rx * RG_W
    return valid, ry * nrx + rx, cls * rg_cls + er * RG_PITCH + ex, er, ex


def decode(entry, region, rg_h, rg_cls, nrx):
    """a real entry of `region` back to its window cell (X, Y), with (er, ex)"""
    entry, region = np.asarray(entry, dtype=np.int64), np.asarray(region, dtype=np.int64)
    cls, rem = entry // rg_cls, entry % rg_cls
    er, ex = rem // RG_PITCH, rem % RG_PITCH
    ry, rx = region // nrx, region % nrx
    return 2 * (rx * RG_W + ex) + (cls & 1), 2 * (ry * rg_h + er) + (cls >> 1), er, ex


def split_bin(e, rg_zero):
    """One bin's entries -> (its real entries, None) or (None, what is wrong).  A bin is four runs in misalignment order 0, 1, 2, 3,
    each its real entries (entry & 3 == r, below rg_zero) followed by ONE rg_zero + r exactly when their number is odd; then one pair
    of rg_zero exactly when the four runs together are no multiple of four."""
    e = np.asarray(e, dtype=np.int64)
    if len(e) % 4:
        return None, "bin length %d is no multiple of four" % len(e)
    pos, real = 0, []
    for r in range(4):
        first = pos
        while pos < len(e) and e[pos] < rg_zero and (e[pos] & 3) == r:
            pos += 1
        real.append(e[first:pos])
        if (pos - first) & 1:
            if pos >= len(e) or e[pos] != rg_zero + r:
                return None, "run %d has %d entries and no padding entry rg_zero + %d behind them" % (r, pos - first, r)
            pos += 1
    rest = e[pos:]
    if (pos & 3) == 0 and len(rest) == 0:
        return np.concatenate(real), None
    if (pos & 3) == 2 and len(rest) == 2 and rest[0] == rg_zero and rest[1] == rg_zero:
        return np.concatenate(real), None
    return None, "after the four runs (%d entries) the bin goes on with %s" % (pos, rest[:6].tolist())


def plan_geometry(cfg, rq, max_n, nx, ny, nt, n_items=8, semantics="karto", rg_h=80):
    """What the host plans for a batch of `n_items` whose longest scan has max_n readings and whose queries reach rq metres
    (ym_host_plan.hpp, plan_sizes; a fresh matcher, Karto semantics, no query reading beyond the matcher's threshold)."""
    assert semantics == "karto"
    res = 1.0 / (1.0 / cfg["resolution"])
    side = int(kt_round_int(cfg["search_size"] / cfg["resolution"])) + 1
    roi_w = side + 2 * int(math.ceil(cfg["range_threshold"] / cfg["resolution"]))
    border = int(kt_round_int(2.0 * cfg["smear_deviation"] / cfg["resolution"])) + 1
    storage_w = roi_w + 2 * border
    centre = border + (roi_w - 1) // 2
    coarse_off = 0.5 * (side - 1) * res
    wh = (int(math.ceil((rq + coarse_off + res) / res)) + 3 + 63) // 64 * 64
    wh = min(wh, centre)
    origin = centre - wh
    win_w = min(2 * wh + 1, storage_w - origin)
    half_w = (win_w + 1) // 2
    lnw = nt if nt <= 8 else 8
    lparts = (nt + lnw - 1) // lnw
    nrx, nry = (half_w + RG_W - 1) // RG_W, (half_w + rg_h - 1) // rg_h
    ng = ((max_n * 23 + 19) // 20 + RG_FLUSH - 1) // RG_FLUSH
    g = dict(nt=nt, lnw=lnw, lparts=lparts, nrx=nrx, nry=nry, nregions=nrx * nry, nbins=nrx * nry * lnw, rg_h=rg_h,
             rg_cls=RG_PITCH * (rg_h + 26), rg_zero=4 * RG_PITCH * (rg_h + 26), ng=ng,
             entries_pstride=min(RG_MAX_ENTRIES, (lnw * max_n * 11 // 10 + 63) // 64 * 64),
             win_w=win_w, origin=origin, border=border, half_w=half_w)
    g["region26"] = bool(n_items >= 8 and nx <= 26 and ny <= 32 and ng <= 8 and nt * max_n <= RG_MAX_ENTRIES and
                         nrx * nry * nt < RG_MAX_BINS and max_n < 2048 and half_w <= 4096)
    return g


def predict(cells, cx0, cy0, g):
    """Everything the lists of one query slot must hold.  cells: [nt][nq][2] lookup cells; g: the geometry (the ABI's, or
    plan_geometry's).  -> dict: per part `bins` {bin: sorted real entries}, `total` (padded), `angle_tot`, `regions_used`, `refused`
    (the clauses that refuse the part, indices into CLAUSES), `flag`; `box` [nregions][lparts][4] tight boxes (255, 0, 255, 0: empty);
    `lost`: pairs whose patch origin lies outside the regions (the lists then cannot be complete)."""
    nt, lnw, lparts, nbins = g["nt"], g["lnw"], g["lparts"], g["nbins"]
    cells = np.asarray(cells, dtype=np.int64).reshape(nt, -1, 2)
    valid, region, entry, er, ex = encode(cx0 + cells[..., 0], cy0 + cells[..., 1], g["rg_h"], g["rg_cls"], g["nrx"], g["nry"])
    box = np.tile(np.array([255, 0, 255, 0], dtype=np.int32), (g["nregions"], lparts, 1))
    parts = []
    for p in range(lparts):
        ks = range(p * lnw, min(nt, (p + 1) * lnw))
        bins, angle_tot, used, total = {}, np.zeros(lnw, dtype=np.int64), set(), 0
        for k in ks:
            v = valid[k]
            b = region[k][v] * lnw + (k - p * lnw)
            for bn in np.unique(b):
                sel = b == bn
                e = np.sort(entry[k][v][sel])
                runs = np.bincount(e & 3, minlength=4)
                padded = (int(((runs + 1) & ~1).sum()) + 3) & ~3
                bins[int(bn)] = e
                angle_tot[k - p * lnw] += padded
                total += padded
                R = int(bn) // lnw
                used.add(R)
                r_, x_ = er[k][v][sel], ex[k][v][sel]
                bx = box[R, p]
                bx[0], bx[1], bx[2], bx[3] = min(bx[0], r_.min()), max(bx[1], r_.max()), min(bx[2], x_.min()), max(bx[3], x_.max())
        refused = []
        if total > g["entries_pstride"]:
            refused.append(0)
        if p * g["entries_pstride"] + total > RG_LAST_POS:
            refused.append(1)
        if (angle_tot > g["ng"] * RG_FLUSH).any():
            refused.append(2)
        if len(used) > RG_MAX_REGIONS:
            refused.append(3)
        parts.append(dict(bins=bins, total=total, angle_tot=angle_tot, regions_used=len(used), refused=refused,
                          flag=-1 if refused else total, pairs=int(sum(valid[k].sum() for k in ks))))
    assert nbins == g["nregions"] * lnw
    return dict(parts=parts, box=box, lost=int((~valid).sum()))
