"""The map segmenter of DESIGN.md ("Map segmenter") restated in numpy / scipy: what the device (include/yagmatch.h,
ym_map_free_space / ym_segments_from_map) is pinned against, integer for integer and label for label.  The rules are this
project's own (scikit-image's SLIC and OpenCV are not available to pin against); only the pre-processing, threshold plus
grey closing, is the reference's segment_map by definition.  Test side only: the package never imports this file."""
import math

import numpy as np
from scipy import ndimage

STAGE_FINAL, STAGE_ASSIGNED = 0, 1


def floorplan(h, w, seed):
    """the synthetic floor plan the segmenter's tests are defined on: rooms, walls with doors, speckle"""
    r = np.random.RandomState(seed); im = np.full((h, w), 200, np.uint8)
    im[10:h-10, 10:w-10] = 255; im[10:h-10, [10, w-11]] = 0; im[[10, h-11], 10:w-10] = 0
    for _ in range(8):
        if r.rand() < .5:
            y = r.randint(30, h-30); x0 = r.randint(10, w//2); x1 = x0 + r.randint(40, w//2)
            im[y:y+3, x0:x1] = 0; d = r.randint(x0, max(x0+1, x1-25)); im[y:y+3, d:d+22] = 255
        else:
            x = r.randint(30, w-30); y0 = r.randint(10, h//2); y1 = y0 + r.randint(40, h//2)
            im[y0:y1, x:x+3] = 0; d = r.randint(y0, max(y0+1, y1-25)); im[d:d+22, x:x+3] = 255
    sp = r.rand(h, w) < 0.002; im[sp & (im == 255)] = 200
    return im


def walled_square(n, value=255):
    """an n x n square of `value` inside a 1-pixel wall of zeros: (n + 2) x (n + 2)"""
    im = np.zeros((n + 2, n + 2), np.uint8)
    im[1:-1, 1:-1] = value
    return im


def spiral(n=170, corridor=14, wall=3):
    """a square spiral corridor, `corridor` pixels wide between walls of `wall` pixels: one long thin 4-connected region"""
    im = np.zeros((n, n), np.uint8)
    pitch = corridor + wall
    for i in range(n):
        a, b = wall + pitch * i, n - wall - pitch * i
        if b - a < corridor:
            break
        im[a:a + corridor, (a - pitch if i else a):b] = 255  # top, reaching back into the ring outside's left side
        im[a:b, b - corridor:b] = 255                         # right
        im[b - corridor:b, a:b] = 255                         # bottom
        im[a + pitch:b, a:a + corridor] = 255                 # left, one wall short of this ring's top
    return im


def free_space(image, close_size=11):
    """A: threshold and grey closing -> (closed uint8, sum, n_free).  Pixels outside the image take no part in a window."""
    a = np.array(image, dtype=np.uint8)
    a[a < 254] = 0
    t = 255 - a
    t = ndimage.maximum_filter(t, size=close_size, mode="constant", cval=0)
    t = ndimage.minimum_filter(t, size=close_size, mode="constant", cval=255)
    closed = (255 - t).astype(np.uint8)
    return closed, int(closed.sum(dtype=np.int64)), int(np.count_nonzero(closed))


def free_space_brute(image, close_size=11):
    """the same closing, window by window over the in-image part of each window"""
    a = np.array(image, dtype=np.uint8)
    a[a < 254] = 0
    t = 255 - a
    h, w = t.shape
    r = close_size // 2
    for op in (np.max, np.min):
        out = np.empty_like(t)
        for y in range(h):
            for x in range(w):
                out[y, x] = op(t[max(0, y - r):y + r + 1, max(0, x - r):x + r + 1])
        t = out
    return (255 - t).astype(np.uint8)


def segment(image, n_segments=0, density=1, close_size=11, iterations=10, min_size_div=4, stage=STAGE_FINAL):
    """A - D -> (labels int32 [h][w], info dict with the keys of ym_segment_info)"""
    closed, total, m = free_space(image, close_size)
    h, w = closed.shape
    if not n_segments:
        n_segments = int(total // 600000 * density)
    if n_segments < 1:
        raise ValueError("n_segments %d" % n_segments)
    if m == 0:
        raise ValueError("no free pixel")
    mask = closed != 0
    # B: seeds
    step = max(1, int(math.sqrt(m / n_segments) + 0.5))
    gw, gh = -(-w // step), -(-h // step)
    ys, xs = np.nonzero(mask)
    cell = (ys // step) * gw + xs // step
    count = np.bincount(cell, minlength=gw * gh).astype(np.int64)
    sum_x = np.zeros(gw * gh, np.int64); np.add.at(sum_x, cell, xs)
    sum_y = np.zeros(gw * gh, np.int64); np.add.at(sum_y, cell, ys)
    seeded = np.flatnonzero(4 * count >= step * step)
    k0 = len(seeded)
    if k0 == 0:
        raise ValueError("no seeded cell")
    cx, cy = sum_x[seeded] / count[seeded], sum_y[seeded] / count[seeded]
    table = np.full((gh + 4, gw + 4), -1, np.int64)  # cell -> centre, with a margin of two cells
    table.reshape(-1)[(seeded // gw + 2) * (gw + 4) + seeded % gw + 2] = np.arange(k0)
    # C: Lloyd
    pcx, pcy = xs // step, ys // step
    fx, fy = xs.astype(np.float64), ys.astype(np.float64)
    assign = np.zeros(len(xs), np.int64)  # centre + 1, 0 = none
    runs = 0
    for _ in range(iterations):
        best = np.full(len(xs), np.inf)
        new = np.zeros(len(xs), np.int64)
        for oy in range(5):  # raster order of cells = increasing centre index: a strict < keeps the lowest on a tie
            for ox in range(5):
                k = table[pcy + oy, pcx + ox]
                ok = k >= 0
                kk = np.where(ok, k, 0)
                dx, dy = fx - cx[kk], fy - cy[kk]
                d2 = np.where(ok, dx * dx + dy * dy, np.inf)
                better = d2 < best
                best = np.where(better, d2, best)
                new = np.where(better, k + 1, new)
        runs += 1
        changed = not np.array_equal(new, assign)
        assign = new
        n = np.bincount(assign, minlength=k0 + 1)[1:].astype(np.int64)
        sx = np.zeros(k0 + 1, np.int64); np.add.at(sx, assign, xs)
        sy = np.zeros(k0 + 1, np.int64); np.add.at(sy, assign, ys)
        has = n > 0
        cx, cy = cx.copy(), cy.copy()
        cx[has], cy[has] = sx[1:][has] / n[has], sy[1:][has] / n[has]
        if not changed:
            break
    assigned = np.zeros((h, w), np.int32)
    assigned[ys, xs] = assign
    min_size = (m // n_segments) // min_size_div
    info = dict(sum=total, n_free=m, n_segments=n_segments, step=step, seeds=k0, iterations_run=runs, min_size=min_size)
    if stage == STAGE_ASSIGNED:
        info.update(segments=0, unlabelled=int(m - np.count_nonzero(assigned)))
        return assigned, info
    # D: components
    comp = np.zeros((h, w), np.int64)
    n_comp = 0
    for k, box in enumerate(ndimage.find_objects(assigned)):
        if box is None:
            continue
        lab, n = ndimage.label(assigned[box] == k + 1)  # (the default structure: 4-connectivity)
        comp[box] += np.where(lab > 0, lab + n_comp, 0)
        n_comp += n
    flat = comp.reshape(-1)
    ids, first, sizes = np.unique(flat, return_index=True, return_counts=True)
    keep = (ids > 0) & (sizes >= min_size)
    order = np.argsort(first[keep], kind="stable")
    number = np.zeros(n_comp + 1, np.int32)
    number[ids[keep][order]] = np.arange(1, len(order) + 1)
    labels = number[comp]
    info.update(segments=len(order), unlabelled=int(m - np.count_nonzero(labels)), components=n_comp)
    return labels.astype(np.int32), info
