// ym_occlive_window.hpp -- the live occupancy grid's window and growth arithmetic, on the host, in
// integers and fp64.  Needs neither HIP nor the rest of the library: ym_abi_occlive.hpp uses it, and so does the stand-alone
// program tests/native/occlive_window_check.cpp, which runs it under the address and undefined-behaviour sanitizers.
//
// Everything is in cells of the ANCHOR's lattice: cell c covers the world coordinates p with Round((p - anchor) * scale) == c.
//   window   the part of the lattice that is reported: per axis origin = Round((min - anchor) * scale), size =
//            Round((max - min) * scale) of the running bounding box (OccupancyGrid::ComputeDimensions in the anchor's frame)
//   reach    every cell a ray of a scan ever added can touch (the sensor's cell and every traced end point's, so also the ends of
//            the rays clipped at the range threshold, which the bounding box does not hold)
//   alloc    the rectangle that has memory: it always holds window and reach, so no count is ever dropped for lying outside
//            today's window, and a window that grows later finds the counts of earlier rays in place
#pragma once
#include <cmath>
#include <cstdint>

namespace ymw {

constexpr int64_t kLatticeLimit = (int64_t)1 << 30; // |cell| below this: cells, sizes and their differences fit an int32
constexpr int64_t kCellCap = 2000000000;            // cells of a window or an allocation (the full renderer's cap)

struct Rect { // x0, y0: lowest cell; empty when w <= 0 or h <= 0
    int64_t x0 = 0, y0 = 0, w = 0, h = 0;
    bool empty() const { return w <= 0 || h <= 0; }
    int64_t cells() const { return empty() ? 0 : w * h; }
};

inline double round_half_away(double v) { return v >= 0.0 ? std::floor(v + 0.5) : std::ceil(v - 0.5); }

inline bool contains(const Rect &outer, const Rect &inner) {
    if (inner.empty()) return true;
    if (outer.empty()) return false;
    return inner.x0 >= outer.x0 && inner.y0 >= outer.y0 && inner.x0 + inner.w <= outer.x0 + outer.w && inner.y0 + inner.h <= outer.y0 + outer.h;
}

inline Rect join(const Rect &a, const Rect &b) {
    if (a.empty()) return b.empty() ? Rect() : b;
    if (b.empty()) return a;
    Rect r;
    r.x0 = a.x0 < b.x0 ? a.x0 : b.x0;
    r.y0 = a.y0 < b.y0 ? a.y0 : b.y0;
    const int64_t x1 = a.x0 + a.w > b.x0 + b.w ? a.x0 + a.w : b.x0 + b.w, y1 = a.y0 + a.h > b.y0 + b.h ? a.y0 + a.h : b.y0 + b.h;
    r.w = x1 - r.x0;
    r.h = y1 - r.y0;
    return r;
}

inline bool in_lattice(const Rect &r) {
    return r.empty() || (r.x0 > -kLatticeLimit && r.y0 > -kLatticeLimit && r.x0 + r.w < kLatticeLimit && r.y0 + r.h < kLatticeLimit);
}

// The window of a bounding box (xmin, ymin, xmax, ymax).  A size may come out 0 (a box without width): such a window is empty and
// cannot be read, but scans can be added to it.  false: a coordinate is not finite or leaves the lattice.
inline bool window_of_box(const double box[4], const double anchor[2], double scale, Rect *out) {
    const double v[4] = {round_half_away((box[0] - anchor[0]) * scale), round_half_away((box[1] - anchor[1]) * scale),
                         round_half_away((box[2] - box[0]) * scale), round_half_away((box[3] - box[1]) * scale)};
    for (double d : v)
        if (!(std::fabs(d) < (double)kLatticeLimit)) return false; // (NaN fails the comparison)
    out->x0 = (int64_t)v[0]; out->y0 = (int64_t)v[1]; out->w = (int64_t)v[2]; out->h = (int64_t)v[3];
    if (out->w < 0) out->w = 0;
    if (out->h < 0) out->h = 0;
    return out->x0 + out->w < kLatticeLimit && out->y0 + out->h < kLatticeLimit;
}

// What an add has to do to the memory.  `need` (window joined with reach) must lie inside the allocation afterwards.
struct Growth {
    bool grow = false; // false: the allocation holds `need` already, nothing else is set
    Rect alloc;        // the new allocation; rows are alloc.w cells apart
    // the old allocation's cells move as ONE rectangle of copy_w x copy_h cells: from row 0 / column 0 of the old buffer (rows
    // old.w apart) to row dst_y / column dst_x of the new one.  copy_w == 0: nothing to move (the first allocation).
    int64_t copy_w = 0, copy_h = 0, dst_x = 0, dst_y = 0;
    int64_t dst_offset() const { return dst_y * alloc.w + dst_x; } // cells from the new buffer's start to the rectangle's first cell
};

// where lattice cell (lx, ly) lies in an allocation's memory (cells from its start), or -1 outside it
inline int64_t cell_offset(const Rect &alloc, int64_t lx, int64_t ly) {
    const int64_t cx = lx - alloc.x0, cy = ly - alloc.y0;
    return cx >= 0 && cx < alloc.w && cy >= 0 && cy < alloc.h ? cy * alloc.w + cx : -1;
}

enum { kGrowOk = 0, kGrowTooLarge = 1, kGrowOutside = 2 };

// slack: cells added on every side of what is needed whenever the memory has to grow anyway (0: every growing add reallocates).
// Where the slack alone would break the cell cap or leave the lattice it is dropped, not the add.
inline int plan_growth(const Rect &old, const Rect &need, int64_t slack, Growth *g) {
    *g = Growth();
    if (need.empty() || contains(old, need)) return kGrowOk;
    if (!in_lattice(need)) return kGrowOutside;
    const Rect both = join(old, need); // (never smaller than the old one: removal does not shrink, and the copy stays inside)
    if (both.w > kCellCap || both.h > kCellCap || both.w * both.h > kCellCap) return kGrowTooLarge;
    Rect wide = both;
    if (slack > 0) {
        if (slack > kLatticeLimit) slack = kLatticeLimit;
        wide.x0 -= slack; wide.y0 -= slack; wide.w += 2 * slack; wide.h += 2 * slack;
        if (!in_lattice(wide) || wide.w > kCellCap || wide.h > kCellCap || wide.w * wide.h > kCellCap) wide = both;
    }
    g->grow = true;
    g->alloc = wide;
    if (!old.empty()) {
        g->copy_w = old.w; g->copy_h = old.h;
        g->dst_x = old.x0 - wide.x0; g->dst_y = old.y0 - wide.y0;
    }
    return kGrowOk;
}

}  // namespace ymw
