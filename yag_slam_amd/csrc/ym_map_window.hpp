// ym_map_window.hpp -- the integer arithmetic of a correlation map's window (DESIGN.md sections 15 to 17), on the host.  Needs
// neither HIP nor the rest of the library: ym_host_mapgrow.hpp and ym_abi_maps.hpp use it, and so does the stand-alone program
// tests/native/map_window_check.cpp, which checks every function against brute force under the address and undefined-behaviour
// sanitizers.
//
// A map is width x height cells; its cell (0, 0) is cell (x0, y0) -- the window's offset -- of the lattice it started in.
#pragma once
#include <cstdint>

namespace ymm {

constexpr int kMaxOffset = 1 << 30;    // a window's offset in lattice cells: exact in fp64 and in the int32 of the kernels
constexpr unsigned kMaxGridRows = 65535; // a launch has at most this many rows of blocks

inline bool offset_ok(int64_t x0, int64_t y0) { return x0 >= -kMaxOffset && x0 <= kMaxOffset && y0 >= -kMaxOffset && y0 <= kMaxOffset; }

struct Box { // the cells [x0, x1) x [y0, y1); empty when x1 <= x0 or y1 <= y0
    int x0 = 0, y0 = 0, x1 = 0, y1 = 0;
    bool empty() const { return x1 <= x0 || y1 <= y0; }
};

inline int64_t max64(int64_t a, int64_t b) { return a > b ? a : b; }
inline int64_t min64(int64_t a, int64_t b) { return a < b ? a : b; }

// ym_map_reframe: new cell (i, j) is old cell (i + dx, j + dy).  The overlap of the old window (old_w x old_h) and the new one
// (width x height), in cells of the new one; without an overlap the empty box 0, 0, 0, 0.  (int64 inside: dx, dy are any int)
inline Box overlap(int old_w, int old_h, int dx, int dy, int width, int height) {
    const int64_t x0 = max64(0, -(int64_t)dx), x1 = min64(width, (int64_t)old_w - dx);
    const int64_t y0 = max64(0, -(int64_t)dy), y1 = min64(height, (int64_t)old_h - dy);
    Box b;
    if (x1 > x0 && y1 > y0) { b.x0 = (int)x0; b.y0 = (int)y0; b.x1 = (int)x1; b.y1 = (int)y1; }
    return b;
}

// The shift handed to the copy kernel.  Without an overlap every source test of the copy must fail: a shift no window reaches,
// which cannot overflow the kernel's int32 sums (x + dx with 0 <= x < 10^9).
struct Shift { int dx, dy; };
inline Shift copy_shift(bool overlaps, int dx, int dy) { return overlaps ? Shift{dx, dy} : Shift{-kMaxOffset * 2 + 1, 0}; }

// A box of cells widened by the taps' reach (half cells every way) and cut to the map: the bounding box of every cell a tap
// reaches from a cell of the box.  An empty box stays empty.
inline Box widen(const Box &b, int half, int width, int height) {
    Box r;
    if (b.empty()) return r;
    r.x0 = (int)max64(0, (int64_t)b.x0 - half); r.y0 = (int)max64(0, (int64_t)b.y0 - half);
    r.x1 = (int)min64(width, (int64_t)b.x1 + half); r.y1 = (int)min64(height, (int64_t)b.y1 + half);
    return r;
}

// the box of the statistics slots X0, Y0, X1, Y1 (X1, Y1 inclusive), widened and cut
inline Box widen_stats(const unsigned long long xyxy[4], int half, int width, int height) {
    Box b;
    b.x0 = (int)xyxy[0]; b.y0 = (int)xyxy[1]; b.x1 = (int)xyxy[2] + 1; b.y1 = (int)xyxy[3] + 1;
    return widen(b, half, width, height);
}

inline Box join(const Box &a, const Box &b) {
    if (a.empty()) return b;
    if (b.empty()) return a;
    Box r;
    r.x0 = a.x0 < b.x0 ? a.x0 : b.x0; r.y0 = a.y0 < b.y0 ? a.y0 : b.y0;
    r.x1 = a.x1 > b.x1 ? a.x1 : b.x1; r.y1 = a.y1 > b.y1 ? a.y1 : b.y1;
    return r;
}

// ym_map_reframe's mark rectangle: the cells of the new window within the taps' reach of the overlap
inline Box mark_rect(const Box &overlap_box, int half, int width, int height) { return widen(overlap_box, half, width, height); }

// The recompute's tile grid over a box: the origin rounded down to the tile, the tiles that cover the box from there.
struct TileGrid { int bx0 = 0, by0 = 0; unsigned tiles_x = 0, tiles_y = 0; };
inline TileGrid tile_grid(const Box &b, int tile_w, int tile_h) {
    TileGrid g;
    if (b.empty()) return g;
    g.bx0 = b.x0 / tile_w * tile_w; g.by0 = b.y0 / tile_h * tile_h;
    g.tiles_x = (unsigned)((b.x1 - g.bx0 + tile_w - 1) / tile_w); g.tiles_y = (unsigned)((b.y1 - g.by0 + tile_h - 1) / tile_h);
    return g;
}

// `rows` rows of blocks in launches of at most kMaxGridRows: piece k starts at row first and has count rows
struct RowPiece { unsigned first, count; };
inline unsigned row_pieces(unsigned rows) { return (rows + kMaxGridRows - 1) / kMaxGridRows; }
inline RowPiece row_piece(unsigned rows, unsigned k) {
    const unsigned first = k * kMaxGridRows, left = rows - first;
    return RowPiece{first, left < kMaxGridRows ? left : kMaxGridRows};
}

}  // namespace ymm
