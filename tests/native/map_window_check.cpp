// map_window_check.cpp -- a correlation map's window arithmetic (yag_slam_amd/csrc/ym_map_window.hpp) run as a program of its own,
// meant to be built with -fsanitize=address,undefined (tests/test_map_reframe_host.py does): every function against brute force on
// small windows, and the limits at their edges.  Prints "ok <checks>" and returns 0, or says what broke and returns 1; an overflow
// is the sanitizer's to report.
#include <climits>
#include <cstdint>
#include <cstdio>
#include <initializer_list>
#include <vector>

#include "ym_map_window.hpp"

using ymm::Box;

static long g_checks = 0;

#define CHECK(cond)                                        \
    do {                                                   \
        g_checks++;                                        \
        if (!(cond)) {                                     \
            std::printf("line %d: %s\n", __LINE__, #cond); \
            return 1;                                      \
        }                                                  \
    } while (0)

static bool same(const Box &a, const Box &b) { return a.x0 == b.x0 && a.y0 == b.y0 && a.x1 == b.x1 && a.y1 == b.y1; }

// the bounding box of a set of cells, grown cell by cell; empty: 0, 0, 0, 0
struct Bounds {
    bool any = false;
    Box b;
    void add(int x, int y) {
        if (!any) { b.x0 = x; b.y0 = y; b.x1 = x + 1; b.y1 = y + 1; any = true; return; }
        if (x < b.x0) b.x0 = x;
        if (y < b.y0) b.y0 = y;
        if (x + 1 > b.x1) b.x1 = x + 1;
        if (y + 1 > b.y1) b.y1 = y + 1;
    }
};

static int offset_limit() {
    const int64_t lim = (int64_t)1 << 30;
    CHECK(ymm::kMaxOffset == lim);
    for (int64_t s : {(int64_t)-1, (int64_t)1}) {
        CHECK(ymm::offset_ok(s * lim, 0) && ymm::offset_ok(0, s * lim) && ymm::offset_ok(s * lim, -s * lim));
        CHECK(!ymm::offset_ok(s * (lim + 1), 0) && !ymm::offset_ok(0, s * (lim + 1)) && !ymm::offset_ok(s * lim, s * (lim + 1)));
    }
    CHECK(ymm::offset_ok(0, 0) && !ymm::offset_ok((int64_t)INT_MAX + INT_MAX, 0) && !ymm::offset_ok(0, (int64_t)INT_MIN + INT_MIN));
    return 0;
}

// the overlap is the set of new cells whose source lies inside the old window; the shift of a call without one reaches no window
static int overlaps() {
    const int sizes[][2] = {{1, 1}, {3, 2}, {5, 7}, {8, 3}};
    for (const auto &o : sizes)
        for (const auto &w : sizes)
            for (int dx = -10; dx <= 10; dx++)
                for (int dy = -10; dy <= 10; dy++) {
                    Bounds want;
                    long cells = 0;
                    for (int y = 0; y < w[1]; y++)
                        for (int x = 0; x < w[0]; x++)
                            if (x + dx >= 0 && x + dx < o[0] && y + dy >= 0 && y + dy < o[1]) { want.add(x, y); cells++; }
                    const Box got = ymm::overlap(o[0], o[1], dx, dy, w[0], w[1]);
                    CHECK(got.empty() == !want.any && same(got, want.b));
                    CHECK((long)(got.x1 - got.x0) * (got.y1 - got.y0) == cells); // (two rectangles meet in a rectangle)
                    const ymm::Shift s = ymm::copy_shift(!got.empty(), dx, dy);
                    if (!got.empty()) CHECK(s.dx == dx && s.dy == dy);
                    else CHECK(s.dx == -2147483647 && s.dy == 0);
                }
    // dx, dy are any int: nothing overflows, and nothing overlaps that far away
    const int far[] = {INT_MIN, INT_MIN + 1, -(1 << 30), 1 << 30, INT_MAX - 1, INT_MAX};
    for (int d : far) {
        CHECK(ymm::overlap(1000000000, 1, d, 0, 1000000000, 1).empty() == (d <= -1000000000 || d >= 1000000000));
        CHECK(ymm::overlap(7, 1000000000, 0, d, 7, 1000000000).empty() == (d <= -1000000000 || d >= 1000000000));
        CHECK(ymm::overlap(31623, 31623, d, d, 31623, 31623).empty());
    }
    return 0;
}

// x + shift for every x a kernel forms (0 <= x < 10^9): no int32 overflow, and below every source window of up to 10^9 cells
static int no_overlap_shift() {
    const ymm::Shift s = ymm::copy_shift(false, 12345, -6789);
    const int64_t xs[] = {0, 1, 65535, 999999998, 999999999};
    for (int64_t x : xs) {
        const int64_t sx = x + (int64_t)s.dx, sy = x + (int64_t)s.dy;
        CHECK(sx >= (int64_t)INT_MIN && sx <= (int64_t)INT_MAX && sy >= (int64_t)INT_MIN && sy <= (int64_t)INT_MAX);
        CHECK(sx < 0); // a source window is [0, src_w): the column test fails whatever the row
    }
    return 0;
}

// the widened box is the bounding box of every cell a tap reaches from the box, cut to the map
static int widened() {
    const int maps[][2] = {{1, 1}, {6, 4}, {9, 9}};
    for (const auto &mp : maps)
        for (int half = 0; half <= 3; half++)
            for (int x0 = 0; x0 < mp[0]; x0++)
                for (int y0 = 0; y0 < mp[1]; y0++)
                    for (int x1 = x0 + 1; x1 <= mp[0]; x1++)
                        for (int y1 = y0 + 1; y1 <= mp[1]; y1++) {
                            Bounds want;
                            for (int y = y0; y < y1; y++)
                                for (int x = x0; x < x1; x++)
                                    for (int sy = -half; sy <= half; sy++)
                                        for (int sx = -half; sx <= half; sx++)
                                            if (x + sx >= 0 && x + sx < mp[0] && y + sy >= 0 && y + sy < mp[1]) want.add(x + sx, y + sy);
                            Box b;
                            b.x0 = x0; b.y0 = y0; b.x1 = x1; b.y1 = y1;
                            CHECK(same(ymm::widen(b, half, mp[0], mp[1]), want.b));
                            CHECK(same(ymm::mark_rect(b, half, mp[0], mp[1]), want.b));
                            const unsigned long long slots[4] = {(unsigned long long)x0, (unsigned long long)y0, (unsigned long long)(x1 - 1),
                                                                 (unsigned long long)(y1 - 1)}; // (the statistics' X1, Y1 are inclusive)
                            CHECK(same(ymm::widen_stats(slots, half, mp[0], mp[1]), want.b));
                        }
    CHECK(ymm::widen(Box(), 5, 100, 100).empty() && ymm::mark_rect(Box(), 5, 100, 100).empty());
    Box a, b; // the largest map there is: nothing overflows at its far corner
    a.x0 = 999999990; a.x1 = 1000000000; a.y0 = 0; a.y1 = 1;
    b = ymm::widen(a, 1 << 20, 1000000000, 1);
    CHECK(b.x0 == 999999990 - (1 << 20) && b.x1 == 1000000000 && b.y0 == 0 && b.y1 == 1);
    CHECK(same(ymm::join(Box(), a), a) && same(ymm::join(a, Box()), a) && ymm::join(Box(), Box()).empty());
    b.x0 = 3; b.x1 = 5; b.y0 = 2; b.y1 = 9;
    const Box j = ymm::join(a, b);
    CHECK(j.x0 == 3 && j.x1 == 1000000000 && j.y0 == 0 && j.y1 == 9);
    return 0;
}

// the tiles cover the box from an origin on the tile lattice, and the row pieces cover every tile row exactly once
static int tiles_and_pieces() {
    const int tw = 64, th = 4;
    const int heights[] = {1, 3, 4, 5, 262139, 262140, 262141, 262209, 4 * 65535 * 2, 4 * 65535 * 2 + 1};
    const int origins[] = {0, 1, 3, 4, 6, 71};
    for (int h : heights)
        for (int y0 : origins)
            for (int x0 : {0, 5, 63, 64, 130}) {
                if (y0 >= h) continue;
                Box b;
                b.x0 = x0; b.x1 = x0 + 70; b.y0 = y0; b.y1 = h;
                const ymm::TileGrid t = ymm::tile_grid(b, tw, th);
                CHECK(t.bx0 % tw == 0 && t.by0 % th == 0 && t.bx0 <= b.x0 && b.x0 - t.bx0 < tw && t.by0 <= b.y0 && b.y0 - t.by0 < th);
                CHECK((int64_t)t.bx0 + (int64_t)t.tiles_x * tw >= b.x1 && (int64_t)t.bx0 + (int64_t)(t.tiles_x - 1) * tw < b.x1);
                CHECK((int64_t)t.by0 + (int64_t)t.tiles_y * th >= b.y1 && (int64_t)t.by0 + (int64_t)(t.tiles_y - 1) * th < b.y1);
                // the launches as the library makes them: piece k covers the cell rows from by0 + first * th on
                std::vector<unsigned char> seen(t.tiles_y, 0);
                unsigned next = 0;
                for (unsigned k = 0; k < ymm::row_pieces(t.tiles_y); k++) {
                    const ymm::RowPiece p = ymm::row_piece(t.tiles_y, k);
                    CHECK(p.count >= 1 && p.count <= 65535 && p.first == next);
                    CHECK((int64_t)t.by0 + (int64_t)p.first * th <= INT_MAX);
                    for (unsigned r = 0; r < p.count; r++) seen.at(p.first + r)++;
                    next = p.first + p.count;
                }
                CHECK(next == t.tiles_y);
                for (unsigned char s : seen) CHECK(s == 1);
            }
    CHECK(ymm::tile_grid(Box(), tw, th).tiles_x == 0 && ymm::tile_grid(Box(), tw, th).tiles_y == 0 && ymm::row_pieces(0) == 0);
    // the pieces themselves: the mark's rows are cell rows
    const unsigned rows[] = {1, 65534, 65535, 65536, 2 * 65535, 2 * 65535 + 1, 262209, 1000000000};
    for (unsigned n : rows) {
        const unsigned k = ymm::row_pieces(n);
        CHECK(k == (n + 65534) / 65535);
        uint64_t covered = 0;
        for (unsigned i = 0; i < k; i++) {
            const ymm::RowPiece p = ymm::row_piece(n, i);
            CHECK(p.first == covered && p.count >= 1 && p.count <= 65535 && (i + 1 == k || p.count == 65535));
            covered += p.count;
        }
        CHECK(covered == n);
    }
    CHECK(ymm::row_pieces(262209) == 5 && ymm::row_pieces((262209 + 3) / 4) == 2);
    return 0;
}

int main() {
    if (offset_limit() || overlaps() || no_overlap_shift() || widened() || tiles_and_pieces()) return 1;
    std::printf("ok %ld\n", g_checks);
    return 0;
}
