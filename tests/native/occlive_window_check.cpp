// occlive_window_check.cpp -- the live occupancy grid's window and growth arithmetic (yag_slam_amd/csrc/ym_occlive_window.hpp) run
// as a program of its own, meant to be built with -fsanitize=address,undefined (tests/test_occupancy_live_host.py does): random grow
// sequences on real buffers, moved with exactly the offsets and rectangles the library hands to its 2-D copies, against a model
// that knows nothing of buffers (a map from lattice cell to count).  Prints "ok <sequences> <grows>" and returns 0, or says what
// broke and returns 1; a bad index is the sanitizer's to report.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <limits>
#include <map>
#include <random>
#include <utility>
#include <vector>

#include "ym_occlive_window.hpp"

using ymw::Rect;

#define CHECK(cond)                                                        \
    do {                                                                   \
        if (!(cond)) {                                                     \
            std::printf("line %d: %s (sequence %d)\n", __LINE__, #cond, g_seq); \
            return 1;                                                      \
        }                                                                  \
    } while (0)

static int g_seq = -1;

static int edge_cases() {
    const double anchor[2] = {0.5, -0.25};
    const double inf = std::numeric_limits<double>::infinity(), nan = std::numeric_limits<double>::quiet_NaN();
    Rect w;
    const double bad[][4] = {{nan, 0, 1, 1}, {0, 0, inf, 1}, {-inf, 0, 1, 1}, {0, 0, 1e300, 1}, {-1e300, -1e300, 1e300, 1e300}, {0, 0, 6e7, 1},
                             {5e7, 0, 5.5e7, 1}};
    for (const auto &b : bad) CHECK(!ymw::window_of_box(b, anchor, 20.0, &w));
    const double flat[4] = {1.0, 1.0, 3.0, 1.0}; // a box without height: a window that can be added to, not read
    CHECK(ymw::window_of_box(flat, anchor, 20.0, &w) && w.w == 40 && w.h == 0 && w.empty() && w.x0 == 10 && w.y0 == 25);
    const double tie[4] = {0.5 - 0.125, -0.25 + 0.125, 0.5 + 0.125, -0.25 + 0.375}; // -2.5 and 2.5 cells: half away from zero
    CHECK(ymw::window_of_box(tie, anchor, 20.0, &w) && w.x0 == -3 && w.y0 == 3 && w.w == 5 && w.h == 5);
    ymw::Growth g;
    Rect old, need;
    need.x0 = -5; need.y0 = 7; need.w = 50000; need.h = 50000; // 2.5e9 cells
    CHECK(ymw::plan_growth(old, need, 64, &g) == ymw::kGrowTooLarge && !g.grow);
    need.w = 40000; need.h = 50000; // exactly the cap: allowed, and the slack that would break it is dropped
    CHECK(ymw::plan_growth(old, need, 64, &g) == ymw::kGrowOk && g.grow && g.alloc.w == 40000 && g.alloc.x0 == -5 && g.copy_w == 0);
    need.x0 = ymw::kLatticeLimit - 10; need.w = 20; need.h = 20;
    CHECK(ymw::plan_growth(old, need, 0, &g) == ymw::kGrowOutside);
    need.x0 = ymw::kLatticeLimit - 100; need.w = 20; // inside, but the slack would leave the lattice: dropped
    CHECK(ymw::plan_growth(old, need, 4096, &g) == ymw::kGrowOk && g.alloc.x0 == need.x0 && g.alloc.w == 20);
    CHECK(ymw::plan_growth(need, Rect(), 5, &g) == ymw::kGrowOk && !g.grow);
    return 0;
}

int main(int argc, char **argv) {
    const int sequences = argc > 1 ? std::atoi(argv[1]) : 4000;
    if (edge_cases()) return 1;
    std::mt19937_64 rng(20240607);
    auto uni = [&](int64_t lo, int64_t hi) { return lo + (int64_t)(rng() % (uint64_t)(hi - lo + 1)); };
    long grows = 0;
    const int64_t slacks[] = {0, 0, 1, 7, 33, 64};
    for (g_seq = 0; g_seq < sequences; g_seq++) {
        const double scale = 1.0 / (0.01 * (double)uni(1, 50));
        const double anchor[2] = {(double)uni(-4000, 4000) / 7.0, (double)uni(-4000, 4000) / 7.0};
        const int64_t slack = slacks[uni(0, 5)];
        Rect alloc, window, reach;
        double box[4] = {1e300, 1e300, -1e300, -1e300};
        std::vector<uint32_t> cnt;               // two planes, like the library's pass and hit counts
        std::map<std::pair<int64_t, int64_t>, uint32_t> model;
        const int steps = (int)uni(1, 8);
        for (int step = 0; step < steps; step++) {
            // a scan: a sensor, a bounding box around it in the world and a reach rectangle around the box's cells
            const double sx = anchor[0] + (double)uni(-1000, 1000) / scale / 17.0, sy = anchor[1] + (double)uni(-1000, 1000) / scale / 17.0;
            const double b[4] = {sx - (double)uni(0, 400) / scale / 13.0, sy - (double)uni(0, 400) / scale / 13.0,
                                 sx + (double)uni(0, 400) / scale / 13.0, sy + (double)uni(0, 400) / scale / 13.0};
            box[0] = b[0] < box[0] ? b[0] : box[0]; box[1] = b[1] < box[1] ? b[1] : box[1];
            box[2] = b[2] > box[2] ? b[2] : box[2]; box[3] = b[3] > box[3] ? b[3] : box[3];
            CHECK(ymw::window_of_box(box, anchor, scale, &window));
            Rect own, r;
            CHECK(ymw::window_of_box(b, anchor, scale, &own));
            r.x0 = own.x0 - uni(0, 20); r.y0 = own.y0 - uni(0, 20);
            r.w = own.w + 1 + (own.x0 - r.x0) + uni(0, 20); r.h = own.h + 1 + (own.y0 - r.y0) + uni(0, 20);
            reach = ymw::join(reach, r);
            const Rect need = ymw::join(window, reach);
            CHECK(ymw::contains(need, window) && ymw::contains(need, reach));
            ymw::Growth g;
            CHECK(ymw::plan_growth(alloc, need, slack, &g) == ymw::kGrowOk);
            if (g.grow) {
                grows++;
                CHECK(ymw::contains(g.alloc, need) && ymw::contains(g.alloc, alloc) && ymw::in_lattice(g.alloc));
                if (slack == 0) CHECK(g.alloc.x0 == ymw::join(alloc, need).x0 && g.alloc.w == ymw::join(alloc, need).w);
                const size_t cells = (size_t)g.alloc.cells(), old_cells = (size_t)alloc.cells();
                std::vector<uint32_t> bigger(2 * cells, 0u);
                CHECK((g.copy_w > 0) == !alloc.empty());
                if (g.copy_w > 0) {
                    CHECK(g.copy_w == alloc.w && g.copy_h == alloc.h && g.dst_offset() == ymw::cell_offset(g.alloc, alloc.x0, alloc.y0));
                    for (int plane = 0; plane < 2; plane++) // hipMemcpy2D(dst, pitch alloc.w, src, pitch old.w, copy_w, copy_h), row by row
                        for (int64_t y = 0; y < g.copy_h; y++)
                            for (int64_t x = 0; x < g.copy_w; x++)
                                bigger.at(plane * cells + (size_t)g.dst_offset() + (size_t)(y * g.alloc.w + x)) =
                                    cnt.at(plane * old_cells + (size_t)(y * alloc.w + x));
                }
                cnt.swap(bigger);
                alloc = g.alloc;
            } else {
                CHECK(ymw::contains(alloc, need));
            }
            // the rays: counts anywhere in the scan's reach
            const int touches = (int)uni(1, 60);
            const size_t cells = (size_t)alloc.cells();
            for (int t = 0; t < touches; t++) {
                const int64_t lx = uni(r.x0, r.x0 + r.w - 1), ly = uni(r.y0, r.y0 + r.h - 1);
                const int64_t off = ymw::cell_offset(alloc, lx, ly);
                CHECK(off >= 0);
                cnt.at((size_t)off) += 1u;
                cnt.at(cells + (size_t)off) += 3u;
                model[{lx, ly}] += 1u;
            }
            CHECK(ymw::cell_offset(alloc, alloc.x0 - 1, alloc.y0) == -1 && ymw::cell_offset(alloc, alloc.x0, alloc.y0 + alloc.h) == -1);
            // every count is where the lattice says, and nothing else is anywhere
            uint64_t want = 0, have = 0;
            for (const auto &kv : model) {
                const int64_t off = ymw::cell_offset(alloc, kv.first.first, kv.first.second);
                CHECK(off >= 0 && cnt.at((size_t)off) == kv.second && cnt.at(cells + (size_t)off) == 3u * kv.second);
                want += kv.second;
            }
            for (size_t i = 0; i < cells; i++) have += cnt[i];
            CHECK(want == have);
            // the window reads as a dense image from its first cell on, rows alloc.w apart
            if (!window.empty()) {
                const int64_t first = ymw::cell_offset(alloc, window.x0, window.y0);
                CHECK(first >= 0);
                const uint32_t last = cnt.at((size_t)(first + (window.h - 1) * alloc.w + window.w - 1));
                const auto it = model.find({window.x0 + window.w - 1, window.y0 + window.h - 1});
                CHECK(last == (it == model.end() ? 0u : it->second));
            }
        }
    }
    std::printf("ok %d %ld\n", sequences, grows);
    return 0;
}
