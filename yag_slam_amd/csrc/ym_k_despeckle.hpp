// ym_k_despeckle.hpp -- a connected-component area filter for byte images: every component of `foreground` cells with fewer
// than min_area cells becomes `fill`, the cleanup the ROS node applies to a rendered occupancy grid before it publishes it
// (ros1/slam_node_ros1:191-197, there with cv2.connectedComponentsWithStats).  The rules are DESIGN.md section 12; they are
// pinned by tests/despeckle_ref.py.  Only component AREAS are used, so no label numbering exists here.
//
// The component stage shares its union-find with the segmenter's (ym_k_unionfind.hpp: atomicMin towards the lowest
// raster index, so the root of a component is its first cell whatever the order of arrival).  The tiling is the segmenter's too:
// a block of 256 threads takes 64 columns x 16 rows, wave w rows 4 w .. 4 w + 3, a lane one column.  The grid is
// one-dimensional (nbx blocks per row of tiles) so that an image of any shape within 2^31 - 1 cells can be launched.
//
// dsp_init_kernel    parent = the start of the cell's run of foreground within its wave's 64 columns, size = 0 (foreground
//                    cells only: nothing else of the two arrays is ever read); counts foreground and other cells.
// dsp_merge_kernel<kConn>
//                    the unions that are MADE, for a foreground cell c = (x, y) with L = (x - 1, y), R = (x + 1, y),
//                    U = (x, y - 1), UL = (x - 1, y - 1), UR = (x + 1, y - 1), each only where that cell is foreground:
//                      c - L   at lane 0 only.  Within a wave the run is one tree from the init pass on.
//                      c - U   unless L and UL are both foreground and in the same wave.  Then L is joined to UL (made, or
//                              implied in the same way further left: the chain ends at lane 0 or where L or UL is missing),
//                              UL - U is a run of the upper row and L - c one of this row.
//                    So every pair of horizontal or vertical neighbours is in one tree; that is 4-connectivity.  Under 8:
//                      c - UL  only if neither U nor L is foreground.  With U: UL - U are horizontal neighbours.  With L: L - UL
//                              are vertical neighbours and L - c horizontal ones.  This holds on either side of a 64-column
//                              border, because c - L across the border is made at lane 0.
//                      c - UR  only if neither U nor R is foreground.  With U: U - UR are horizontal neighbours.  With R: R - UR
//                              are vertical neighbours, and c - R is a run, or the union R makes at its lane 0.
//                    A wave without a foreground cell in a row leaves the row after one load.
// dsp_sizes_kernel   every foreground cell's parent becomes its root, every root's size its cells: one integer atomic per
//                    distinct root of a wave's 64 cells.  A wave without foreground does nothing.
// dsp_apply_kernel   out = fill where (foreground and size[root] < min_area) or (not foreground and the background rule
//                    fired: 0 < other cells < min_area), else the input byte.  Counts components, removed components and
//                    cleared cells.  `out` may be the input image.
// Every loop has a bound: the walk to a root follows strictly decreasing indices, a union retries at most kUnionCap times
// and then raises stats[kDspErr], and the host fails the call.  Stages depend on each other only across launches.  All sums
// that cross threads are integer sums: the output is the same from run to run.  No kernel uses scratch or LDS.  Plain C++
// and vector memory operations only.  Part of ym_kernels.hpp.
#pragma once

namespace ym {

enum { kDspFg = 0, kDspBg = 1, kDspComponents = 2, kDspRemoved = 3, kDspCleared = 4, kDspErr = 5, kDspStatSlots = 8 };

struct DespeckleArgs {
    const uint8_t *image; // [height][width] (dense)
    uint8_t *out;         // [height][width]; may be `image`
    int32_t width, height;
    int32_t nbx;          // ceil(width / 64): block b takes tile (b % nbx, b / nbx)
    int32_t foreground, fill;
    unsigned min_area;
    unsigned *parent;     // [height * width] at a foreground cell: raster index of a cell of its component, never above its own
    unsigned *size;       // [height * width] at a root: the component's cells
    unsigned long long *stats; // [kDspStatSlots]
};

__device__ __forceinline__ int dsp_tile_x(const DespeckleArgs &a) { return (int)(blockIdx.x % (unsigned)a.nbx) * 64 + (int)(threadIdx.x & 63); }
__device__ __forceinline__ int dsp_tile_y(const DespeckleArgs &a, int j) {
    return (int)(blockIdx.x / (unsigned)a.nbx) * 16 + (int)(threadIdx.x >> 6) * 4 + j; // (the same for every lane of a wave)
}

// grid nbx * ceil(height / 16), 256 threads
__global__ __launch_bounds__(256) void dsp_init_kernel(DespeckleArgs a) {
    const int lane = threadIdx.x & 63, x = dsp_tile_x(a);
    unsigned n_fg = 0, n_bg = 0;
#pragma unroll 1
    for (int j = 0; j < 4; j++) {
        const int y = dsp_tile_y(a, j);
        if (y >= a.height) break;
        const bool in = x < a.width;
        const bool fg = in && a.image[(size_t)y * a.width + x] == a.foreground;
        const unsigned long long m = __ballot(fg);
        n_fg += (unsigned)__popcll(m);
        n_bg += (unsigned)__popcll(__ballot(in && !fg));
        if (!m) continue;
        const unsigned long long starts = m & ~(m << 1); // foreground lanes whose left lane is not
        const int first = 63 - __clzll((long long)(starts & (~0ull >> (63 - lane)))); // the last run start at or before this lane
        if (fg) {
            const size_t i = (size_t)y * a.width + x;
            a.parent[i] = (unsigned)(i - (size_t)(lane - first));
            a.size[i] = 0;
        }
    }
    if (lane == 0) {
        if (n_fg) atomicAdd(&a.stats[kDspFg], (unsigned long long)n_fg);
        if (n_bg) atomicAdd(&a.stats[kDspBg], (unsigned long long)n_bg);
    }
}

__device__ __forceinline__ void dsp_union(const DespeckleArgs &a, unsigned i, unsigned j) {
    if (!uf_union(a.parent, i, j)) atomicOr(&a.stats[kDspErr], 1ull);
}

// grid as dsp_init_kernel.  kConn: 4 or 8
template <int kConn>
__global__ __launch_bounds__(256) void dsp_merge_kernel(DespeckleArgs a) {
    const int lane = threadIdx.x & 63, x = dsp_tile_x(a);
    const uint8_t f = (uint8_t)a.foreground;
#pragma unroll 1
    for (int j = 0; j < 4; j++) {
        const int y = dsp_tile_y(a, j);
        if (y >= a.height) break;
        const uint8_t *row = a.image + (size_t)y * a.width;
        const bool fg = x < a.width && row[x] == f;
        if (!fg) continue; // (a wave without foreground in this row leaves it here as a whole)
        const unsigned i = (unsigned)((size_t)y * a.width + x);
        const bool l = x > 0 && row[x - 1] == f;
        if (l && lane == 0) dsp_union(a, i, i - 1u);
        if (y == 0) continue;
        const uint8_t *up = row - a.width;
        const bool u = up[x] == f;
        if (u) {
            if (lane == 0 || !l || up[x - 1] != f) dsp_union(a, i, i - (unsigned)a.width);
        } else if (kConn == 8) {
            if (!l && x > 0 && up[x - 1] == f) dsp_union(a, i, i - (unsigned)a.width - 1u);
            if (x + 1 < a.width && up[x + 1] == f && row[x + 1] != f) dsp_union(a, i, i - (unsigned)a.width + 1u);
        }
    }
}

// grid as dsp_init_kernel
__global__ __launch_bounds__(256) void dsp_sizes_kernel(DespeckleArgs a) {
    const int x = dsp_tile_x(a);
#pragma unroll 1
    for (int j = 0; j < 4; j++) {
        const int y = dsp_tile_y(a, j);
        if (y >= a.height) break;
        const bool fg = x < a.width && a.image[(size_t)y * a.width + x] == a.foreground;
        uf_wave_sizes(fg, (unsigned)((size_t)y * a.width + x), a.parent, a.size);
    }
}

// grid as dsp_init_kernel
__global__ __launch_bounds__(256) void dsp_apply_kernel(DespeckleArgs a) {
    const int lane = threadIdx.x & 63, x = dsp_tile_x(a);
    const unsigned long long n_bg = a.stats[kDspBg]; // (final since the init launch)
    const bool fill_bg = n_bg > 0 && n_bg < (unsigned long long)a.min_area;
    unsigned comps = 0, removed = 0, cleared = 0;
#pragma unroll 1
    for (int j = 0; j < 4; j++) {
        const int y = dsp_tile_y(a, j);
        if (y >= a.height) break;
        const size_t i = (size_t)y * a.width + x;
        const bool in = x < a.width;
        const uint8_t v = in ? a.image[i] : (uint8_t)0;
        const bool fg = in && v == a.foreground;
        bool small = false, is_root = false;
        if (fg) {
            const unsigned root = a.parent[i];
            is_root = root == (unsigned)i;
            small = a.size[root] < a.min_area;
        }
        if (in) a.out[i] = (fg ? small : fill_bg) ? (uint8_t)a.fill : v;
        comps += (unsigned)__popcll(__ballot(is_root));
        removed += (unsigned)__popcll(__ballot(is_root && small));
        cleared += (unsigned)__popcll(__ballot(small));
    }
    if (lane == 0) {
        if (comps) atomicAdd(&a.stats[kDspComponents], (unsigned long long)comps);
        if (removed) atomicAdd(&a.stats[kDspRemoved], (unsigned long long)removed);
        if (cleared) atomicAdd(&a.stats[kDspCleared], (unsigned long long)cleared);
    }
}

}  // namespace ym
