// ym_k_yagmap.hpp -- "yagpy" semantics against a prebuilt map, many items per enqueue: map_points_many_kernel, yag_map_kernel.
// Part of ym_kernels.hpp (include that, not this file).
#pragma once

namespace ym {

// The query point sets of N independent match_scan_sets_with_map calls (map_points_kernel's work, one block per item): item b's
// scans are scans[scan_begin .. scan_begin + n_scans), its points go to out + out_off and their number to states[b].nq.
struct MapItemDesc {
    int32_t scan_begin, n_scans;
    int64_t out_off;          // in points
    double ox_real, oy_real;  // the item's search centre: the mean of its query positions, computed on the host
};
struct MapPointsManyArgs {
    const YmScanRef *scans;
    const MapItemDesc *items;
    int32_t max_n, pad;
    double2 *out;
    YmItemState *states;
};
// grid (n_items), 1024 threads, dynamic LDS = YM_PREP_LDS_BYTES(max_n)
__global__ __launch_bounds__(1024) void map_points_many_kernel(MapPointsManyArgs a) {
    constexpr int NT = 1024;
    extern __shared__ __attribute__((aligned(16))) unsigned char lds_raw[];
    __shared__ int s_cnt[(YM_MAX_BEAMS / NT + 1) * (NT / 64)];
    const PrepLds l = prep_lds(lds_raw, a.max_n);
    const MapItemDesc it = a.items[blockIdx.x];
    double2 *out = a.out + it.out_off;
    int total = 0;
    const double c0 = cos(0.0), s0 = sin(0.0), tx = -it.ox_real, ty = -it.oy_real;
    for (int q = 0; q < it.n_scans; q++) {
        const YmScanRef sr = a.scans[it.scan_begin + q];
        const int np = project_points<NT>(sr, sr.pose[0], sr.pose[1], sr.pose[2], true, l.sx, l.sy, s_cnt);
        for (int i = threadIdx.x; i < np; i += NT) {
            const double px = l.sx[i], py = l.sy[i];
            out[total + i] = make_double2((px * c0 - py * s0) + tx, (py * c0 + px * s0) + ty);
        }
        total += np;
        __syncthreads();
    }
    if (threadIdx.x == 0) a.states[blockIdx.x].nq = total;
}

// The integer sums of yag_score_kernel's map branch for either pass, without its roundings per (hypothesis, point) pair.  Hypothesis
// (ix, iy, k) reads for point l the cell (rint(((xv[ix] + r.x) - map_ox) / res), rint(((yv[iy] + r.y) - map_oy) / res)), r = the point
// rotated by tv[k] (helpers.py:134-153): the column depends on (ix, l, k) alone and the row on (iy, l, k) alone, so a (point, angle) pair
// costs nx + ny roundings instead of 2 nx ny -- the same operations on the same operands, the division through yag_rint_div.
// One block of four waves per (item, angle).  The block walks the item's points in tiles of YM_YAG_MAP_TILE: wave w takes the points
// w, w + 4, ... of the tile, lane i writes the column of hypothesis column i and the row offset (row * map_w) of hypothesis row i to
// LDS, -1 for a cell outside the map.  After the barrier thread (w, lane) owns column ix = lane and the rows iy = w, w + 4, ...: per
// point one column read, per row a row-offset read that is the same address for the whole wave, and one map byte -- the lanes of a
// wave read neighbouring bytes of one map row (a lattice step is a fraction of a cell).  The sixteen sums of a thread stay in registers.
// Lattices up to YM_YAG_MAP_DIM positions per axis; an item with a wider one is left to yag_score_kernel (YagArgs::map_dim makes that
// kernel skip the items served here) and counted.  Blocks are dealt to the XCDs as yag_fine_kernel's are: the angles of an item share one L2.
// A few items alone leave the device empty -- one item is 21 blocks, each walking a thousand points one latency after the other -- so
// on small calls map_split blocks share the points of an (item, angle): each adds its partial sums to the zeroed volume with integer
// atomics (exact whatever the order) and yag_map_score_kernel scores the finished sums.  map_split = 1: the block scores its own.
// YagArgs::map_sets (match_scan_sets, ym_k_sets.hpp): the map is the item's own grid (grid_stride), its corner the item's off_x, off_y,
// and the penalty find_best_pose's, centred on the grid; the items are counted apart.
#define YM_YAG_MAP_DIM 64
#define YM_YAG_MAP_TILE 32
__global__ __launch_bounds__(256) void yag_map_kernel(YagArgs a) {
    constexpr int D = YM_YAG_MAP_DIM, P = YM_YAG_MAP_TILE, NW = 4, R = D / NW;
    __shared__ int s_col[P][D], s_row[P][D];
    __shared__ double2 s_cs;
    const int S = a.map_split > 1 ? a.map_split : 1;
    const int xcd = blockIdx.x & 7, j_ = (blockIdx.x >> 3) / S, part = (blockIdx.x >> 3) % S; // (the parts of an (item, angle) on one XCD)
    const int b = (j_ / a.maxt) * 8 + xcd, k = j_ % a.maxt, tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    if (b >= a.n_items) return;
    const YmItemState &st = a.states[b];
    const int nx = st.ydims[a.pass][0], ny = st.ydims[a.pass][1], nt = st.ydims[a.pass][2];
    const bool served = nx <= D && ny <= D;
    if (a.counters && a.pass == 0 && k == 0 && part == 0 && tid == 0) atomicAdd(&a.counters[(served ? 4 : 5) + (a.map_sets ? 2 : 0)], 1ull);
    if (!served || k >= nt || nx * ny == 0) return; // (block-uniform)
    const double *ax = a.axes + (size_t)b * 3 * YM_YAG_MAX_DIM;
    const double xv = lane < nx ? ax[lane] : 0.0, yv = lane < ny ? ax[YM_YAG_MAX_DIM + lane] : 0.0, tv = ax[2 * YM_YAG_MAX_DIM + k];
    if (tid == 0) s_cs = make_double2(cos(tv), sin(tv));
    __syncthreads();
    const double rc = s_cs.x, rs = s_cs.y;
    const double ox = a.map_sets ? st.off_x : a.map_ox, oy = a.map_sets ? st.off_y : a.map_oy, res = a.map_res, rres = 1.0 / res;
    const int GW = a.map_w, GH = a.map_h;
    const double2 *__restrict__ ql = reinterpret_cast<const double2 *>(st.ql);
    const uint8_t *__restrict__ grid = a.grid + (size_t)b * a.grid_stride;
    const int np = st.nq;
    unsigned acc[R];
#pragma unroll
    for (int j = 0; j < R; j++) acc[j] = 0u;
    const int share = ((np + S - 1) / S + P - 1) / P * P; // points per part: whole tiles
    const int l_end = min(np, (part + 1) * share);
    for (int l0 = part * share; l0 < l_end; l0 += P) {
        const int pc = min(P, l_end - l0);
        for (int p = w; p < pc; p += NW) {
            const double2 r = yag_rotate(ql[l0 + p], rc, rs);
            if (lane < nx) {
                const double x = xv + r.x;
                const double gx = yag_rint_div(x - ox, res, rres);
                const int _x = (int)gx;
                s_col[p][lane] = (_x >= 0 && _x < GW) ? _x : -1;
            }
            if (lane < ny) {
                const double y = yv + r.y;
                const double gy = yag_rint_div(y - oy, res, rres);
                const int _y = (int)gy;
                s_row[p][lane] = (_y >= 0 && _y < GH) ? _y * GW : -1; // (below 2^31: a map holds at most 10^9 cells)
            }
        }
        __syncthreads();
        if (lane < nx)
            for (int p = 0; p < pc; p++) {
                const int c = s_col[p][lane];
#pragma unroll
                for (int j = 0; j < R; j++) {
                    const int iy = w + NW * j; // (wave-uniform)
                    if (iy < ny) {
                        // (no branch on the cell: byte 0 of the map stands in for a cell outside it and adds nothing, so the
                        // loads of a point -- and of the next -- are in flight together)
                        const int ro = s_row[p][iy];
                        const bool in = (c | ro) >= 0;
                        const unsigned v = grid[in ? (unsigned)(ro + c) : 0u];
                        acc[j] += in ? v : 0u;
                    }
                }
            }
        __syncthreads();
    }
    if (lane < nx)
#pragma unroll
        for (int j = 0; j < R; j++) {
            const int iy = w + NW * j;
            if (iy >= ny) continue;
            if (S == 1) yag_store_score(a, st, b, k, iy, lane, nx, ny, acc[j], np, xv, ax[YM_YAG_MAX_DIM + iy], tv, ox, oy, res, GW, !a.map_sets);
            else if (acc[j]) atomicAdd(&a.sums[(size_t)b * a.vol_stride + ((size_t)k * ny + iy) * nx + lane], acc[j]);
        }
}

// map_split > 1: the scores of the sums the parts added up.  grid (ceil(maxd * maxd / 256), maxt, B): yag_score_kernel's shape.
__global__ __launch_bounds__(256) void yag_map_score_kernel(YagArgs a) {
    const int b = blockIdx.z, k = blockIdx.y;
    const YmItemState &st = a.states[b];
    const int nx = st.ydims[a.pass][0], ny = st.ydims[a.pass][1], nt = st.ydims[a.pass][2];
    const int c = blockIdx.x * 256 + threadIdx.x;
    if (k >= nt || c >= nx * ny || nx > a.map_dim || ny > a.map_dim) return;
    const int iy = c / nx, ix = c - iy * nx;
    const double *ax = a.axes + (size_t)b * 3 * YM_YAG_MAX_DIM;
    const unsigned sum = a.sums[(size_t)b * a.vol_stride + ((size_t)k * ny + iy) * nx + ix];
    yag_store_score(a, st, b, k, iy, ix, nx, ny, sum, st.nq, ax[ix], ax[YM_YAG_MAX_DIM + iy], ax[2 * YM_YAG_MAX_DIM + k], a.map_sets ? st.off_x : a.map_ox,
                    a.map_sets ? st.off_y : a.map_oy, a.map_res, a.map_w, !a.map_sets);
}

}  // namespace ym
