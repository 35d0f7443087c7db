// ym_k_mapgrow.hpp -- a resident correlation map that takes scans: map_grow_cells_kernel, map_grow_smear_kernel, map_clear_kernel.
// Part of ym_kernels.hpp (include that, not this file).  DESIGN.md section 15.
#pragma once

namespace ym {

// The reference's add_scan_to_grid (helpers.py:105-131: per point reading the cell becomes 1.0 and smear_point max-stamps the
// float kernel around it) into a map that stays on the device.  Every write is a maximum -- the stamp itself too: the tables' centre tap
// and 1.0 are the largest values a grid holds -- so the result depends neither on the order of the points nor on that of the scans.
// Two stages:
//   cells   one lane per beam: the world point of project_points(., true, .) -- the same expressions on the same operands, without
//           its compaction, for which no order is needed here --, the cell of world_to_grid (helpers.py:82-83: fp64 division, round
//           half to even), the counts and the bounding box of the stamped cells
//   smear   one lane per (beam, tap): a 64-bit unsigned atomic maximum on the bit pattern of the cell's double.  For doubles >= 0 the
//           order of the bit patterns is the order of the values, grids hold values in [0, 1] (ym_map_from_grid's contract) and taps
//           are > 0.  The taps of a row are consecutive lanes and consecutive doubles: a wave instruction is two or three contiguous
//           segments.  A plain load first: a cell that already holds at least the tap -- most of them, where scans overlap --
//           costs no atomic.  That load may be stale; values only grow, so a stale value is a lower one and at worst the atomic is
//           issued where it was not needed.
//   bytes   the same lanes again, in a launch of its own (the maxima are complete): g8 = (uint8_t)(int)(100 * cell), the form the
//           scoring kernels read.  Lanes that share a cell write the same byte.  Only touched cells are rewritten.
enum { kMgPoints = 0, kMgStamped, kMgDropped, kMgX0, kMgY0, kMgX1, kMgY1, kMgStatSlots };

struct MapGrowArgs {
    const YmScanRef *scans;     // the scans of this launch
    int32_t n_scans, max_n;     // max_n: the longest scan, the stride of `cells`
    int32_t width, height;
    double ox, oy, res;         // world position of cell (0, 0), cell size
    int32_t *cells;             // [n_scans][max_n] gy * width + gx of a stamped reading, -1: no reading or outside the map
    unsigned long long *stats;  // [kMgStatSlots]; X0, Y0 start at the largest value, X1, Y1 (inclusive) and the counts at 0
    const double *kernel;       // [ksize][ksize] the float taps (helpers.py:86-97)
    int32_t ksize, pad;
    double *cgrid;
    uint8_t *g8;
};

// grid (n_scans), 1024 threads
__global__ __launch_bounds__(1024) void map_grow_cells_kernel(MapGrowArgs a) {
    __shared__ unsigned long long s_stat[kMgStatSlots];
    const YmScanRef sr = a.scans[blockIdx.x];
    int32_t *cells = a.cells + (size_t)blockIdx.x * a.max_n;
    const int tid = threadIdx.x;
    if (tid < kMgStatSlots) s_stat[tid] = (tid == kMgX0 || tid == kMgY0) ? ~0ull : 0ull;
    __syncthreads();
    const double px = sr.pose[0], py = sr.pose[1], pt = sr.pose[2];
    unsigned points = 0, stamped = 0;
    int x0 = INT32_MAX, y0 = INT32_MAX, x1 = -1, y1 = -1;
    for (int i = tid; i < a.max_n; i += 1024) {
        int cell = -1;
        if (i < sr.n) {
            const double r = sr.ranges[i];
            if (!(r > sr.range_threshold || isnan(r))) { // _get_point_readings, helpers.py:63
                const double angle = pt + sr.min_angle + i * sr.angle_inc;
                const double x = px + r * cos(angle), y = py + r * sin(angle);
                // a NaN or an infinity fails the comparisons; so does what does not fit an int32 (the map has fewer cells per side)
                const double gx = rint((x - a.ox) / a.res), gy = rint((y - a.oy) / a.res);
                points++;
                if (gx >= 0.0 && gx < (double)a.width && gy >= 0.0 && gy < (double)a.height) {
                    const int cx = (int)gx, cy = (int)gy;
                    cell = cy * a.width + cx; // (below 2^31: a map holds at most 10^9 cells)
                    stamped++;
                    x0 = min(x0, cx); y0 = min(y0, cy); x1 = max(x1, cx); y1 = max(y1, cy);
                }
            }
        }
        cells[i] = cell;
    }
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) {
        points += __shfl_xor(points, d); stamped += __shfl_xor(stamped, d);
        x0 = min(x0, __shfl_xor(x0, d)); y0 = min(y0, __shfl_xor(y0, d));
        x1 = max(x1, __shfl_xor(x1, d)); y1 = max(y1, __shfl_xor(y1, d));
    }
    if ((tid & 63) == 0 && points) {
        atomicAdd(&s_stat[kMgPoints], (unsigned long long)points);
        if (stamped) {
            atomicAdd(&s_stat[kMgStamped], (unsigned long long)stamped);
            atomicMin(&s_stat[kMgX0], (unsigned long long)x0); atomicMin(&s_stat[kMgY0], (unsigned long long)y0);
            atomicMax(&s_stat[kMgX1], (unsigned long long)x1); atomicMax(&s_stat[kMgY1], (unsigned long long)y1);
        }
    }
    __syncthreads();
    if (tid == 0 && s_stat[kMgPoints]) {
        atomicAdd(&a.stats[kMgPoints], s_stat[kMgPoints]);
        atomicAdd(&a.stats[kMgDropped], s_stat[kMgPoints] - s_stat[kMgStamped]);
        if (s_stat[kMgStamped]) {
            atomicAdd(&a.stats[kMgStamped], s_stat[kMgStamped]);
            atomicMin(&a.stats[kMgX0], s_stat[kMgX0]); atomicMin(&a.stats[kMgY0], s_stat[kMgY0]);
            atomicMax(&a.stats[kMgX1], s_stat[kMgX1]); atomicMax(&a.stats[kMgY1], s_stat[kMgY1]);
        }
    }
}

// grid (ceil(max_n * ksize^2 / 256), n_scans), 256 threads.  BYTES = false: the maxima; true: the bytes of the touched cells.
template <bool BYTES>
__global__ __launch_bounds__(256) void map_grow_smear_kernel(MapGrowArgs a) {
    const int kk = a.ksize * a.ksize, half = a.ksize / 2;
    const unsigned idx = blockIdx.x * 256u + threadIdx.x; // (max_n * kk is below 2^31: the host checks)
    const int p = (int)(idx / (unsigned)kk), t = (int)(idx - (unsigned)p * (unsigned)kk);
    if (p >= a.max_n) return;
    const int cell = a.cells[(size_t)blockIdx.y * a.max_n + p];
    if (cell < 0) return;
    const int sy = t / a.ksize, sx = t - sy * a.ksize;
    const int gy = cell / a.width, gx = cell - gy * a.width;
    const int x = gx + (sx - half), y = gy + (sy - half);
    if (x < 0 || x >= a.width || y < 0 || y >= a.height) return; // in_grid_bounds, helpers.py:115
    const size_t c = (size_t)y * a.width + x;
    if (BYTES) {
        a.g8[c] = (uint8_t)(int)(100 * a.cgrid[c]);
    } else {
        double v = a.kernel[t]; // kernel[sy][sx], helpers.py:116
        if (sx == half && sy == half) v = 1.0 > v ? 1.0 : v; // the stamp itself, helpers.py:130
        if (a.cgrid[c] < v)
            atomicMax(reinterpret_cast<unsigned long long *>(a.cgrid) + c, (unsigned long long)__double_as_longlong(v));
    }
}

// both arrays of a map to zero: eight cells per thread, the rest of the last eight one by one.  grid (ceil(n / 2048)), 256 threads
__global__ __launch_bounds__(256) void map_clear_kernel(double *cgrid, uint8_t *g8, size_t n) {
    const size_t i0 = ((size_t)blockIdx.x * 256 + threadIdx.x) * 8;
    if (i0 + 8 <= n) {
        double2 *c = reinterpret_cast<double2 *>(cgrid + i0); // (64-byte aligned: i0 is a multiple of eight)
        const double2 z = make_double2(0.0, 0.0);
        c[0] = z; c[1] = z; c[2] = z; c[3] = z;
        *reinterpret_cast<unsigned long long *>(g8 + i0) = 0ull;
    } else {
        for (size_t i = i0; i < n; i++) { cgrid[i] = 0.0; g8[i] = 0; }
    }
}

}  // namespace ym
