// ym_k_seenthrough.hpp -- which held readings does a newer scan look straight through: seen_sweep_kernel, seen_protect_kernel,
// seen_count_kernel.  Part of ym_kernels.hpp (include that, not this file).  DESIGN.md section 19; tests/seenthrough_ref.py restates it.
#pragma once

namespace ym {

// The evidence a counted map needs to notice that the world changed.  A viewer scan's ray from its sensor cell to a reading's cell
// sweeps the cells it crosses more than `clearance` cells before its end; a cell within `protect` cells (Chebyshev) of any viewer
// reading's end cell is never swept; a held reading whose cell is swept was seen through.  Three stages over a byte mask [h][w] the
// host zeroed, each a launch of its own, so a stage reads only what the launch before it completed:
//   sweep    a wave per viewer ray.  The ray's cells are Grid::TraceLine's (occ_trace_wave_kernel's closed form: after k major steps
//            the minor coordinate has moved floor((2 k dm + dM) / (2 dM)) cells); the lanes take k = k0 + lane, + 64, ... of the part
//            of the walk whose major coordinate lies in the window.  A swept cell gets a plain byte store of 1: lanes and waves that
//            share a cell store the same value.
//   protect  one lane per (viewer reading, cell of its (2 protect + 1)^2 neighbourhood): a plain byte store of 0.
//   count    the held scans' cells come from map_grow_cells_kernel at the poses they were added at (the cell rule stays stated once
//            for everything the map holds); a block per held scan reads the mask there, writes the optional flags and makes one plain
//            store of (inside, seen).
// No atomics, no LDS beyond the block reductions' few words, no block waits on another.
struct SeenArgs {
    const YmScanRef *scans;     // sweep, protect: the viewers of this launch
    int32_t max_n;              // the longest scan of the list the launch reads: the stride of `cells` and `flags`
    int32_t width, height;
    double ox, oy, res;         // the map's anchor and cell size
    int32_t wx0, wy0;           // the window's offset in the anchor's lattice
    int32_t clearance, protect;
    uint8_t *mask;              // [height][width] 1: swept
    int32_t *walked;            // sweep: [n_viewers][gridDim.x] the rays each block walked
    const int32_t *cells;       // count: [n_scans][max_n] what map_grow_cells_kernel wrote
    int32_t *counts;            // count: [n_scans][2] inside, seen
    uint8_t *flags;             // count: null or [n_scans][max_n] 1: the reading was seen through
};

// The lattice cell of world coordinate x minus the window's offset: map_grow_cells_kernel's quotient and rounding, without the cut to
// the window.  False: the quotient is not finite or does not fit an int32.  (|w0| <= 2^30: the difference is exact in fp64 and fits
// 64 bits with room to spare.)
__device__ __forceinline__ bool seen_coord(double x, double o, double res, int w0, long long &c) {
    const double q = rint((x - o) / res);
    if (!(q > -2147483648.0 && q < 2147483648.0)) return false;
    c = (long long)(q - (double)w0);
    return true;
}

// the end cell of beam i of a viewer, by _get_point_readings' rule and project_points' expressions (map_grow_cells_kernel's)
__device__ __forceinline__ bool seen_end_cell(const YmScanRef &sr, int i, const SeenArgs &a, long long &cx, long long &cy) {
    const double r = sr.ranges[i];
    if (r > sr.range_threshold || isnan(r)) return false;
    const double angle = sr.pose[2] + sr.min_angle + i * sr.angle_inc;
    const double x = sr.pose[0] + r * cos(angle), y = sr.pose[1] + r * sin(angle);
    return seen_coord(x, a.ox, a.res, a.wx0, cx) && seen_coord(y, a.oy, a.res, a.wy0, cy);
}

enum { kSeenRaysPerWave = 4, kSeenRaysPerBlock = 4 * kSeenRaysPerWave };

// grid (ceil(max_n / 16), n_viewers), 256 threads: four waves, four consecutive rays each
__global__ __launch_bounds__(256) void seen_sweep_kernel(SeenArgs a) {
    __shared__ int s_walked[4];
    const YmScanRef sr = a.scans[blockIdx.y];
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    long long sx, sy;
    const bool sensor = seen_coord(sr.pose[0], a.ox, a.res, a.wx0, sx) && seen_coord(sr.pose[1], a.oy, a.res, a.wy0, sy);
    int walked = 0;
    const int first = blockIdx.x * kSeenRaysPerBlock + wave * kSeenRaysPerWave;
    for (int i = first; i < first + kSeenRaysPerWave && i < sr.n && sensor; i++) {
        long long x0 = sx, y0 = sy, x1, y1;
        if (!seen_end_cell(sr, i, a, x1, y1)) continue;
        walked++;
        const long long adx = x1 > x0 ? x1 - x0 : x0 - x1, ady = y1 > y0 ? y1 - y0 : y0 - y1;
        const bool steep = ady > adx;
        if (steep) { long long t = x0; x0 = y0; y0 = t; t = x1; x1 = y1; y1 = t; }
        const bool from_end = x0 > x1; // the walk starts at the reading's cell: a cell's distance to the end is k, else dM - k
        if (from_end) { long long t = x0; x0 = x1; x1 = t; t = y0; y0 = y1; y1 = t; }
        const long long dM = x1 - x0, dm = y1 > y0 ? y1 - y0 : y0 - y1;
        const bool up = y0 < y1;
        // the steps whose major coordinate lies in the window and whose distance to the end exceeds the clearance
        const long long major_n = steep ? a.height : a.width, minor_n = steep ? a.width : a.height;
        long long k_lo = x0 < 0 ? -x0 : 0, k_hi = dM < major_n - 1 - x0 ? dM : major_n - 1 - x0;
        if (from_end) k_lo = k_lo > (long long)a.clearance + 1 ? k_lo : (long long)a.clearance + 1;
        else k_hi = k_hi < dM - 1 - (long long)a.clearance ? k_hi : dM - 1 - (long long)a.clearance;
        // 2 k dm + dM < 2^31 while dM < 2^15: every ray of a matcher the host admits.  A longer one comes only from a reading no sensor
        // gives (a large negative range passes _get_point_readings' rule) and sweeps nothing: the rule says so.
        if (dM >= 32768) continue;
        const unsigned dm2 = 2u * (unsigned)dm, uM = (unsigned)dM, uM2 = 2u * uM;
        for (long long k = k_lo + lane; k <= k_hi; k += 64) { // (k_lo <= k_hi only where dM >= 1)
            const long long m = (long long)(((unsigned)k * dm2 + uM) / uM2);
            const long long major = x0 + k, minor = up ? y0 + m : y0 - m;
            if (minor >= 0 && minor < minor_n) a.mask[steep ? (size_t)major * a.width + (size_t)minor : (size_t)minor * a.width + (size_t)major] = 1;
        }
    }
    if (lane == 0) s_walked[wave] = walked;
    __syncthreads();
    if (threadIdx.x == 0) a.walked[(size_t)blockIdx.y * gridDim.x + blockIdx.x] = s_walked[0] + s_walked[1] + s_walked[2] + s_walked[3];
}

// grid (ceil(max_n * (2 protect + 1)^2 / 256), n_viewers), 256 threads (the product is below 2^31: the host checks)
__global__ __launch_bounds__(256) void seen_protect_kernel(SeenArgs a) {
    const YmScanRef sr = a.scans[blockIdx.y];
    const int side = 2 * a.protect + 1, nn = side * side;
    const unsigned idx = blockIdx.x * 256u + threadIdx.x;
    const int i = (int)(idx / (unsigned)nn), t = (int)(idx - (unsigned)i * (unsigned)nn);
    if (i >= sr.n) return;
    long long cx, cy;
    if (!seen_end_cell(sr, i, a, cx, cy)) return;
    const int ty = t / side, tx = t - ty * side;
    const long long x = cx + (tx - a.protect), y = cy + (ty - a.protect);
    if (x < 0 || x >= a.width || y < 0 || y >= a.height) return;
    a.mask[(size_t)y * a.width + (size_t)x] = 0;
}

// grid (n_scans), 256 threads
__global__ __launch_bounds__(256) void seen_count_kernel(SeenArgs a) {
    __shared__ int s_part[2][4];
    const int32_t *cells = a.cells + (size_t)blockIdx.x * a.max_n;
    uint8_t *flags = a.flags ? a.flags + (size_t)blockIdx.x * a.max_n : nullptr;
    int inside = 0, seen = 0;
    for (int i = threadIdx.x; i < a.max_n; i += 256) {
        const int cell = cells[i]; // (-1 beyond the scan's last beam too)
        const uint8_t f = cell >= 0 ? a.mask[cell] : 0;
        inside += cell >= 0;
        seen += f;
        if (flags) flags[i] = f;
    }
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) { inside += __shfl_xor(inside, d); seen += __shfl_xor(seen, d); }
    if ((threadIdx.x & 63) == 0) { s_part[0][threadIdx.x >> 6] = inside; s_part[1][threadIdx.x >> 6] = seen; }
    __syncthreads();
    if (threadIdx.x == 0) {
        int2 out;
        out.x = s_part[0][0] + s_part[0][1] + s_part[0][2] + s_part[0][3];
        out.y = s_part[1][0] + s_part[1][1] + s_part[1][2] + s_part[1][3];
        *reinterpret_cast<int2 *>(a.counts + 2 * (size_t)blockIdx.x) = out;
    }
}

}  // namespace ym
