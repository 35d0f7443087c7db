// ym_k_mapgrow.hpp -- a resident correlation map that takes scans: map_grow_cells_kernel, map_grow_smear_kernel, map_clear_kernel;
// one that lets them go again: map_count_kernel, map_forget_mark_kernel, map_forget_gather_kernel;
// and one whose window moves: map_reframe_copy_kernel, map_reframe_mark_kernel.
// Part of ym_kernels.hpp (include that, not this file).  DESIGN.md sections 15, 16 and 17.
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
enum { kMgPoints = 0, kMgStamped, kMgDropped, kMgX0, kMgY0, kMgX1, kMgY1, kMgOverlap, kMgStatSlots };

struct MapGrowArgs {
    const YmScanRef *scans;     // the scans of this launch
    int32_t n_scans, max_n;     // max_n: the longest scan, the stride of `cells`
    int32_t width, height;
    double ox, oy, res;         // world position of lattice cell (0, 0) -- the map's anchor --, cell size
    int32_t wx0, wy0;           // the map's cell (0, 0) is lattice cell (wx0, wy0): 0, 0 unless the map was reframed (section 17)
    int32_t ex0, ey0, ex1, ey1; // ym_map_reframe: readings in the cells [ex0, ex1) x [ey0, ey1) are counted in kMgOverlap and yield -1
                                // (their counts were copied); empty -- ex1 <= ex0 -- for every other caller
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
    unsigned points = 0, stamped = 0, overlap = 0;
    int x0 = INT32_MAX, y0 = INT32_MAX, x1 = -1, y1 = -1;
    for (int i = tid; i < a.max_n; i += 1024) {
        int cell = -1;
        if (i < sr.n) {
            const double r = sr.ranges[i];
            if (!(r > sr.range_threshold || isnan(r))) { // _get_point_readings, helpers.py:63
                const double angle = pt + sr.min_angle + i * sr.angle_inc;
                const double x = px + r * cos(angle), y = py + r * sin(angle);
                // a NaN or an infinity fails the comparisons; so does what does not fit an int32 (the map has fewer cells per side)
                // the cell in the anchor's lattice, then the window's integer offset: exact in fp64 (|offset| <= 2^30), so a reading
                // has the same lattice cell wherever the window lies
                const double gx = rint((x - a.ox) / a.res) - (double)a.wx0, gy = rint((y - a.oy) / a.res) - (double)a.wy0;
                points++;
                if (gx >= 0.0 && gx < (double)a.width && gy >= 0.0 && gy < (double)a.height) {
                    const int cx = (int)gx, cy = (int)gy;
                    if (cx >= a.ex0 && cx < a.ex1 && cy >= a.ey0 && cy < a.ey1) {
                        overlap++;
                    } else {
                        cell = cy * a.width + cx; // (below 2^31: a map holds at most 10^9 cells)
                        stamped++;
                        x0 = min(x0, cx); y0 = min(y0, cy); x1 = max(x1, cx); y1 = max(y1, cy);
                    }
                }
            }
        }
        cells[i] = cell;
    }
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) {
        points += __shfl_xor(points, d); stamped += __shfl_xor(stamped, d); overlap += __shfl_xor(overlap, d);
        x0 = min(x0, __shfl_xor(x0, d)); y0 = min(y0, __shfl_xor(y0, d));
        x1 = max(x1, __shfl_xor(x1, d)); y1 = max(y1, __shfl_xor(y1, d));
    }
    if ((tid & 63) == 0 && points) {
        atomicAdd(&s_stat[kMgPoints], (unsigned long long)points);
        if (overlap) atomicAdd(&s_stat[kMgOverlap], (unsigned long long)overlap);
        if (stamped) {
            atomicAdd(&s_stat[kMgStamped], (unsigned long long)stamped);
            atomicMin(&s_stat[kMgX0], (unsigned long long)x0); atomicMin(&s_stat[kMgY0], (unsigned long long)y0);
            atomicMax(&s_stat[kMgX1], (unsigned long long)x1); atomicMax(&s_stat[kMgY1], (unsigned long long)y1);
        }
    }
    __syncthreads();
    if (tid == 0 && s_stat[kMgPoints]) {
        atomicAdd(&a.stats[kMgPoints], s_stat[kMgPoints]);
        atomicAdd(&a.stats[kMgDropped], s_stat[kMgPoints] - s_stat[kMgStamped] - s_stat[kMgOverlap]);
        if (s_stat[kMgOverlap]) atomicAdd(&a.stats[kMgOverlap], s_stat[kMgOverlap]);
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

// ---- counted maps: a map that can forget
// A counted map keeps stamps[height][width], the number of readings stamped in each cell, and the invariant that cgrid and g8 are what
// map_from_occupancy_kernel makes of the image stamps > 0.  Adding keeps it as above (the smear is that kernel's scatter form, section 15).
// Removing takes the counts down and then recomputes, by that kernel's gather, exactly the cells within reach of a cell whose count fell
// to zero:
//   count   one lane per beam, on the cells map_grow_cells_kernel left.  REMOVE: an atomic subtraction; a reading that meets a
//           count of zero puts its one back and is counted as unmatched (the caller named a pose the scan was not added at); the lane
//           that takes a count to zero appends the cell to `released` and widens the released box.  Removes of a call run before its adds,
//           so a count reaches zero at most once per call and `released` holds no cell twice.  Add: an atomic add; a cell whose count
//           was already positive has its taps in the map (the invariant, or the lane of this launch that found zero), so its entry in
//           `cells` is struck out and the smear skips it.
//   mark    one lane per (released cell, tap): the byte dirty[target] = 1 (lanes that share a target store the same value)
//   gather  64 x 4 tiles over the released box widened by the taps' reach.  A tile without a dirty cell leaves; the others stage
//           stamps > 0 of the tile and its halo in LDS, and every dirty cell takes the maximum of kernel[sy][sx] over the stamped cells
//           that reach it -- map_from_occupancy_kernel's loop on the same table --, writes both forms and clears its flag.
//           It runs after the smear of the same call: the counts it reads hold what that call added.
enum { kMuUnmatched = 0, kMuReleased, kMuGained, kMuX0, kMuY0, kMuX1, kMuY1, kMuStatSlots };
enum { kMfTileW = 64, kMfTileH = 4 };

struct MapForgetArgs {
    int32_t *cells;             // [n_scans][max_n] what map_grow_cells_kernel wrote
    int32_t max_n;
    int32_t width, height;
    uint32_t *stamps;           // [height][width] readings stamped per cell
    int32_t *released;          // cells whose count fell to zero in this call; stats[kMuReleased] is its cursor
    unsigned long long *stats;  // [kMuStatSlots]; X0, Y0 start at the largest value, the rest at 0
    uint8_t *dirty;             // [height][width] 1: within reach of a released cell
    const double *kernel;       // [ksize][ksize]
    int32_t ksize;
    int32_t first, count;       // mark: released[first .. first + count)
    int32_t bx0, by0, bx1, by1; // gather: the cells [bx0, bx1) x [by0, by1); bx0, by0 multiples of the tile
    double *cgrid;
    uint8_t *g8;
};

// grid (ceil(max_n / 256), n_scans), 256 threads
template <bool REMOVE>
__global__ __launch_bounds__(256) void map_count_kernel(MapForgetArgs a) {
    const int p = blockIdx.x * 256 + threadIdx.x;
    int32_t *slot = a.cells + (size_t)blockIdx.y * a.max_n + p;
    const int cell = p < a.max_n ? *slot : -1;
    const int lane = threadIdx.x & 63;
    if (REMOVE) {
        bool unmatched = false, released = false;
        if (cell >= 0) {
            // One hardware atomic per reading: a compare-and-swap loop took 110 ms to move 2000 scans of a hall at 0.05 m, where
            // hundreds of readings share a cell, and this form 3.7 ms (profiles/map_forget_time.json).  Read as an int32, the count a decrement finds is positive
            // exactly as often as the cell held readings: the decrements that find less put their one back, so the value never exceeds
            // what is truly left, and the first of them comes only when nothing is left.  Exactly one decrement finds 1.
            const int old = (int)atomicSub(&a.stamps[cell], 1u);
            if (old <= 0) { atomicAdd(&a.stamps[cell], 1u); unmatched = true; }
            released = old == 1;
        }
        const unsigned long long mu = __ballot(unmatched), mr = __ballot(released);
        int x0 = INT32_MAX, y0 = INT32_MAX, x1 = -1, y1 = -1;
        if (released) { y0 = y1 = cell / a.width; x0 = x1 = cell - y0 * a.width; }
#pragma unroll
        for (int d = 32; d >= 1; d >>= 1) {
            x0 = min(x0, __shfl_xor(x0, d)); y0 = min(y0, __shfl_xor(y0, d));
            x1 = max(x1, __shfl_xor(x1, d)); y1 = max(y1, __shfl_xor(y1, d));
        }
        unsigned long long base = 0;
        if (lane == 0) {
            if (mu) atomicAdd(&a.stats[kMuUnmatched], (unsigned long long)__popcll(mu));
            if (mr) {
                base = atomicAdd(&a.stats[kMuReleased], (unsigned long long)__popcll(mr));
                atomicMin(&a.stats[kMuX0], (unsigned long long)x0); atomicMin(&a.stats[kMuY0], (unsigned long long)y0);
                atomicMax(&a.stats[kMuX1], (unsigned long long)x1); atomicMax(&a.stats[kMuY1], (unsigned long long)y1);
            }
        }
        base = __shfl(base, 0);
        // (the list has room for every cell of the map, and no cell is released twice in a call)
        if (released) a.released[base + (unsigned long long)__popcll(mr & ((1ull << lane) - 1ull))] = cell;
    } else {
        bool gained = false;
        if (cell >= 0) {
            gained = atomicAdd(&a.stamps[cell], 1u) == 0u; // (2^32 readings in one cell are out of reach: a call holds fewer)
            if (!gained) *slot = -1;
        }
        const unsigned long long mg = __ballot(gained);
        if (lane == 0 && mg) atomicAdd(&a.stats[kMuGained], (unsigned long long)__popcll(mg));
    }
}

// grid (ceil(count * ksize^2 / 256)), 256 threads (count * ksize^2 is below 2^31: the host cuts the list)
__global__ __launch_bounds__(256) void map_forget_mark_kernel(MapForgetArgs a) {
    const int kk = a.ksize * a.ksize, half = a.ksize / 2;
    const unsigned idx = blockIdx.x * 256u + threadIdx.x;
    const int r = (int)(idx / (unsigned)kk), t = (int)(idx - (unsigned)r * (unsigned)kk);
    if (r >= a.count) return;
    const int cell = a.released[(size_t)a.first + r];
    const int sy = t / a.ksize, sx = t - sy * a.ksize;
    const int gy = cell / a.width, gx = cell - gy * a.width;
    const int x = gx + (sx - half), y = gy + (sy - half);
    if (x < 0 || x >= a.width || y < 0 || y >= a.height) return;
    a.dirty[(size_t)y * a.width + x] = 1;
}

// grid (ceil((bx1 - bx0) / 64), ceil((by1 - by0) / 4)), 256 threads, (64 + ksize - 1) * (4 + ksize - 1) bytes of dynamic LDS
__global__ __launch_bounds__(256) void map_forget_gather_kernel(MapForgetArgs a) {
    extern __shared__ uint8_t s_occ[]; // [4 + 2 half][64 + 2 half] stamps > 0, zero outside the map
    const int half = a.ksize / 2, tw = kMfTileW + 2 * half, th = kMfTileH + 2 * half;
    const int tx = threadIdx.x & 63, ty = threadIdx.x >> 6;
    const int x = a.bx0 + blockIdx.x * kMfTileW + tx, y = a.by0 + blockIdx.y * kMfTileH + ty;
    const size_t c = (size_t)y * a.width + x;
    const bool dirty = x < a.bx1 && y < a.by1 && a.dirty[c] != 0; // (bx1 <= width, by1 <= height)
    if (!__syncthreads_or(dirty)) return;
    const int hx0 = x - tx - half, hy0 = y - ty - half;
    for (int i = threadIdx.x; i < tw * th; i += 256) {
        const int ly = i / tw, lx = i - ly * tw;
        const int gx = hx0 + lx, gy = hy0 + ly;
        s_occ[i] = (gx >= 0 && gx < a.width && gy >= 0 && gy < a.height && a.stamps[(size_t)gy * a.width + gx] > 0u) ? 1 : 0;
    }
    __syncthreads();
    if (!dirty) return;
    const uint8_t *centre = s_occ + (ty + half) * tw + (tx + half);
    double v = 0.0;
    for (int sy = 0; sy < a.ksize; sy++) {
        const uint8_t *row = centre - (sy - half) * tw; // the stamped points that reach (x, y) through the taps of row sy
        for (int sx = 0; sx < a.ksize; sx++) {
            if (row[-(sx - half)]) {
                const double cand = a.kernel[sy * a.ksize + sx];
                v = cand > v ? cand : v;
            }
        }
    }
    if (*centre) v = 1.0 > v ? 1.0 : v;
    a.cgrid[c] = v;
    a.g8[c] = (uint8_t)(int)(100 * v);
    a.dirty[c] = 0;
}

// ---- maps whose window moves
// ym_map_reframe builds the map of a new window in new arrays: new cell (i, j) is old cell (i + dx, j + dy).
//   copy    one pass over the new window, four consecutive cells per thread: grid, bytes and counts come from the old arrays inside
//           the overlap and are zero elsewhere, the dirty flags are zero.  The destination is written in aligned pieces (two double2,
//           one uint4, two 32-bit words: the group starts at a multiple of four cells); the source row is shifted by dx and is read cell
//           by cell -- consecutive lanes read consecutive groups, so a wave still reads contiguous memory.  The copied counts are
//           summed: per wave by shuffles, per block in LDS, one 64-bit atomic per block.
//   restamp map_grow_cells_kernel with the old window as its exclusion rectangle, map_count_kernel<false> and the two smear launches
//           on the held scans: what the old window dropped and the new one holds is stamped now.
//   mark    a cell's copied value stands only if its tap neighbourhood meets both windows in the same cells.  Of the others, a new
//           cell out of reach of the overlap is completed by the restamp's scatter (every stamped cell that reaches it is new); the
//           rest -- all of them within the taps' reach of the overlap -- are flagged here and recomputed by map_forget_gather_kernel
//           from the new window's counts.
struct MapReframeArgs {
    const double *src_cgrid; const uint8_t *src_g8; const uint32_t *src_stamps; // the old window (src_stamps: counted maps)
    int32_t src_w, src_h;
    int32_t dx, dy;             // new cell (i, j) = old cell (i + dx, j + dy)
    int32_t width, height;      // the new window
    double *cgrid; uint8_t *g8; uint32_t *stamps; uint8_t *dirty; // the new arrays (stamps, dirty: counted maps)
    unsigned long long *stats;  // [0] the sum of the copied counts, [1] the cells marked dirty
    int32_t mx0, my0, mx1, my1; // mark: the cells [mx0, mx1) x [my0, my1) of the new window, the overlap widened by the taps' reach
    int32_t half;
};

// grid (ceil(width * height / 1024)), 256 threads
template <bool COUNTED>
__global__ __launch_bounds__(256) void map_reframe_copy_kernel(MapReframeArgs a) {
    __shared__ unsigned long long s_sum;
    if (threadIdx.x == 0) s_sum = 0ull;
    __syncthreads();
    const size_t n = (size_t)a.width * a.height;
    const size_t i0 = ((size_t)blockIdx.x * 256 + threadIdx.x) * 4;
    unsigned long long sum = 0ull;
    if (i0 < n) {
        int y = (int)(i0 / (size_t)a.width), x = (int)(i0 - (size_t)y * a.width);
        double v[4];
        uint32_t b[4], s[4];
#pragma unroll
        for (int k = 0; k < 4; k++) {
            const int sx = x + a.dx, sy = y + a.dy;
            v[k] = 0.0; b[k] = 0u; s[k] = 0u;
            // (y may pass the last row in the last group: those entries are not stored)
            if (sx >= 0 && sx < a.src_w && sy >= 0 && sy < a.src_h && y < a.height) {
                const size_t c = (size_t)sy * a.src_w + sx;
                v[k] = a.src_cgrid[c]; b[k] = a.src_g8[c];
                if (COUNTED) { s[k] = a.src_stamps[c]; sum += s[k]; }
            }
            if (++x == a.width) { x = 0; y++; }
        }
        if (i0 + 4 <= n) { // (cgrid + i0: 32-byte aligned, stamps + i0: 16, g8 + i0 and dirty + i0: 4)
            double2 *d = reinterpret_cast<double2 *>(a.cgrid + i0);
            d[0] = make_double2(v[0], v[1]); d[1] = make_double2(v[2], v[3]);
            *reinterpret_cast<uint32_t *>(a.g8 + i0) = b[0] | (b[1] << 8) | (b[2] << 16) | (b[3] << 24);
            if (COUNTED) {
                *reinterpret_cast<uint4 *>(a.stamps + i0) = make_uint4(s[0], s[1], s[2], s[3]);
                *reinterpret_cast<uint32_t *>(a.dirty + i0) = 0u;
            }
        } else {
            for (int k = 0; i0 + k < n; k++) {
                a.cgrid[i0 + k] = v[k]; a.g8[i0 + k] = (uint8_t)b[k];
                if (COUNTED) { a.stamps[i0 + k] = s[k]; a.dirty[i0 + k] = 0; }
            }
        }
    }
    if (COUNTED) {
        unsigned lo = (unsigned)sum, hi = (unsigned)(sum >> 32);
#pragma unroll
        for (int d = 32; d >= 1; d >>= 1) { // (the 64-bit sum travels as its two halves)
            const unsigned long long o = ((unsigned long long)__shfl_xor(hi, d) << 32) | __shfl_xor(lo, d);
            sum += o;
            lo = (unsigned)sum; hi = (unsigned)(sum >> 32);
        }
        if ((threadIdx.x & 63) == 0 && sum) atomicAdd(&s_sum, sum);
        __syncthreads();
        if (threadIdx.x == 0 && s_sum) atomicAdd(&a.stats[0], s_sum);
    }
}

// grid (ceil((mx1 - mx0) / 256), my1 - my0 in pieces of 65535), 256 threads; a.my0 is the first row of the piece
__global__ __launch_bounds__(256) void map_reframe_mark_kernel(MapReframeArgs a) {
    const int x = a.mx0 + blockIdx.x * 256 + threadIdx.x, y = a.my0 + blockIdx.y;
    bool mark = false;
    if (x < a.mx1 && y < a.my1) {
        // the neighbourhood [x - half, x + half] x [y - half, y + half] cut to the new window and to the old one (in new cells)
        const int nx0 = x - a.half, nx1 = x + a.half + 1, ny0 = y - a.half, ny1 = y + a.half + 1;
        const int ax0 = max(nx0, 0), ax1 = min(nx1, a.width), ay0 = max(ny0, 0), ay1 = min(ny1, a.height);
        const int bx0 = max(nx0, -a.dx), bx1 = min(nx1, a.src_w - a.dx), by0 = max(ny0, -a.dy), by1 = min(ny1, a.src_h - a.dy);
        const bool old_empty = bx1 <= bx0 || by1 <= by0; // (the new cut holds (x, y) itself)
        mark = old_empty || ax0 != bx0 || ax1 != bx1 || ay0 != by0 || ay1 != by1;
        if (mark) a.dirty[(size_t)y * a.width + x] = 1;
    }
    const int cnt = __syncthreads_count(mark);
    if (threadIdx.x == 0 && cnt) atomicAdd(&a.stats[1], (unsigned long long)cnt);
}

}  // namespace ym
