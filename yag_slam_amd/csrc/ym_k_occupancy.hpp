// ym_k_occupancy.hpp -- occupancy-grid rendering: the other native call of yag-slam's loop,
// karto_scanmatcher.create_occupancy_grid(scans, resolution, range_threshold) (/root/reference/yag_slam/graph_slam.py:341-342,
// /root/reference/ros1/slam_node_ros1:187-202).  The wheel's source is not in /root/reference: this restates open_karto's
// OccupancyGrid::{CreateFromScans, ComputeDimensions, AddScan, RayTrace, Update, UpdateCell}, Grid<T>::TraceLine and
// LocalizedRangeScan::Update (bounding box); image codes as slam_node_ros1:199-202 reads them (0 occupied, 200 unknown,
// 255 free).  PARITY UNPINNED, like every Karto-side piece.
//
// The same kernels serve the full renderer (occupancy_render) and the live occupancy grid, whose pass and
// hit counts stay on the device and are changed by exactly the rays that changed.  Cells are those of the lattice of an ANCHOR:
// a world coordinate's cell is kt_round_int((p - anchor) * scale), and the origin of the memory is subtracted from that
// integer.  (Folding the origin into the offset would round differently: (p - (anchor + k * res)) * scale is not
// (p - anchor) * scale - k in fp64.)  Counts are unsigned and a removal adds 0xFFFFFFFF: wrap-around makes it exact.  The full
// renderer is the case anchor = the bounding box's minimum, origin (0, 0), pitch = width, sign = 1, window = all the memory.
// Part of ym_kernels.hpp (include that, not this file).
#pragma once

namespace ym {

struct OccArgs {
    const YmScanRef *scans;    // readings + the pose each scan is traced at; the laser's MAXIMUM range travels in range_threshold (scan_ref)
    int32_t n_scans, max_n;
    double range_threshold;    // create_occupancy_grid's third argument: the laser's range threshold for this rendering
    double scale, anchor_x, anchor_y; // CoordinateConverter of the lattice (scale = 1 / resolution, offset = the anchor)
    int32_t org_x, org_y;      // lattice cell of the memory's cell (0, 0)
    int32_t width, height;     // cells that have memory; rows are `pitch` cells apart
    int64_t pitch;
    unsigned *pass, *hits;
    unsigned sign;             // 1 or 0xFFFFFFFF
    int32_t *reach;            // [n_scans][4] lattice cells xmin, ymin, xmax, ymax (occ_reach_kernel)
    // occ_update_kernel: the window inside the memory, and the dense image it fills
    int32_t win_x, win_y, win_w, win_h;
    uint8_t *image;            // [win_h][win_w]
    double *boxes;             // [n_scans][4] xmin, ymin, xmax, ymax of every scan's bounding box (occ_bbox_kernel)
};

// LocalizedRangeScan::Update: the bounding box holds the sensor position and every point reading with
// minimum range <= r <= range threshold.  grid (n_scans), 256 threads
__global__ __launch_bounds__(256) void occ_bbox_kernel(OccArgs a) {
    __shared__ double scratch[16];
    const YmScanRef sr = a.scans[blockIdx.x];
    double x0 = sr.pose[0], y0 = sr.pose[1], x1 = sr.pose[0], y1 = sr.pose[1];
    for (int i = threadIdx.x; i < sr.n; i += 256) {
        const double r = sr.ranges[i];
        if (!(r >= sr.min_range && r <= a.range_threshold)) continue;
        const double angle = sr.pose[2] + sr.min_angle + i * sr.angle_inc;
        const double px = sr.pose[0] + r * cos(angle), py = sr.pose[1] + r * sin(angle);
        x0 = px < x0 ? px : x0; x1 = px > x1 ? px : x1;
        y0 = py < y0 ? py : y0; y1 = py > y1 ? py : y1;
    }
    struct OpMinD { __device__ double operator()(double p, double q) const { return p < q ? p : q; } };
    x0 = block_reduce(x0, OpMinD(), 1e300, scratch);
    y0 = block_reduce(y0, OpMinD(), 1e300, scratch);
    x1 = block_reduce(x1, OpMaxD(), -1e300, scratch);
    y1 = block_reduce(y1, OpMaxD(), -1e300, scratch);
    if (threadIdx.x == 0) {
        double *b = a.boxes + 4 * (size_t)blockIdx.x;
        b[0] = x0; b[1] = y0; b[2] = x1; b[3] = y1;
    }
}

// OccupancyGrid::AddScan + RayTrace: beam i of a scan as a ray between two lattice cells; false: the reading is not traced
__device__ __forceinline__ bool occ_ray(const YmScanRef &sr, int i, const OccArgs &a, int &x0, int &y0, int &x1, int &y1, bool &end_valid) {
    const double r = sr.ranges[i];
    // AddScan: readings at or below the minimum range, at or beyond the maximum range, or NaN are ignored
    if (r <= sr.min_range || r >= sr.range_threshold /* max_range travels in this field here */ || isnan(r)) return false;
    end_valid = r < (a.range_threshold - YM_KT_TOLERANCE);
    const double angle = sr.pose[2] + sr.min_angle + i * sr.angle_inc;
    double px = sr.pose[0] + r * cos(angle), py = sr.pose[1] + r * sin(angle);
    if (r >= a.range_threshold) { // trace up to the range threshold only
        const double ratio = a.range_threshold / r;
        const double dx = px - sr.pose[0], dy = py - sr.pose[1];
        px = sr.pose[0] + ratio * dx;
        py = sr.pose[1] + ratio * dy;
    }
    x0 = world_to_grid(sr.pose[0], a.anchor_x, a.scale); y0 = world_to_grid(sr.pose[1], a.anchor_y, a.scale);
    x1 = world_to_grid(px, a.anchor_x, a.scale); y1 = world_to_grid(py, a.anchor_y, a.scale);
    return true;
}

// The lattice cells a scan's rays can touch: a line's cells lie in the box of its two end cells.  Unlike the bounding box of
// occ_bbox_kernel this holds the ends of the rays clipped at the threshold.  grid (n_scans), 256 threads
__global__ __launch_bounds__(256) void occ_reach_kernel(OccArgs a) {
    __shared__ int scratch[16];
    const YmScanRef sr = a.scans[blockIdx.x];
    int bx0 = world_to_grid(sr.pose[0], a.anchor_x, a.scale), by0 = world_to_grid(sr.pose[1], a.anchor_y, a.scale);
    int bx1 = bx0, by1 = by0;
    for (int i = threadIdx.x; i < sr.n; i += 256) {
        int x0, y0, x1, y1;
        bool valid;
        if (!occ_ray(sr, i, a, x0, y0, x1, y1, valid)) continue;
        bx0 = x1 < bx0 ? x1 : bx0; bx1 = x1 > bx1 ? x1 : bx1;
        by0 = y1 < by0 ? y1 : by0; by1 = y1 > by1 ? y1 : by1;
    }
    bx0 = block_reduce(bx0, OpMinI(), INT32_MAX, scratch);
    by0 = block_reduce(by0, OpMinI(), INT32_MAX, scratch);
    bx1 = block_reduce(bx1, OpMaxI(), INT32_MIN, scratch);
    by1 = block_reduce(by1, OpMaxI(), INT32_MIN, scratch);
    if (threadIdx.x == 0) {
        int32_t *b = a.reach + 4 * (size_t)blockIdx.x;
        b[0] = bx0; b[1] = by0; b[2] = bx1; b[3] = by1;
    }
}

__device__ __forceinline__ void occ_count(const OccArgs &a, unsigned *plane, int lx, int ly) {
    const int cx = lx - a.org_x, cy = ly - a.org_y;
    if (cx >= 0 && cx < a.width && cy >= 0 && cy < a.height) atomicAdd(&plane[(size_t)cy * (size_t)a.pitch + cx], a.sign);
}

// Grid<T>::TraceLine (Bresenham, both end cells included), one thread per beam with the running error: the full renderer's form,
// and the live grid's behind ym_occmap_debug_option 1 = 1.  Pass and hit counts are sums, so the order the rays are traced in does
// not matter.  grid (ceil(max_n / 256), n_scans), 256 threads
__global__ __launch_bounds__(256) void occ_trace_thread_kernel(OccArgs a) {
    const YmScanRef sr = a.scans[blockIdx.y];
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= sr.n) return;
    int x0, y0, x1, y1;
    bool end_valid;
    if (!occ_ray(sr, i, a, x0, y0, x1, y1, end_valid)) return;
    const int tx = x1, ty = y1;
    const bool steep = abs(y1 - y0) > abs(x1 - x0);
    if (steep) { int t = x0; x0 = y0; y0 = t; t = x1; x1 = y1; y1 = t; }
    if (x0 > x1) { int t = x0; x0 = x1; x1 = t; t = y0; y0 = y1; y1 = t; }
    const int delta_x = x1 - x0, delta_y = abs(y1 - y0);
    int error = 0, y = y0;
    const int ystep = y0 < y1 ? 1 : -1;
    for (int x = x0; x <= x1; x++) {
        occ_count(a, a.pass, steep ? y : x, steep ? x : y);
        error += delta_y;
        if (2 * error >= delta_x) { y += ystep; error -= delta_x; }
    }
    // RayTrace: a valid end point counts once more as a pass, and as a hit
    if (end_valid) {
        occ_count(a, a.pass, tx, ty);
        occ_count(a, a.hits, tx, ty);
    }
}

// The live grid's default form.  A publish is a few scans, too few rays for a thread each: a wave owns a ray, its lanes take the
// cells k = lane, lane + 64, ... of the walk.  After k major steps the minor coordinate has
// moved m(k) = floor((2 k dm + dM) / (2 dM)) cells (tests/occupancy_ref.py states it; Grid::TraceLine's running error, closed).
// k <= dM and dm <= dM, and the host admits only range_threshold * scale < 2^24 cells, so 2 k dm + dM < 2^50: 64-bit integers hold it,
// and 32-bit ones whenever dM < 2^15 (2 * 32767^2 + 32767 < 2^31), which is every ray of a 0.05 m grid out to 1.6 km.
// The valid end point's extra pass and its hit are lane 0's.  grid (ceil(max_n / 4), n_scans), 256 threads = 4 rays
__global__ __launch_bounds__(256) void occ_trace_wave_kernel(OccArgs a) {
    const YmScanRef sr = a.scans[blockIdx.y];
    const int i = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (i >= sr.n) return;
    int x0, y0, x1, y1;
    bool end_valid;
    if (!occ_ray(sr, i, a, x0, y0, x1, y1, end_valid)) return;
    if (lane == 0 && end_valid) {
        occ_count(a, a.pass, x1, y1);
        occ_count(a, a.hits, x1, y1);
    }
    const bool steep = abs(y1 - y0) > abs(x1 - x0);
    if (steep) { int t = x0; x0 = y0; y0 = t; t = x1; x1 = y1; y1 = t; }
    if (x0 > x1) { int t = x0; x0 = x1; x1 = t; t = y0; y0 = y1; y1 = t; }
    const int d_major = x1 - x0, d_minor = abs(y1 - y0);
    const bool up = y0 < y1;
    if (d_major < 32768) {
        const unsigned dm2 = 2u * (unsigned)d_minor, dM = (unsigned)d_major, dM2 = 2u * dM;
        for (int k = lane; k <= d_major; k += 64) {
            const int m = dM ? (int)(((unsigned)k * dm2 + dM) / dM2) : 0;
            const int major = x0 + k, minor = up ? y0 + m : y0 - m;
            occ_count(a, a.pass, steep ? minor : major, steep ? major : minor);
        }
    } else {
        const unsigned long long dm2 = 2ull * (unsigned long long)d_minor, dM = (unsigned long long)d_major, dM2 = 2ull * dM;
        for (int k = lane; k <= d_major; k += 64) {
            const int m = (int)(((unsigned long long)k * dm2 + dM) / dM2);
            const int major = x0 + k, minor = up ? y0 + m : y0 - m;
            occ_count(a, a.pass, steep ? minor : major, steep ? major : minor);
        }
    }
}

// OccupancyGrid::Update / UpdateCell (MinPassThrough 2, OccupancyThreshold 0.1) on the window of the counts -> the image codes the
// ROS node reads, a dense [win_h][win_w] image.  grid (ceil(win_w / 256), min(win_h, 65535))
__global__ __launch_bounds__(256) void occ_update_kernel(OccArgs a) {
    const int x = blockIdx.x * 256 + threadIdx.x;
    if (x >= a.win_w) return;
    for (int y = blockIdx.y; y < a.win_h; y += gridDim.y) { // (a launch has at most 65535 rows of blocks)
        const size_t src = (size_t)(a.win_y + y) * (size_t)a.pitch + (size_t)(a.win_x + x);
        const unsigned pass = a.pass[src], hits = a.hits[src];
        uint8_t v = 200; // GridStates_Unknown
        if (pass > 2u) {
            const double ratio = (double)hits / (double)pass;
            v = ratio > 0.1 ? 0 /* GridStates_Occupied */ : 255 /* GridStates_Free */;
        }
        a.image[(size_t)y * (size_t)a.win_w + x] = v;
    }
}

}  // namespace ym
