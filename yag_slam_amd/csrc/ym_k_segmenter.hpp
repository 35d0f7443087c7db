// ym_k_segmenter.hpp -- the map segmenter: a prior map's image to its label image (0 = no segment, 1 .. K), the step the
// reference does with OpenCV morphology and scikit-image's SLIC (yag_slam/splicing.py:32-55).  The pre-processing is the
// reference's by definition; the superpixel rules are this library's own ("Map segmenter"; PARITY with
// scikit-image UNPINNED) and are pinned by tests/segmenter_ref.py.  Integer arithmetic is exact; floating point is fp64 as
// written (the library is compiled with -ffp-contract=off); every sum that crosses threads is an integer sum, so no result
// depends on the order of arrival.
//
// seg_close_kernel      A: threshold (< 254 -> 0), t = 255 - a, grey dilation then erosion with a (2 r + 1)^2 square, both
//                       separable, pixels outside the image taking no part; closed = 255 - t, its exact sum and its count of
//                       non-zero pixels.  One 64 x 64 output tile per block through two LDS byte planes with a halo of 2 r.
// seg_cell_sums_kernel  B: count / sum_x / sum_y of the free pixels of every step x step cell.
// seg_flag_count_kernel, seg_scan_kernel, seg_rank_kernel<kSeeds / kRoots>
//                       a raster-order prefix sum over flags in three launches (per-block counts, one block over the counts,
//                       ranks).  kSeeds: the seeded cells (4 count >= step^2) get centre indices 0 .. K0 - 1 and their
//                       first centres; kRoots: the surviving component roots get segment numbers 1 .. K.
// seg_assign_kernel     C, the hot one: a block takes (a 64 x 64 part of) one cell, so all its pixels share the centres
//                       seeded in the 5 x 5 cells around it: loaded once into LDS, every pixel takes the nearest (strict <
//                       in raster order of cells = lowest centre index on a tie), sums per candidate go through LDS and
//                       leave as at most 75 64-bit global atomics per block.
// seg_centres_kernel    C.6: centres with pixels move to their pixels' mean, into the other centre buffer.
// seg_cc_init_kernel, seg_cc_merge_kernel, seg_cc_sizes_kernel
//                       D: union-find (ym_k_unionfind.hpp) over equal 4-neighbours, so the root
//                       of a component is its first pixel whatever the order.  Parents start at the start of the pixel's
//                       run within its wave's 64 columns; the merge pass joins runs across rows and across 64-column
//                       borders; the sizes pass flattens every pixel to its root and counts.
// seg_relabel_kernel    D.4: label = number of the pixel's root (0 for a dropped fragment or a pixel without a centre).
// Every loop has a bound; a bound that is reached raises err[kSegErrLoop] and the host fails the call.  Stages depend on
// each other only across launches.  Plain C++ and vector memory operations only.  Part of ym_kernels.hpp.
#pragma once

namespace ym {

constexpr int kCloseTile = 64;     // output tile of the closing
constexpr int kCloseMaxR = 15;     // close_size <= 31
constexpr int kClosePitch = 128;   // LDS row (>= kCloseTile + 4 kCloseMaxR)
constexpr int kCloseRows = kCloseTile + 4 * kCloseMaxR;
constexpr int kSegPart = 64;       // a block of the cell kernels takes at most kSegPart x kSegPart pixels of one cell
constexpr int kSegScanChunk = 4096; // items per block of the prefix sum
enum { kSegErrLoop = 0, kSegChanged = 1, kSegTotal = 2, kSegErrSlots = 4 };
enum { kSeeds = 0, kRoots = 1 };

struct SegmenterArgs {
    const uint8_t *src;   // [height][width] the map image (dense)
    uint8_t *closed;      // [height][width]
    int32_t width, height, radius;
    unsigned long long *sums; // [0] sum of closed, [1] free pixels, [2] labelled pixels
    unsigned *err;        // [kSegErrSlots]
    // cells
    int32_t step, gw, gh, parts; // parts: blocks per cell side = ceil(step / kSegPart)
    int32_t nbx;          // gw parts: the cell kernels' grid is one-dimensional, rows of nbx blocks
    unsigned long long *cell_acc; // [3][cells] count, sum_x, sum_y
    int32_t *cell_centre; // [cells] centre index, -1 = not seeded
    long long n_items;    // of the prefix sum: cells, or pixels
    unsigned *block_counts; // [ceil(n_items / kSegScanChunk)], in place: counts, then exclusive offsets
    unsigned n_blocks;
    // centres
    int32_t n_centres;
    const double2 *centres; // [n_centres] (x, y)
    double2 *centres_next;
    unsigned long long *acc; // [3][n_centres] count, sum_x, sum_y
    int32_t *assign;      // [height][pitch] centre + 1, 0 = none
    int32_t pitch;
    // components
    unsigned *parent;     // [height * width] raster index of a pixel of the same component, never above its own
    unsigned *size;       // [height * width] at a root: the component's pixels (0: 2^32 of them), then its number
    unsigned long long min_size;
    int32_t *labels;      // [height][pitch]
};

__device__ __forceinline__ unsigned long long wave_sum_u64(unsigned long long v) {
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) v += __shfl_xor(v, d, 64);
    return v;
}

// grid (ceil(width / 64), ceil(height / 64)), 256 threads
__global__ __launch_bounds__(256) void seg_close_kernel(SegmenterArgs a) {
    __shared__ uint8_t pa[kCloseRows * kClosePitch], pb[kCloseRows * kClosePitch];
    __shared__ unsigned long long red[8];
    const int t = threadIdx.x, r = a.radius;
    const int x0 = blockIdx.x * kCloseTile, y0 = blockIdx.y * kCloseTile;
    const int n4 = kCloseTile + 4 * r, n2 = kCloseTile + 2 * r;
    // pa[i][j] = t at (y0 - 2 r + i, x0 - 2 r + j), 0 outside the image (t >= 0: a zero takes no part in a maximum)
    for (int i = t; i < n4 * n4; i += 256) {
        const int row = i / n4, col = i - row * n4;
        const int y = y0 - 2 * r + row, x = x0 - 2 * r + col;
        uint8_t v = 0;
        if (y >= 0 && y < a.height && x >= 0 && x < a.width) {
            const uint8_t s = a.src[(size_t)y * a.width + x];
            v = (uint8_t)(255 - (s < 254 ? 0 : s));
        }
        pa[row * kClosePitch + col] = v;
    }
    __syncthreads();
    // pb[i][j] = max over columns: rows as pa, column j = x0 - r + j
    for (int i = t; i < n4 * n2; i += 256) {
        const int row = i / n2, col = i - row * n2;
        const uint8_t *p = &pa[row * kClosePitch + col];
        unsigned m = 0;
        for (int k = 0; k <= 2 * r; k++) m = max(m, (unsigned)p[k]);
        pb[row * kClosePitch + col] = (uint8_t)m;
    }
    __syncthreads();
    // pa[i][j] = the dilation at (y0 - r + i, x0 - r + j); 255 outside the image (takes no part in a minimum)
    for (int i = t; i < n2 * n2; i += 256) {
        const int row = i / n2, col = i - row * n2;
        const int y = y0 - r + row, x = x0 - r + col;
        unsigned m = 255;
        if (y >= 0 && y < a.height && x >= 0 && x < a.width) {
            const uint8_t *p = &pb[row * kClosePitch + col];
            m = 0;
            for (int k = 0; k <= 2 * r; k++) m = max(m, (unsigned)p[k * kClosePitch]);
        }
        pa[row * kClosePitch + col] = (uint8_t)m;
    }
    __syncthreads();
    // pb[i][j] = min over columns: row y0 - r + i, column x0 + j
    for (int i = t; i < n2 * kCloseTile; i += 256) {
        const int row = i / kCloseTile, col = i - row * kCloseTile;
        const uint8_t *p = &pa[row * kClosePitch + col];
        unsigned m = 255;
        for (int k = 0; k <= 2 * r; k++) m = min(m, (unsigned)p[k]);
        pb[row * kClosePitch + col] = (uint8_t)m;
    }
    __syncthreads();
    unsigned long long sum = 0, n_free = 0;
    for (int i = t; i < kCloseTile * kCloseTile; i += 256) {
        const int row = i / kCloseTile, col = i - row * kCloseTile;
        const int y = y0 + row, x = x0 + col;
        if (y >= a.height || x >= a.width) continue;
        const uint8_t *p = &pb[row * kClosePitch + col];
        unsigned m = 255;
        for (int k = 0; k <= 2 * r; k++) m = min(m, (unsigned)p[k * kClosePitch]);
        const unsigned c = 255u - m;
        a.closed[(size_t)y * a.width + x] = (uint8_t)c;
        sum += c;
        n_free += c != 0;
    }
    sum = wave_sum_u64(sum);
    n_free = wave_sum_u64(n_free);
    if ((t & 63) == 0) {
        red[t >> 6] = sum;
        red[4 + (t >> 6)] = n_free;
    }
    __syncthreads();
    if (t == 0) {
        atomicAdd(&a.sums[0], red[0] + red[1] + red[2] + red[3]);
        atomicAdd(&a.sums[1], red[4] + red[5] + red[6] + red[7]);
    }
}

// the pixels a block of the cell kernels takes: with (bx, by) = (blockIdx.x % nbx, blockIdx.x / nbx), part (bx % parts,
// by % parts) of cell (bx / parts, by / parts), clipped at the cell and at the image
struct SegPart {
    int cx, cy, x0, y0, w, h;
};
__device__ __forceinline__ SegPart seg_part(const SegmenterArgs &a) {
    SegPart p;
    const int by = blockIdx.x / a.nbx, bx = blockIdx.x - by * a.nbx;
    p.cx = bx / a.parts;
    p.cy = by / a.parts;
    const int px = (bx - p.cx * a.parts) * kSegPart, py = (by - p.cy * a.parts) * kSegPart;
    p.x0 = p.cx * a.step + px;
    p.y0 = p.cy * a.step + py;
    p.w = max(0, min(min(kSegPart, a.step - px), a.width - p.x0));
    p.h = max(0, min(min(kSegPart, a.step - py), a.height - p.y0));
    return p;
}

// grid gw parts * gh parts, 256 threads
__global__ __launch_bounds__(256) void seg_cell_sums_kernel(SegmenterArgs a) {
    __shared__ unsigned long long red[12];
    const SegPart p = seg_part(a);
    const int t = threadIdx.x, n = p.w * p.h;
    unsigned long long cnt = 0, sx = 0, sy = 0;
    for (int i = t; i < n; i += 256) {
        const int ly = i / p.w, x = p.x0 + (i - ly * p.w), y = p.y0 + ly;
        if (a.closed[(size_t)y * a.width + x]) {
            cnt++;
            sx += (unsigned)x;
            sy += (unsigned)y;
        }
    }
    cnt = wave_sum_u64(cnt);
    sx = wave_sum_u64(sx);
    sy = wave_sum_u64(sy);
    if ((t & 63) == 0) {
        red[t >> 6] = cnt;
        red[4 + (t >> 6)] = sx;
        red[8 + (t >> 6)] = sy;
    }
    __syncthreads();
    if (t < 3) {
        const unsigned long long v = red[4 * t] + red[4 * t + 1] + red[4 * t + 2] + red[4 * t + 3];
        const size_t cells = (size_t)a.gw * a.gh;
        if (v) atomicAdd(&a.cell_acc[t * cells + (size_t)p.cy * a.gw + p.cx], v);
    }
}

template <int kWhat>
__device__ __forceinline__ bool seg_flag(const SegmenterArgs &a, long long i) {
    if (i >= a.n_items) return false;
    if (kWhat == kSeeds) return 4ull * a.cell_acc[i] >= (unsigned long long)a.step * (unsigned long long)a.step;
    // a root: its own parent.  (A pixel without a centre is its own parent too: the assignment tells them apart.)
    const long long y = i / a.width;
    if (a.parent[i] != (unsigned)i || a.assign[y * a.pitch + (i - y * a.width)] == 0) return false;
    const unsigned s = a.size[i];
    return s == 0u || s >= a.min_size; // (a root counts itself: 0 is a count of 2^32 that wrapped)
}

// grid n_blocks, 256 threads: block_counts[b] = flags among items [b kSegScanChunk, (b + 1) kSegScanChunk)
template <int kWhat>
__global__ __launch_bounds__(256) void seg_flag_count_kernel(SegmenterArgs a) {
    __shared__ unsigned red[4];
    const int t = threadIdx.x;
    const long long base = (long long)blockIdx.x * kSegScanChunk;
    unsigned n = 0;
#pragma unroll 1
    for (int j = 0; j < kSegScanChunk / 256; j++) n += seg_flag<kWhat>(a, base + j * 256 + t);
    n = (unsigned)wave_sum_u64(n);
    if ((t & 63) == 0) red[t >> 6] = n;
    __syncthreads();
    if (t == 0) a.block_counts[blockIdx.x] = red[0] + red[1] + red[2] + red[3];
}

// one block of 1024 threads: block_counts -> exclusive offsets in place, err[kSegTotal] = the total
__global__ __launch_bounds__(1024) void seg_scan_kernel(SegmenterArgs a) {
    __shared__ unsigned wave_tot[16];
    __shared__ unsigned carry_s;
    const int t = threadIdx.x, lane = t & 63, w = t >> 6;
    if (t == 0) carry_s = 0;
    __syncthreads();
#pragma unroll 1
    for (unsigned base = 0; base < a.n_blocks; base += 1024) {
        const unsigned i = base + t;
        const unsigned v = i < a.n_blocks ? a.block_counts[i] : 0u;
        unsigned incl = v; // inclusive scan of the wave
#pragma unroll
        for (int d = 1; d < 64; d <<= 1) {
            const unsigned o = __shfl_up(incl, d, 64);
            if (lane >= d) incl += o;
        }
        if (lane == 63) wave_tot[w] = incl;
        __syncthreads();
        unsigned before = carry_s, all = 0;
        for (int k = 0; k < 16; k++) {
            if (k < w) before += wave_tot[k];
            all += wave_tot[k];
        }
        if (i < a.n_blocks) a.block_counts[i] = before + incl - v;
        __syncthreads();
        if (t == 0) carry_s += all;
        __syncthreads();
    }
    if (t == 0) a.err[kSegTotal] = carry_s;
}

// grid n_blocks, 256 threads: the flagged items' ranks in raster order
template <int kWhat>
__global__ __launch_bounds__(256) void seg_rank_kernel(SegmenterArgs a) {
    __shared__ unsigned wave_tot[4];
    const int t = threadIdx.x, lane = t & 63, w = t >> 6;
    const long long base = (long long)blockIdx.x * kSegScanChunk;
    unsigned carry = a.block_counts[blockIdx.x];
#pragma unroll 1
    for (int j = 0; j < kSegScanChunk / 256; j++) {
        const long long i = base + j * 256 + t;
        const bool flag = seg_flag<kWhat>(a, i);
        const unsigned long long m = __ballot(flag);
        if (lane == 0) wave_tot[w] = (unsigned)__popcll(m);
        __syncthreads();
        unsigned before = carry, all = 0;
        for (int k = 0; k < 4; k++) {
            if (k < w) before += wave_tot[k];
            all += wave_tot[k];
        }
        const unsigned rank = before + (unsigned)__popcll(m & ((1ull << lane) - 1ull));
        carry += all;
        __syncthreads();
        if (i >= a.n_items) continue;
        if (kWhat == kSeeds) {
            a.cell_centre[i] = flag ? (int32_t)rank : -1;
            if (flag) {
                const size_t cells = (size_t)a.n_items;
                const double n = (double)a.cell_acc[i];
                a.centres_next[rank] = make_double2((double)a.cell_acc[cells + i] / n, (double)a.cell_acc[2 * cells + i] / n);
            }
        } else if (a.parent[i] == (unsigned)i) {
            a.size[i] = flag ? rank + 1u : 0u; // (only this thread reads size[i] in this launch: the flag above)
        }
    }
}

// grid gw parts * gh parts, 256 threads
__global__ __launch_bounds__(256) void seg_assign_kernel(SegmenterArgs a) {
    __shared__ int s_k[25];
    __shared__ double s_x[25], s_y[25];
    __shared__ unsigned long long s_acc[75];
    __shared__ int s_changed;
    const SegPart p = seg_part(a);
    const int t = threadIdx.x, n = p.w * p.h;
    if (t < 25) {
        const int oy = t / 5, cy = p.cy + oy - 2, cx = p.cx + (t - oy * 5) - 2;
        int k = -1;
        if (cy >= 0 && cy < a.gh && cx >= 0 && cx < a.gw) k = a.cell_centre[(size_t)cy * a.gw + cx];
        s_k[t] = k;
        const double2 c = k >= 0 ? a.centres[k] : make_double2(0.0, 0.0);
        s_x[t] = c.x;
        s_y[t] = c.y;
    }
    if (t < 75) s_acc[t] = 0;
    if (t == 0) s_changed = 0;
    __syncthreads();
    // a thread's pixels mostly take the same centre: it sums a run of equal choices and hands it to LDS when the choice changes
    int cur = -1, changed = 0;
    unsigned cnt = 0;
    unsigned long long sx = 0, sy = 0;
    auto flush = [&]() {
        if (cur >= 0 && cnt) {
            atomicAdd(&s_acc[cur], (unsigned long long)cnt);
            atomicAdd(&s_acc[25 + cur], sx);
            atomicAdd(&s_acc[50 + cur], sy);
        }
    };
    for (int i = t; i < n; i += 256) {
        const int ly = i / p.w, x = p.x0 + (i - ly * p.w), y = p.y0 + ly;
        int best = -1;
        if (a.closed[(size_t)y * a.width + x]) {
            const double fx = (double)x, fy = (double)y;
            double best_d = 0.0;
#pragma unroll 1
            for (int c = 0; c < 25; c++) {
                if (s_k[c] < 0) continue;
                const double dx = fx - s_x[c], dy = fy - s_y[c];
                const double d = dx * dx + dy * dy;
                if (best < 0 || d < best_d) {
                    best = c;
                    best_d = d;
                }
            }
        }
        const int32_t label = best >= 0 ? s_k[best] + 1 : 0;
        int32_t *out = &a.assign[(size_t)y * a.pitch + x];
        changed |= *out != label;
        *out = label;
        if (best != cur) {
            flush();
            cur = best;
            cnt = 0;
            sx = sy = 0;
        }
        cnt++;
        sx += (unsigned)x;
        sy += (unsigned)y;
    }
    flush();
    if (changed) s_changed = 1;
    __syncthreads();
    if (t < 75) {
        const int c = t % 25;
        if (s_k[c] >= 0 && s_acc[c]) atomicAdd(&a.acc[(size_t)(t / 25) * a.n_centres + s_k[c]], s_acc[t]);
    }
    if (t == 0 && s_changed) atomicOr(&a.err[kSegChanged], 1u);
}

// grid ceil(n_centres / 256), 256 threads
__global__ __launch_bounds__(256) void seg_centres_kernel(SegmenterArgs a) {
    const int k = blockIdx.x * 256 + threadIdx.x;
    if (k >= a.n_centres) return;
    const unsigned long long n = a.acc[k];
    double2 c = a.centres[k];
    if (n) c = make_double2((double)a.acc[(size_t)a.n_centres + k] / (double)n, (double)a.acc[2 * (size_t)a.n_centres + k] / (double)n);
    a.centres_next[k] = c;
}

// grid (ceil(width / 64), ceil(height / 16)), 256 threads: wave w takes rows 4 w .. 4 w + 3 of the tile, a lane one column.
// parent = the first pixel of the lane's run of equal assignment within the wave's 64 columns
__global__ __launch_bounds__(256) void seg_cc_init_kernel(SegmenterArgs a) {
    const int lane = threadIdx.x & 63, x = blockIdx.x * 64 + lane;
#pragma unroll 1
    for (int j = 0; j < 4; j++) {
        const int y = blockIdx.y * 16 + (threadIdx.x >> 6) * 4 + j; // (the same for every lane of a wave)
        if (y >= a.height) break;
        const int v = x < a.width ? a.assign[(size_t)y * a.pitch + x] : -1;
        const int left = __shfl_up(v, 1, 64);
        const unsigned long long starts = __ballot(lane == 0 || left != v);
        const int first = 63 - __clzll((long long)(starts & (~0ull >> (63 - lane)))); // the last run start at or before this lane
        if (x < a.width) a.parent[(size_t)y * a.width + x] = (unsigned)((size_t)y * a.width + (x - lane + first));
    }
}

// grid as seg_cc_init_kernel.  Within a wave's 64 columns a run is one tree already, so a pixel joins its upper neighbour only
// where a run starts (its own, or the upper row's above it), and its left neighbour only across a 64-column border.
// (uf_union: ym_k_unionfind.hpp)
__global__ __launch_bounds__(256) void seg_cc_merge_kernel(SegmenterArgs a) {
    const int lane = threadIdx.x & 63, x = blockIdx.x * 64 + lane;
    if (x >= a.width) return;
#pragma unroll 1
    for (int j = 0; j < 4; j++) {
        const int y = blockIdx.y * 16 + (threadIdx.x >> 6) * 4 + j;
        if (y >= a.height) break;
        const int32_t *row = a.assign + (size_t)y * a.pitch;
        const int v = row[x];
        if (v == 0) continue;
        const unsigned i = (unsigned)((size_t)y * a.width + x);
        const bool left_same = x > 0 && row[x - 1] == v;
        if (left_same && lane == 0 && !uf_union(a.parent, i, i - 1u)) atomicOr(&a.err[kSegErrLoop], 1u);
        if (y > 0 && row[x - a.pitch] == v && (lane == 0 || !left_same || row[x - 1 - a.pitch] != v) && !uf_union(a.parent, i, i - (unsigned)a.width))
            atomicOr(&a.err[kSegErrLoop], 1u);
    }
}

// grid as seg_cc_init_kernel: every pixel's parent becomes its root, every root's size its pixels
__global__ __launch_bounds__(256) void seg_cc_sizes_kernel(SegmenterArgs a) {
    const int lane = threadIdx.x & 63, x = blockIdx.x * 64 + lane;
#pragma unroll 1
    for (int j = 0; j < 4; j++) {
        const int y = blockIdx.y * 16 + (threadIdx.x >> 6) * 4 + j;
        if (y >= a.height) break;
        const bool live = x < a.width && a.assign[(size_t)y * a.pitch + x] != 0;
        uf_wave_sizes(live, (unsigned)((size_t)y * a.width + x), a.parent, a.size);
    }
}

// grid as seg_cc_init_kernel: the label image, and the count of labelled pixels
__global__ __launch_bounds__(256) void seg_relabel_kernel(SegmenterArgs a) {
    const int lane = threadIdx.x & 63, x = blockIdx.x * 64 + lane;
    unsigned long long n = 0;
#pragma unroll 1
    for (int j = 0; j < 4; j++) {
        const int y = blockIdx.y * 16 + (threadIdx.x >> 6) * 4 + j;
        if (y >= a.height) break;
        if (x >= a.width) continue;
        int32_t label = 0;
        if (a.assign[(size_t)y * a.pitch + x] != 0) label = (int32_t)a.size[a.parent[(size_t)y * a.width + x]];
        a.labels[(size_t)y * a.pitch + x] = label;
        n += label != 0;
    }
    n = wave_sum_u64(n);
    if (lane == 0 && n) atomicAdd(&a.sums[2], n);
}

}  // namespace ym
