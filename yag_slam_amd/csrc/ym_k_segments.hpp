// ym_k_segments.hpp -- the segment graph of a prior map from its label image: the reference's determine_centroids and
// create_edges (yag_slam/splicing.py:57-80), each one pass over the image with integer arithmetic.
//
// The label image is int32 [rows][pitch] (x = column, y = row), 0 = no segment, 1 .. K = segments.  The device copy's pitch
// is a multiple of 4 and its rows start 16-byte aligned, so a lane reads four labels with one load; columns >= width of
// the last vector are masked by coordinate, never by value.
//
// segment_range_kernel   the smallest and the largest label (the host sizes the statistics by them and refuses negatives)
// segment_stats_kernel   per label: pixel count, sum of columns, sum of rows, as 64-bit integers.  determine_centroids is then
//                        (sum_x / count, sum_y / count), one correctly rounded float64 division each: bit for bit np.mean of
//                        the integer coordinate arrays (every sum stays below 2^53 for images up to 65536 x 65536).
//                        Segments are compact, so a 64 x 64 tile holds few labels: a block sums into an LDS table keyed by
//                        label (kStatSlots entries, linear probing) and issues one global atomic triple per (block, label);
//                        a label that finds the table full goes to the global sums directly (slower, still exact).
// segment_edges_kernel   create_edges.  The boundary mask is skimage.segmentation.find_boundaries with its defaults
//                        (connectivity=1, mode="thick").  scikit-image's source is not part of the reference: the rule here
//                        restates the library's documented behaviour -- a pixel is a boundary pixel when the maximum and the
//                        minimum of the labels over the pixel and its 4 neighbours differ, neighbours outside the image are
//                        ignored, label 0 takes part like any other value.  PARITY with scikit-image itself UNPINNED; the
//                        fixture (tests/golden/make_golden_segments.py) pins it against the same rule written with scipy's
//                        grey dilation and erosion.
//                        For a boundary pixel (y, x) with y >= 2 and x >= 2 the window is rows y-2 .. y+1, columns x-2 .. x+1
//                        clipped at the bottom and right borders (the reference's slice [y-2:y+2, x-2:x+2]; for y < 2 or
//                        x < 2 that slice is empty on any image of 4 or more rows / columns and the pixel counts nothing --
//                        part of the contract).  Exactly two distinct non-zero labels a < b in the window: the pair (a, b)
//                        is counted once for this pixel, and the pixel's raster index y * width + x competes for the pair's
//                        first index (the reference's dict insertion order).  One label, or three and more: nothing.
//                        A tile of 64 x 16 pixels and its halo (2 up and left, 1 down and right; the mask's own 1-pixel halo
//                        lies inside it) is staged in LDS with zeros outside the image: a zero never counts in a window, so
//                        the clipping needs no test there; the mask tests coordinates.
//                        Pairs are counted in a global hash table keyed by (a << 32 | b): atomicCAS claims a slot, atomicAdd
//                        counts, atomicMin keeps the first index -- all integer, so the table's content does not depend on
//                        the order of arrival (only the slot a pair lands in does; the host sorts by first index).  A pair
//                        that finds no slot within kPairProbes sets the overflow flag: the host retries with a larger table.
// segment_compact_kernel the used slots of the table, packed.
// Plain C++ and vector memory operations only.  Part of ym_kernels.hpp (include that, not this file).
#pragma once

namespace ym {

constexpr int kSegTileW = 64;      // columns of a tile: one lane per column (edges), 16 lanes x 4 labels per row (stats)
constexpr int kSegStatTileH = 64;  // rows of a statistics tile
constexpr int kSegEdgeTileH = 16;  // rows of an edge tile: 4 per wave
constexpr int kStatSlots = 128;    // LDS table of the statistics block (a power of two)
constexpr int kSegLdsPitch = 72;   // LDS row of an edge tile: columns x0 - 4 .. x0 + 67 (the body starts 16-byte aligned)
constexpr int kSegRangeBlocks = 4096; // blocks of the label-range pass
constexpr int kPairProbes = 1024;  // slots a pair tries before it reports the table full
constexpr unsigned long long kPairEmpty = ~0ull;

struct SegArgs {
    const int32_t *img; // [height][pitch], pitch % 4 == 0
    int32_t width, height, pitch;
    // segment_range_kernel
    int32_t *range;     // [2]: min, max (initialised to INT32_MAX, INT32_MIN)
    // segment_stats_kernel
    int32_t n_labels;
    unsigned long long *count, *sum_x, *sum_y; // [n_labels], zeroed
    // segment_edges_kernel
    uint8_t *mask;                 // [height][width] 0 / 1 (the mask form), or null
    unsigned long long *keys;      // [slots] kPairEmpty
    unsigned *pair_count;          // [slots] 0
    unsigned long long *pair_first; // [slots] ~0
    uint32_t slots;                // a power of two
    unsigned *flags;               // [0] a label outside [0, n_labels) seen, [1] pair table full, [2] used slots, [3] compacted
    // segment_compact_kernel
    int32_t *out_pairs;            // [used][2] (a - 1, b - 1)
    int32_t *out_counts;           // [used]
    long long *out_first;          // [used]
};

// grid: any (grid-stride over the rows' vectors; the host launches at most kSegRangeBlocks), 256 threads
__global__ __launch_bounds__(256) void segment_range_kernel(SegArgs a) {
    const size_t vec_per_row = (size_t)(a.width + 3) / 4;
    const size_t n_vec = vec_per_row * (size_t)a.height;
    int lo = INT32_MAX, hi = INT32_MIN;
    for (size_t i = (size_t)blockIdx.x * 256u + threadIdx.x; i < n_vec; i += (size_t)gridDim.x * 256u) {
        const size_t y = i / vec_per_row;
        const int x = (int)(i - y * vec_per_row) * 4;
        const int4 v = *reinterpret_cast<const int4 *>(a.img + y * (size_t)a.pitch + x);
        const int l[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
        for (int k = 0; k < 4; k++)
            if (x + k < a.width) {
                lo = min(lo, l[k]);
                hi = max(hi, l[k]);
            }
    }
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) {
        lo = min(lo, __shfl_xor(lo, d, 64));
        hi = max(hi, __shfl_xor(hi, d, 64));
    }
    if ((threadIdx.x & 63) == 0 && lo <= hi) {
        atomicMin(&a.range[0], lo);
        atomicMax(&a.range[1], hi);
    }
}

// grid (ceil(width / 64), ceil(height / 64)), 256 threads: thread t reads labels 4 (t % 16) .. + 3 of rows t / 16 + 16 i
__global__ __launch_bounds__(256) void segment_stats_kernel(SegArgs a) {
    __shared__ int s_key[kStatSlots];
    __shared__ unsigned s_cnt[kStatSlots], s_sx[kStatSlots], s_sy[kStatSlots];
    const int t = threadIdx.x;
    if (t < kStatSlots) {
        s_key[t] = -1;
        s_cnt[t] = s_sx[t] = s_sy[t] = 0u;
    }
    __syncthreads();
    const int x = blockIdx.x * kSegTileW + (t & 15) * 4;
    const int y0 = blockIdx.y * kSegStatTileH + (t >> 4);
    bool bad = false;
    // a run of n equal labels of one row: n pixels, columns summing to sx (a tile's sums stay below 2^28)
    auto add = [&](int label, unsigned n, unsigned sx, unsigned sy) {
        unsigned s = ((unsigned)label * 0x9E3779B1u) >> 25;
#pragma unroll 1
        for (int p = 0; p < kStatSlots; p++, s = (s + 1) & (kStatSlots - 1)) {
            const int old = atomicCAS(&s_key[s], -1, label);
            if (old == -1 || old == label) {
                atomicAdd(&s_cnt[s], n);
                atomicAdd(&s_sx[s], sx);
                atomicAdd(&s_sy[s], sy);
                return;
            }
        }
        atomicAdd(&a.count[label], (unsigned long long)n);
        atomicAdd(&a.sum_x[label], (unsigned long long)sx);
        atomicAdd(&a.sum_y[label], (unsigned long long)sy);
    };
    if (x < a.width) {
#pragma unroll 1
        for (int i = 0; i < kSegStatTileH / 16; i++) {
            const int y = y0 + 16 * i;
            if (y >= a.height) break;
            const int4 v = *reinterpret_cast<const int4 *>(a.img + (size_t)y * a.pitch + x);
            const int l[4] = {v.x, v.y, v.z, v.w};
            int cur = -1;
            unsigned n = 0, sx = 0;
#pragma unroll
            for (int k = 0; k < 4; k++) {
                if (x + k >= a.width) continue;
                if (l[k] < 0 || l[k] >= a.n_labels) {
                    bad = true;
                    continue;
                }
                if (l[k] != cur) {
                    if (n) add(cur, n, sx, n * (unsigned)y);
                    cur = l[k];
                    n = 0;
                    sx = 0;
                }
                n++;
                sx += (unsigned)(x + k);
            }
            if (n) add(cur, n, sx, n * (unsigned)y);
        }
    }
    if (bad) atomicOr(&a.flags[0], 1u);
    __syncthreads();
    if (t < kStatSlots && s_key[t] >= 0) {
        const int label = s_key[t];
        atomicAdd(&a.count[label], (unsigned long long)s_cnt[t]);
        atomicAdd(&a.sum_x[label], (unsigned long long)s_sx[t]);
        atomicAdd(&a.sum_y[label], (unsigned long long)s_sy[t]);
    }
}

// n boundary pixels of one row, the first at raster index `index`, counted the pair `key`
__device__ inline void segment_pair_insert(const SegArgs &a, unsigned long long key, unsigned n, unsigned long long index) {
    unsigned long long h = key * 0x9E3779B97F4A7C15ull;
    unsigned s = (unsigned)(h >> 32) & (a.slots - 1);
    const unsigned probes = a.slots < (unsigned)kPairProbes ? a.slots : (unsigned)kPairProbes;
#pragma unroll 1
    for (unsigned p = 0; p < probes; p++, s = (s + 1) & (a.slots - 1)) {
        // (a key is written once and never changes: a plain read that sees one is final, one that sees "empty" is settled by the CAS)
        unsigned long long old = a.keys[s];
        if (old == kPairEmpty) {
            old = atomicCAS(&a.keys[s], kPairEmpty, key);
            if (old == kPairEmpty) {
                atomicAdd(&a.flags[2], 1u);
                old = key;
            }
        }
        if (old == key) {
            atomicAdd(&a.pair_count[s], n);
            atomicMin(&a.pair_first[s], index);
            return;
        }
    }
    atomicOr(&a.flags[1], 1u);
}

// grid (ceil(width / 64), ceil(height / 16)), 256 threads: wave w takes rows 4 w .. 4 w + 3 of the tile, a lane one column.
// kMask: write the boundary mask and count nothing (the tests' view of the first half of the rule)
template <bool kMask>
__global__ __launch_bounds__(256) void segment_edges_kernel(SegArgs a) {
    // LDS row r = image row y0 - 2 + r (kSegEdgeTileH + 3 rows), LDS column c = image column x0 - 4 + c
    __shared__ __attribute__((aligned(16))) int tile[(kSegEdgeTileH + 3) * kSegLdsPitch];
    const int t = threadIdx.x;
    const int x0 = blockIdx.x * kSegTileW, y0 = blockIdx.y * kSegEdgeTileH;
    // the body: 16 vectors per row (x0 is a multiple of 64, the device rows are 16-byte aligned and padded to a multiple of 4)
    for (int i = t; i < (kSegEdgeTileH + 3) * 16; i += 256) {
        const int r = i >> 4, x = x0 + (i & 15) * 4, y = y0 - 2 + r;
        int4 v = make_int4(0, 0, 0, 0);
        if (y >= 0 && y < a.height && x < a.width) {
            v = *reinterpret_cast<const int4 *>(a.img + (size_t)y * a.pitch + x);
            if (x + 1 >= a.width) v.y = 0;
            if (x + 2 >= a.width) v.z = 0;
            if (x + 3 >= a.width) v.w = 0;
        }
        *reinterpret_cast<int4 *>(&tile[r * kSegLdsPitch + 4 + (i & 15) * 4]) = v;
    }
    // the halo columns: x0 - 2, x0 - 1 and x0 + 64
    if (t < (kSegEdgeTileH + 3) * 3) {
        const int r = t / 3, k = t - 3 * r;
        const int x = k < 2 ? x0 - 2 + k : x0 + kSegTileW, y = y0 - 2 + r;
        int v = 0;
        if (y >= 0 && y < a.height && x >= 0 && x < a.width) v = a.img[(size_t)y * a.pitch + x];
        tile[r * kSegLdsPitch + 4 + (x - x0)] = v;
    }
    __syncthreads();
    const int lane = t & 63;
    const int x = x0 + lane;
    const bool live = x < a.width;
    const int *col = &tile[4 + lane]; // col[r * kSegLdsPitch + dx]: image (y0 - 2 + r, x + dx)
#pragma unroll 1
    for (int j = 0; j < 4; j++) {
        const int ry = (t >> 6) * 4 + j, y = y0 + ry; // (the same for every lane of a wave)
        if (y >= a.height) break;
        const int *c = col + (ry + 2) * kSegLdsPitch;
        const int v = c[0];
        int lo = v, hi = v;
        if (x > 0) { lo = min(lo, c[-1]); hi = max(hi, c[-1]); }
        if (x + 1 < a.width) { lo = min(lo, c[1]); hi = max(hi, c[1]); }
        if (y > 0) { lo = min(lo, c[-kSegLdsPitch]); hi = max(hi, c[-kSegLdsPitch]); }
        if (y + 1 < a.height) { lo = min(lo, c[kSegLdsPitch]); hi = max(hi, c[kSegLdsPitch]); }
        const bool boundary = live && lo != hi;
        if (kMask) {
            if (live) a.mask[(size_t)y * a.width + x] = boundary ? 1 : 0;
            continue;
        }
        // the pair this pixel counts (0: none; a pair's high half is a label >= 1)
        unsigned long long key = 0;
        if (boundary && y >= 2 && x >= 2) {
            // the distinct non-zero labels of the 4 x 4 window (zeros outside the image): the first two, and whether there are more
            int l0 = 0, l1 = 0;
            bool more = false;
#pragma unroll
            for (int dy = -2; dy <= 1; dy++)
#pragma unroll
                for (int dx = -2; dx <= 1; dx++) {
                    const int w = c[dy * kSegLdsPitch + dx];
                    if (w == 0 || w == l0 || w == l1) continue;
                    if (l0 == 0) l0 = w;
                    else if (l1 == 0) l1 = w;
                    else more = true;
                }
            if (!more && l1 != 0) key = ((unsigned long long)(unsigned)min(l0, l1) << 32) | (unsigned)max(l0, l1);
        }
        if (key != 0) segment_pair_insert(a, key, 1u, (unsigned long long)y * (unsigned)a.width + (unsigned)x);
    }
}

// grid ceil(slots / 256), 256 threads
__global__ __launch_bounds__(256) void segment_compact_kernel(SegArgs a) {
    const unsigned s = blockIdx.x * 256u + threadIdx.x;
    if (s >= a.slots) return;
    const unsigned long long key = a.keys[s];
    if (key == kPairEmpty) return;
    const unsigned o = atomicAdd(&a.flags[3], 1u);
    a.out_pairs[2 * (size_t)o] = (int32_t)(unsigned)(key >> 32) - 1;
    a.out_pairs[2 * (size_t)o + 1] = (int32_t)(unsigned)(key & 0xFFFFFFFFull) - 1;
    a.out_counts[o] = (int32_t)a.pair_count[s];
    a.out_first[o] = (long long)a.pair_first[s];
}

}  // namespace ym
