// ym_k_sets.hpp -- "yagpy" semantics, several query scans matched as one point set against a chain of base scans
// (Scan2DMatcherPy.match_scan_sets, yag_slam/scan_matching.py:56-122): sets_grid_kernel.
// Part of ym_kernels.hpp (include that, not this file).  DESIGN.md section 18.
#pragma once

namespace ym {

// The G x G grid of every item of a chunk, as the bytes scoring reads (int(100 * cell), helpers.py:142-145), built from the item's base
// scans by the reference's rules (scan_matching.py:76-86):
//   points    every point reading of the base scan at its pose, compacted in beam order (project_points: _get_point_readings)
//   filter    validate_points (helpers.py:298-329) with the item's VIEW-POINT, which is not its search centre: the position of the
//             set's last query scan.  The rule is a chain: a reading farther than 0.2 m from the last trigger point closes a run, the run
//             (the readings after the previous trigger up to and including this one) is kept when the new trigger lies on the left of
//             the line from the view-point through the old one, and reading 0 and the readings after the last trigger belong to no run.
//             One thread walks the chain over the points in LDS -- the same operations on the same operands in the same order -- and
//             leaves the list of triggers (index, kept or not); every other reading then finds its run by a binary search.
//   cells     world_to_grid (helpers.py:82-83: fp64 division, round half to even) on the item's own origin; a reading outside
//             G x G is dropped (add_scan_to_grid, helpers.py:123-131)
//   smear     one lane per (kept reading, row of taps): smear_point's maximum (helpers.py:106-119), taps outside G x G dropped.
//             int(100 * v) grows with v, so the maximum of the byte table's entries is the byte of the maximum of the float taps, and
//             a maximum depends on no order: the row's bytes are raised word by word, a compare-and-swap on each aligned word
//             they touch, repeated while a byte there is lower (a byte outside the row takes part with 0).  The stamp itself (1.0)
//             is the table's centre tap.  gridDim.y blocks share the rows of a job; each projects and filters for itself.
// A base scan with fewer than two point readings stamps nothing (the reference raises an IndexError on an empty one: defined here).
struct SetsGridArgs {
    const YmScanRef *scans;     // the base scans of the call
    const int2 *jobs;           // this chunk's (base scan, item of the chunk) pairs
    const double2 *view;        // per item of the chunk: the view-point
    const YmItemState *states;  // per item of the chunk: off_x, off_y = world position of grid cell (0, 0)
    int32_t max_n, G;
    double res;
    const uint8_t *ktab;        // [ksize][ksize] int(100 * tap)
    int32_t ksize, pad;
    uint8_t *grid;              // [items of the chunk][grid_stride]
    size_t grid_stride;         // a multiple of four
};

// byte-wise maximum of two words
__device__ __forceinline__ unsigned sets_max4(unsigned a, unsigned b) {
    unsigned r = 0;
#pragma unroll
    for (int j = 0; j < 4; j++) r |= max(__builtin_amdgcn_ubfe(a, 8 * j, 8), __builtin_amdgcn_ubfe(b, 8 * j, 8)) << (8 * j);
    return r;
}

// the four bytes of the aligned word `w` of an item's grid raised to at least those of `v`
__device__ __forceinline__ void sets_word_max(unsigned *w, unsigned v) {
    unsigned old = __hip_atomic_load(w, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    for (;;) { // (bytes only grow: a stale value is a lower one and costs one more round)
        const unsigned nw = sets_max4(old, v);
        if (nw == old) break;
        const unsigned got = atomicCAS(w, old, nw);
        if (got == old) break;
        old = got;
    }
}

// grid (jobs of the chunk, blocks per job), NT threads, dynamic LDS = YM_PREP_LDS_BYTES(max_n)
template <int NT>
__global__ __launch_bounds__(NT) void sets_grid_kernel(SetsGridArgs a) {
    extern __shared__ __attribute__((aligned(16))) unsigned char lds_raw[];
    __shared__ int s_cnt[(YM_MAX_BEAMS / NT + 1) * (NT / 64)];
    __shared__ int s_ntrig;
    const PrepLds l = prep_lds(lds_raw, a.max_n);
    const int tid = threadIdx.x;
    const int2 job = a.jobs[blockIdx.x];
    const YmScanRef sr = a.scans[job.x];
    const int b = job.y;
    const int np = project_points<NT>(sr, sr.pose[0], sr.pose[1], sr.pose[2], true, l.sx, l.sy, s_cnt);
    if (np < 2) return; // (block-uniform)
    const double2 vp = a.view[b];
    int *trig = l.nxt; // trigger i of the chain: the index of its reading, complemented when its run is dropped
    int *cell = l.ex;  // per reading: gy * G + gx of a kept one inside the grid, else -1
    if (tid == 0) {
        const double msd = 0.2 * 0.2;
        const double vpx = vp.x, vpy = vp.y;
        double fpx = l.sx[0], fpy = l.sy[0];
        int nt = 0;
        for (int i = 1; i < np; i++) {
            const double cpx = l.sx[i], cpy = l.sy[i];
            if ((fpx - cpx) * (fpx - cpx) + (fpy - cpy) * (fpy - cpy) > msd) {
                const double a_ = vpy - fpy;
                const double b_ = fpx - vpx;
                const double c_ = fpy * vpx - fpx * vpy;
                fpx = cpx;
                fpy = cpy;
                const double ss = cpx * a_ + cpy * b_ + c_;
                trig[nt++] = ss > 0.0 ? i : ~i;
            }
        }
        s_ntrig = nt;
    }
    __syncthreads();
    const int nt = s_ntrig;
    const double ox = a.states[b].off_x, oy = a.states[b].off_y, res = a.res;
    const int G = a.G;
    for (int i = tid; i < np; i += NT) {
        int c = -1;
        int lo = 0, hi = nt; // the first trigger at or after reading i closes its run
        while (lo < hi) {
            const int mid = (lo + hi) >> 1;
            const int t = trig[mid];
            if ((t < 0 ? ~t : t) < i) lo = mid + 1;
            else hi = mid;
        }
        if (i > 0 && lo < nt && trig[lo] >= 0) {
            // (a NaN or an infinity fails the comparisons; so does what does not fit an int32)
            const double gx = rint((l.sx[i] - ox) / res), gy = rint((l.sy[i] - oy) / res);
            if (gx >= 0.0 && gx < (double)G && gy >= 0.0 && gy < (double)G) c = (int)gy * G + (int)gx; // (below 2^31: the host checks G)
        }
        cell[i] = c;
    }
    __syncthreads();
    const int ks = a.ksize, half = ks / 2;
    uint8_t *grid = a.grid + (size_t)b * a.grid_stride;
    const unsigned total = (unsigned)np * (unsigned)ks; // (below 2^31: the host checks)
    for (unsigned idx = blockIdx.y * NT + tid; idx < total; idx += NT * gridDim.y) {
        const int p = (int)(idx / (unsigned)ks), sy = (int)(idx - (unsigned)p * (unsigned)ks);
        const int c = cell[p];
        if (c < 0) continue;
        const int gy = c / G, gx = c - gy * G;
        const int y = gy + (sy - half);
        if (y < 0 || y >= G) continue; // in_grid_bounds, helpers.py:115
        const int x0 = max(0, gx - half), x1 = min(G - 1, gx + half);
        const int k0 = sy * ks - (gx - half); // kernel[sy][sx], helpers.py:116: the tap of column x is ktab[k0 + x]
        const int row = y * G, lo = row + x0, hi = row + x1; // (below 2^31)
        for (int wb = lo & ~3; wb <= hi; wb += 4) {
            unsigned v = 0;
#pragma unroll
            for (int j = 0; j < 4; j++) {
                const int at = wb + j;
                if (at >= lo && at <= hi) v |= (unsigned)a.ktab[k0 + (at - row)] << (8 * j);
            }
            if (v) sets_word_max(reinterpret_cast<unsigned *>(grid + wb), v); // (an item's grid starts at a multiple of four bytes)
        }
    }
}

}  // namespace ym
