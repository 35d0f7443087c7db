// ym_k_locate.hpp -- locate a point set anywhere in a resident map: exact branch-and-bound over a max pyramid
// (host side ym_abi_locate.hpp).
//
// The score of hypothesis (k, cx, cy) is S = sum_l g8[cy + d_l.y][cx + d_l.x] with the integer offsets d of heading k
// (loc_offsets_kernel: the only fp64 of the search), reads outside the map counting 0.  Level j of the pyramid holds
// M_j[y][x] = max g8 over [x, x + 2^j) x [y, y + 2^j), stored for x, y >= -(2^j - 1) too: a window that hangs over the low
// edge still bounds the cells inside it.  A node (k, X, Y) of level j covers cx in [X, X + 2^j), cy in [Y, Y + 2^j); its bound
// B = sum_l M_j[Y + d_l.y][X + d_l.x] is >= S of every cell it covers (each term is), and equals S at level 0.  A node is
// dropped only when B < max(tau, S_min) -- strictly less: a tie may hide a smaller index -- so no hypothesis of the final
// top-K is ever lost, whatever the order nodes are visited in.
//
// A node is 64 bits: k << 32 | Y << 16 | X (maps up to 65536 x 65536, 65536 headings).  A leaf that survives becomes a key
// S << 40 | (2^40 - 1 - index), index = (k H + cy) W + cx < 2^40: larger key = better, keys are unique, the order is total.
#pragma once

namespace ym {

constexpr int kLocMaxLevels = 8;
constexpr int kLocMaxTop = 64;
constexpr int kLocMaxExcl = 15;    // picks a places search excludes (ym_locator_locate_places: at most 16 places)
constexpr int kLocTile = 8192;     // points of one heading staged in LDS at a time (32 KB)
constexpr int kLocThreads = 256;
constexpr uint64_t kLocIndexMask = (1ull << 40) - 1;

// the search state of one ym_locator_locate call, resident on the device
struct LocState {
    int32_t tau;        // the K-th best exact score so far, -1 while fewer than K are known
    int32_t n_top;      // entries of top[]
    uint32_t n_out;     // entries the running launch has appended to its output buffer
    uint32_t overflow;  // an append would have passed the end of the buffer (it was not written)
    uint32_t bad_offset; // an offset beyond int16
    uint32_t k_rem;     // radix select: the rank still looked for among the keys that share `prefix`
    uint32_t n_sel, pad;
    uint64_t prefix;    // radix select: the digits fixed so far
    unsigned long long survivors[kLocMaxLevels + 1];
    uint32_t hist[256];
    uint64_t sel[kLocMaxTop];
    uint64_t top[kLocMaxTop]; // keys, best first
    uint64_t beam[kLocMaxTop]; // the probe: keys (bound, position in the probed frontier) of the nodes it follows
    int32_t n_beam, pad2;
    // a places search: the picks so far (k, cx, cy, 0) and what the exact pass dropped because it was near one of them
    unsigned long long excluded_leaves, excluded_nodes;
    int32_t excl[kLocMaxExcl][4];
};

__device__ __forceinline__ uint64_t loc_node(uint32_t k, uint32_t x, uint32_t y) { return (uint64_t)k << 32 | (uint64_t)y << 16 | x; }

// ---- the pyramid: level j from level j - 1 by four reads at offsets 0 and h = 2^(j - 1); a read outside what the source
// level stores is 0.  Cell (x, y) of a level with margin m lies at [(y + m) * pitch + x + m].
__global__ __launch_bounds__(256) void loc_pyramid_kernel(const uint8_t *src, int sp, int sr, int sm, uint8_t *dst, int dp, int dr, int dm, int h) {
    const int ix = blockIdx.x * 64 + (threadIdx.x & 63), iy = blockIdx.y * 4 + (threadIdx.x >> 6);
    if (ix >= dp || iy >= dr) return;
    const int x = ix - dm + sm, y = iy - dm + sm; // in the source's storage
    int v = 0;
#pragma unroll
    for (int q = 0; q < 4; q++) {
        const int xx = x + (q & 1) * h, yy = y + (q >> 1) * h;
        if ((unsigned)xx < (unsigned)sp && (unsigned)yy < (unsigned)sr) {
            const int s = src[(size_t)yy * sp + xx];
            v = s > v ? s : v;
        }
    }
    dst[(size_t)iy * dp + ix] = (uint8_t)v;
}

// ---- the offset table: one (heading, point) pair per thread.  r = yag_rotate(P, c, s), d = rint(r / res): fp64 exactly as
// written (the library is built without contraction), so numpy restates it bit for bit.
__global__ __launch_bounds__(256) void loc_offsets_kernel(const double2 *pts, int stride, int nq, const double2 *dir_cs, int n_angles, double res,
                                                          uint32_t *out, LocState *st) {
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= (size_t)nq * n_angles) return;
    const int k = (int)(i / nq), l = (int)(i - (size_t)k * nq);
    const double2 cs = dir_cs[k];
    const double2 r = yag_rotate(pts[(size_t)l * stride], cs.x, cs.y);
    const double dx = rint(r.x / res), dy = rint(r.y / res);
    uint32_t o = 0;
    if (fabs(dx) <= 32767.0 && fabs(dy) <= 32767.0) o = (uint32_t)(uint16_t)(int16_t)(int)dx | (uint32_t)(uint16_t)(int16_t)(int)dy << 16;
    else atomicOr(&st->bad_offset, 1u); // (NaN lands here too)
    out[i] = o;
}

// ---- the top-level nodes [t0, t0 + n) of the (k, Y, X) order
__global__ __launch_bounds__(256) void loc_top_nodes_kernel(uint64_t t0, uint32_t n, uint32_t tx_n, uint32_t ty_n, int level, uint64_t *out) {
    const uint32_t i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const uint64_t t = t0 + i, per = (uint64_t)tx_n * ty_n;
    const uint32_t k = (uint32_t)(t / per), r = (uint32_t)(t - (uint64_t)k * per);
    const uint32_t ty = r / tx_n, tx = r - ty * tx_n;
    out[i] = loc_node(k, tx << level, ty << level);
}

// ---- before a level's launch: the output buffer starts empty; the leaves' buffer starts with the best known so far, so
// that the merge selects among old and new alike
__global__ __launch_bounds__(64) void loc_begin_kernel(LocState *st, uint64_t *out, int leaf) {
    const int n = leaf ? st->n_top : 0;
    if ((int)threadIdx.x < n) out[threadIdx.x] = st->top[threadIdx.x];
    if (threadIdx.x == 0) st->n_out = (uint32_t)n;
}

struct LocScoreArgs {
    const uint64_t *in;      // the frontier of this level
    uint32_t n_in;
    uint64_t *out;           // children (level > 0) or keys (level 0)
    uint32_t out_cap;
    const uint32_t *offsets; // [n_angles][nq] int16 pairs
    int32_t nq;
    const uint8_t *lvl;      // this level of the pyramid
    int32_t pitch, rows, margin;
    int32_t level, W, H;
    int32_t s_min;
    LocState *st;
    // the exclusion of a places search (read by the EXCL instantiations only): st->excl[0 .. n_excl)
    int32_t n_excl, sep_headings, circular, n_angles;
    int64_t sep_cells2;
};

// Is every hypothesis of node (k, X, Y) of level a.level near one pick?  Near: dk <= sep_headings (dk = |k - k'|, on a circle
// of n_angles headings when `circular`) and (x - x')^2 + (y - y')^2 <= sep_cells2.  The node's square is clipped to the map;
// its farthest corner from the pick decides.  At level 0 this is the leaf test itself.  Integers only; at most kLocMaxExcl turns.
__device__ __forceinline__ bool loc_excluded(const LocScoreArgs &a, int k, int X, int Y) {
    const int side = 1 << a.level;
    const int x1 = min(X + side, a.W) - 1, y1 = min(Y + side, a.H) - 1;
    const int n = min(a.n_excl, kLocMaxExcl);
    bool hit = false;
    for (int e = 0; e < n; e++) {
        const int pk = a.st->excl[e][0], px = a.st->excl[e][1], py = a.st->excl[e][2];
        int dk = abs(k - pk);
        if (a.circular) dk = min(dk, a.n_angles - dk);
        const int64_t dx = max(abs(X - px), abs(x1 - px)), dy = max(abs(Y - py), abs(y1 - py));
        hit |= dk <= a.sep_headings && dx * dx + dy * dy <= a.sep_cells2;
    }
    return hit;
}

__device__ __forceinline__ int loc_wave_scan(int v, int lane, int &total) { // exclusive prefix sum over the wave
    int s = v;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const int t = __shfl_up(s, o, 64);
        if (lane >= o) s += t;
    }
    total = __shfl(s, 63, 64);
    return s - v;
}

// ---- node scoring, prune and expand.  One node per lane; the frontier is (nearly) in (k, Y, X) order, so the lanes of a wave
// are neighbouring nodes of one heading along a row and a point's 64 byte reads fall into one or two lines.  The heading's
// offsets are staged through LDS in tiles (every lane reads the same word: a broadcast) and shared by the block's four waves;
// a block whose nodes span several headings takes them one after the other.  Integer adds only; the loads of eight points are
// in flight together (clamped to the level's first byte where the read falls outside, and not counted).
// A survivor of level > 0 appends its children that start inside the map -- the wave reserves its slots with one atomic and
// writes the upper row of children, then the lower, each in lane order, which keeps rows together for the next level.
// MODE 0: a level above the map (prune, expand).  MODE 1: level 0 (prune, keys for the merge).  MODE 2: the probe -- every
// node's key (bound, position in the frontier) is written, nothing is pruned or counted.
// EXCL (a places search): a node that is wholly near a pick is not scored.  The exact pass drops and
// counts it -- at level 0 that is the leaf test, which alone keeps the result exact; above, it only saves work -- and the probe
// gives it the key score 0, so that neither the beam nor tau follows an excluded hypothesis.  Without EXCL the kernel is what
// ym_locator_locate has always launched.
template <int MODE, bool EXCL>
__global__ __launch_bounds__(kLocThreads) void loc_score_kernel(LocScoreArgs a) {
    extern __shared__ __attribute__((aligned(16))) unsigned char loc_lds_raw[];
    uint32_t *s_off = reinterpret_cast<uint32_t *>(loc_lds_raw);
    __shared__ int s_next;
    const int tid = threadIdx.x, lane = tid & 63;
    const uint32_t i = blockIdx.x * kLocThreads + tid;
    const bool valid = i < a.n_in;
    const uint64_t node = valid ? a.in[i] : 0;
    const int X = (int)(node & 0xffff), Y = (int)((node >> 16) & 0xffff);
    bool excluded = false;
    if (EXCL) excluded = valid && loc_excluded(a, (int)(node >> 32), X, Y);
    const int k = valid && !excluded ? (int)(node >> 32) : INT_MAX; // (INT_MAX: no heading's turn scores this lane)
    const int bx = X + a.margin, by = Y + a.margin;
    const uint8_t *lvl = a.lvl;
    const unsigned pitch = (unsigned)a.pitch, rows = (unsigned)a.rows;
    int sum = 0, kcur = -1;
    for (;;) {
        if (tid == 0) s_next = INT_MAX;
        __syncthreads();
        int c = k > kcur ? k : INT_MAX;
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) c = min(c, __shfl_xor(c, o, 64));
        if (lane == 0 && c != INT_MAX) atomicMin(&s_next, c);
        __syncthreads();
        const int kn = s_next; // the block's next heading
        if (kn == INT_MAX) break;
        const bool mine = k == kn;
        const uint32_t *src = a.offsets + (size_t)kn * a.nq;
        for (int t0 = 0; t0 < a.nq; t0 += kLocTile) {
            const int nt = min(kLocTile, a.nq - t0);
            __syncthreads(); // the readers of the tile before (and of s_next) are through
            for (int l = tid; l < nt; l += kLocThreads) s_off[l] = src[t0 + l];
            __syncthreads();
            if (mine) {
#pragma unroll 8
                for (int l = 0; l < nt; l++) {
                    const uint32_t o = s_off[l];
                    const unsigned x = (unsigned)(bx + (int)(int16_t)(o & 0xffffu)), y = (unsigned)(by + ((int)o >> 16));
                    const bool in = x < pitch && y < rows;
                    const int v = lvl[in ? y * pitch + x : 0u];
                    sum += in ? v : 0;
                }
            }
        }
        kcur = kn;
    }
    if (MODE == 2) { // (the frontier's order is the keys' order: position i, no counter)
        if (valid) a.out[i] = (uint64_t)sum << 40 | (kLocIndexMask - i);
        return;
    }
    if (EXCL) {
        const int n_excluded = __popcll(__ballot(excluded));
        if (lane == 0 && n_excluded) atomicAdd(MODE == 1 ? &a.st->excluded_leaves : &a.st->excluded_nodes, (unsigned long long)n_excluded);
    }
    const int tau = a.st->tau;
    const bool keep = valid && !excluded && sum >= (tau > a.s_min ? tau : a.s_min);
    const unsigned long long kept = __ballot(keep);
    const int n_kept = __popcll(kept);
    if (lane == 0 && n_kept) atomicAdd(&a.st->survivors[a.level], (unsigned long long)n_kept);
    if (MODE == 1) {
        uint32_t base = 0;
        if (lane == 0 && n_kept) base = atomicAdd(&a.st->n_out, (uint32_t)n_kept);
        base = __shfl(base, 0, 64);
        if ((uint64_t)base + n_kept > a.out_cap) {
            if (lane == 0) atomicOr(&a.st->overflow, 1u);
        } else if (keep) {
            const uint64_t index = ((uint64_t)k * a.H + Y) * a.W + X;
            a.out[base + __popcll(kept & ((1ull << lane) - 1))] = (uint64_t)sum << 40 | (kLocIndexMask - index);
        }
    } else {
        const int h = 1 << (a.level - 1);
        const int cx = X + h < a.W ? 2 : 1;
        const int upper = keep ? cx : 0, lower = keep && Y + h < a.H ? cx : 0;
        int n_upper, n_lower;
        const int at_upper = loc_wave_scan(upper, lane, n_upper), at_lower = loc_wave_scan(lower, lane, n_lower);
        const int n_new = n_upper + n_lower;
        uint32_t base = 0;
        if (lane == 0 && n_new) base = atomicAdd(&a.st->n_out, (uint32_t)n_new);
        base = __shfl(base, 0, 64);
        if ((uint64_t)base + n_new > a.out_cap) {
            if (lane == 0) atomicOr(&a.st->overflow, 1u);
        } else {
            if (upper) {
                a.out[base + at_upper] = loc_node(k, X, Y);
                if (cx == 2) a.out[base + at_upper + 1] = loc_node(k, X + h, Y);
            }
            if (lower) {
                a.out[base + n_upper + at_lower] = loc_node(k, X, Y + h);
                if (cx == 2) a.out[base + n_upper + at_lower + 1] = loc_node(k, X + h, Y + h);
            }
        }
    }
}

// ---- (host) the launch of the node scoring kernel of one level: the instantiations without exclusion are those ym_locator_locate has always launched
template <int MODE>
static void loc_launch_score(const LocScoreArgs &a, size_t lds, hipStream_t st) {
    const dim3 grid((a.n_in + kLocThreads - 1) / kLocThreads), block(kLocThreads);
    if (a.n_excl > 0) hipLaunchKernelGGL((loc_score_kernel<MODE, true>), grid, block, lds, st, a);
    else hipLaunchKernelGGL((loc_score_kernel<MODE, false>), grid, block, lds, st, a);
}

// ---- the top-K merge: a radix select of the K-th largest key, eight 8-bit digits from the top.  Keys are unique, so
// exactly K keys are >= it; they are collected (in any order) and ranked by counting: deterministic.
__global__ __launch_bounds__(256) void loc_sel_hist_kernel(const uint64_t *keys, uint32_t n, int shift, LocState *st) {
    __shared__ uint32_t s_h[256];
    s_h[threadIdx.x] = 0;
    __syncthreads();
    const uint64_t prefix = st->prefix;
    for (uint32_t i = blockIdx.x * 256 + threadIdx.x; i < n; i += gridDim.x * 256) {
        const uint64_t key = keys[i];
        if (shift == 56 || (key >> (shift + 8)) == (prefix >> (shift + 8))) atomicAdd(&s_h[(key >> shift) & 255], 1u);
    }
    __syncthreads();
    if (s_h[threadIdx.x]) atomicAdd(&st->hist[threadIdx.x], s_h[threadIdx.x]);
}

// one thread: the digit in which the rank falls; the histogram is left zero for the next pass
__global__ __launch_bounds__(64) void loc_sel_pick_kernel(int shift, uint32_t k_first, LocState *st) {
    if (threadIdx.x != 0) return;
    uint32_t k_rem = shift == 56 ? k_first : st->k_rem;
    uint64_t prefix = shift == 56 ? 0 : st->prefix;
    int d = 255;
    for (; d > 0; d--) {
        const uint32_t c = st->hist[d];
        if (k_rem <= c) break;
        k_rem -= c;
    }
    for (int j = 0; j < 256; j++) st->hist[j] = 0;
    st->k_rem = k_rem;
    st->prefix = prefix | (uint64_t)d << shift;
}

__global__ __launch_bounds__(256) void loc_sel_collect_kernel(const uint64_t *keys, uint32_t n, LocState *st) {
    const uint64_t kth = st->prefix;
    for (uint32_t i = blockIdx.x * 256 + threadIdx.x; i < n; i += gridDim.x * 256) {
        const uint64_t key = keys[i];
        if (key >= kth) {
            const uint32_t slot = atomicAdd(&st->n_sel, 1u);
            if (slot < (uint32_t)kLocMaxTop) st->sel[slot] = key;
        }
    }
}

// dest 0: the selected keys are the best hypotheses so far (top[], and tau once there are top_k of them).  dest 1: they are the
// probe's beam.  dest 2: they are exact scores the probe found at level 0 -- only tau learns from them (the exact pass meets
// the same leaves again, so they must not enter top[] here).
__global__ __launch_bounds__(64) void loc_sel_rank_kernel(int top_k, int dest, LocState *st) {
    __shared__ uint64_t s_key[kLocMaxTop];
    const int n = min((int)st->n_sel, kLocMaxTop), t = threadIdx.x;
    if (t < n) s_key[t] = st->sel[t];
    __syncthreads();
    if (t < n) {
        int rank = 0;
        for (int j = 0; j < n; j++) rank += s_key[j] > s_key[t] ? 1 : 0;
        const int32_t score = (int32_t)(s_key[t] >> 40);
        if (dest == 0) st->top[rank] = s_key[t];
        if (dest == 1) st->beam[rank] = s_key[t];
        if (dest != 1 && rank == top_k - 1 && score > st->tau) st->tau = score;
    }
    if (t == 0) {
        if (dest == 0) st->n_top = n;
        if (dest == 1) st->n_beam = n;
        st->n_sel = 0;
    }
}

// ---- the probe's step down: the children of the beam's nodes, in beam order (one wave: deterministic)
__global__ __launch_bounds__(64) void loc_probe_expand_kernel(LocState *st, const uint64_t *in, int level, int W, int H, uint64_t *out) {
    const int t = threadIdx.x;
    const bool on = t < st->n_beam;
    const uint64_t node = on ? in[kLocIndexMask - (st->beam[t] & kLocIndexMask)] : 0;
    const uint32_t k = (uint32_t)(node >> 32);
    const int X = (int)(node & 0xffff), Y = (int)((node >> 16) & 0xffff), h = 1 << (level - 1);
    const int cx = X + h < W ? 2 : 1, cy = Y + h < H ? 2 : 1;
    int total;
    int at = loc_wave_scan(on ? cx * cy : 0, t, total);
    if (on) {
        for (int q = 0; q < 4; q++)
            if ((q & 1) < cx && (q >> 1) < cy) out[at++] = loc_node(k, X + (q & 1) * h, Y + (q >> 1) * h);
    }
    if (t == 0) st->n_out = (uint32_t)total;
}

}  // namespace ym
