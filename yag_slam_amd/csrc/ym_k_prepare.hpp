// ym_k_prepare.hpp -- K1 prepare: the scan projection and trigger chain (prepare_kernel, points_kernel, K0 structure_kernel), the
// cells stage in its three drivers (prepare_cells fused, cells_from_cache in registers, cells_from_cache_staged through LDS) over one
// statement of each cell rule (roi_offset, side_keeps, window_cell, store_cell), and K1c tiles_kernel.  K1b select: ym_k_select.hpp.
// Part of ym_kernels.hpp (include that, not this file).
#pragma once

namespace ym {

// ================================================================== K1 prepare
#define YM_PREP_LDS_BYTES(max_n) ((size_t)(max_n) * 25 + ((size_t)(max_n) / 64 + 2) * 4 + 16)
#define YM_INLINE_SCANS 16
#ifndef YM_CELLS_Q
#define YM_CELLS_Q 3         // chunks of 256 points the REGISTER path of the cells stage keeps in flight (cells_from_cache: the fused
                             // prepare_kernel and cells_kernel<false>); the staged path (cells_from_cache_staged) does not read it
#endif
// the staged path of cells_kernel (cells_from_cache_staged): chunks of 256 points whose loads one group issues together -- a
// 1081-reading scan is one group -- and the longest scan of a call that still takes it.  A block stages 16 bytes per reading of
// max_n in LDS, and the path is only worth having while a CU holds at least the seven blocks the register path's 72 VGPRs give
// it: 160 KiB / 7 = 23 405 bytes, rounded down to the LDS allocation granule (1280 bytes) 23 040 = 1440 readings.  Argued from
// occupancy; the crossover itself was not measured.
#define YM_CELLS_GROUP 5
#define YM_CELLS_STAGED_MAX_N 1440
#define YM_CELLS_STAGED_LDS_BYTES(max_n) ((size_t)(max_n) * 16)
struct YmInlineDesc {        // call descriptor passed in the kernel arguments (single item, few scans)
    YmItem item;
    YmScanRef scans[YM_INLINE_SCANS];
};
struct PrepareArgs {
    const YmScanRef *scans;  // device copy of the call descriptor; unused when use_inline
    const YmItem *items;
    int32_t use_inline;
    int32_t pad0;
    YmInlineDesc inl;
    YmGeom g;
    YmLattice lat;           // coarse lattice
    YmItemState *states;
    double2 *qlocal;         // [query slots][max_n]
    int32_t *qnp;            // [query slots] number of point readings of the slot's query
    YmCell *cells;           // [B][max_base][max_n]  window cell of every base point (ym_types.h), "no cell" when filtered
    int4 *bbox;              // [B][max_base][YM_N_BOXES(max_n)] window bounding box of YM_BOX_CELLS consecutive cells
    double2 *ctrig;          // [B][nt_stride] (cos, sin) of every coarse angle
    int32_t *hypcell;        // [B][2][dim_stride]
    double *probs;           // [B][ny*nx] cleared here, filled by the score stage
    int32_t max_n, max_base, nt_stride, dim_stride;
    // batches: the heavy work (projection, trigger chain) runs once per distinct stale scan / distinct query in
    // points_kernel; jobs[j] = scan index, bit 31 set = "as a query, into query slot (j's low bits in qjob_slot)"
    const int32_t *jobs;     // [n_jobs] scan index | (query ? 0x80000000 : 0)
    const int32_t *job_slot; // [n_jobs] query slot of a query job
    unsigned long long *stamps;
    // device-chained sequences (ym_map_sequence): the host sized the raster's tile rectangle from PREDICTED poses; a kept
    // cell outside cell_box (window cells whose smear stays inside the launched tiles) or an earlier step's fault makes
    // *fault = step (first one wins) and the host repeats from there with the poses it then knows
    int32_t *fault;          // null: not a chained step
    int32_t step, pad1;
    int32_t cell_box[4];     // x0, y0, x1, y1 (inclusive)
    int32_t *tile_max_zero;  // batches with raster work lists: the word tiles_kernel raises to the longest list, zeroed here (a
                             // memset of its own was one more launch in the chain), or null
};

// LDS carve-up shared by the kernels that project a scan
struct PrepLds {
    double *sx, *sy;
    int *nxt, *ex, *ent;
    unsigned char *chain;
};
__device__ __forceinline__ PrepLds prep_lds(unsigned char *raw, int max_n) {
    PrepLds l;
    l.sx = reinterpret_cast<double *>(raw);
    l.sy = l.sx + max_n;
    l.nxt = reinterpret_cast<int *>(l.sy + max_n);
    l.ex = l.nxt + max_n;                     // exit of the chain walk from point i out of its segment
    l.ent = l.ex + max_n;                     // chain entry node per 64-point segment (max_n/64 + 1)
    l.chain = reinterpret_cast<unsigned char *>(l.ent + max_n / 64 + 2);
    return l;
}

// ---- point readings, compacted in beam order (LocalizedRangeScan::Update / _get_point_readings) -> sx, sy; returns np.
// One barrier for the whole scan instead of two per NT beams: pass 1 counts the valid beams of every (chunk of NT
// beams, wave) by ballot, pass 2 re-reads the ranges (L1) and places each valid beam after everything before it.
template <int NT>
__device__ __forceinline__ int project_points(const YmScanRef &sr, double px, double py, double pt, bool yag, double *sx, double *sy,
                                              int *s_cnt /* (YM_MAX_BEAMS / NT + 1) * NT / 64 */, int32_t *cidx_out = nullptr) {
    constexpr int NW = NT / 64;
    const int tid = threadIdx.x;
    const int lane_ = tid & 63, wave_ = tid >> 6;
    const int per = (sr.n + NT - 1) / NT; // chunks of NT beams
    auto valid = [&](int i, double &r) {
        r = 0.0;
        if (i >= sr.n) return false;
        r = sr.ranges[i];
        return yag ? !(r > sr.range_threshold || isnan(r)) : (r >= sr.min_range && r <= sr.range_threshold);
    };
    for (int k = 0; k < per; k++) {
        double r;
        const unsigned long long m = __ballot(valid(k * NT + tid, r));
        if (lane_ == 0) s_cnt[k * NW + wave_] = __popcll(m);
    }
    __syncthreads();
    int running = 0;
    for (int k = 0; k < per; k++) {
        const int i = k * NT + tid;
        double r;
        const bool ok = valid(i, r);
        const unsigned long long m = __ballot(ok);
        int before = 0, total = 0;
#pragma unroll
        for (int w = 0; w < NW; w++) {
            const int c = s_cnt[k * NW + w];
            before += w < wave_ ? c : 0;
            total += c;
        }
        const int pos = running + before + __popcll(m & ((1ull << lane_) - 1ull));
        if (ok) {
            const double angle = pt + sr.min_angle + i * sr.angle_inc;
            sx[pos] = px + r * cos(angle);
            sy[pos] = py + r * sin(angle);
        }
        if (cidx_out && i < sr.n) cidx_out[i] = ok ? pos : -1;
        running += total;
    }
    __syncthreads();
    return running;
}

// The same with the compaction known (YmScanRef::cidx, from structure_kernel: which beams give a point reading, and where
// it goes, does not depend on the pose): one pass, one round of loads, one barrier.  gov != null: the scan's deciding
// pairs travel with it into LDS (l.nxt / l.ex are free when no chain is walked).
template <int NT>
__device__ __forceinline__ int project_points_indexed(const YmScanRef &sr, double px, double py, double pt, const PrepLds &l, bool with_gov) {
    for (int i = threadIdx.x; i < sr.n; i += NT) {
        const int pos = sr.cidx[i];
        const double r = sr.ranges[i];
        if (pos >= 0) {
            const double angle = pt + sr.min_angle + i * sr.angle_inc;
            l.sx[pos] = px + r * cos(angle);
            l.sy[pos] = py + r * sin(angle);
        }
    }
    if (with_gov) {
        const int2 *gov = reinterpret_cast<const int2 *>(sr.gov);
        for (int i = threadIdx.x; i < sr.cnp; i += NT) {
            const int2 g = gov[i];
            l.nxt[i] = g.x;
            l.ex[i] = g.y;
        }
    }
    __syncthreads();
    return sr.cnp;
}

// ---- the query-independent half of the valid-point filter (ScanMatcher::FindValidPoints / validate_points), parallel
// form: nxt[i] = first j > i farther than d from point i; the trigger chain is 0 -> nxt[0] -> ...; chain[i] = 1 for
// its nodes.  Marked without one long serial walk: cut the points into segments of 64; (1) every point walks to the
// first node past its own segment, (2) one thread hops from segment to segment with those exits (<= n/64 hops),
// (3) one thread per entered segment marks the chain nodes inside it.
// GUARD: also report (block-wide) whether any distance test came within YM_CHAIN_GUARD of the threshold.  The chain is a
// function of those tests' outcomes alone; squared distances between the same two readings computed at two different
// poses differ by rounding only (< 1e-11 m^2 for poses within 10 km and headings within 1000 rad: coordinates below 2^14 m
// carry errors below 4e-12 m, distances are at most 0.2 m), so a scan without a near test has the SAME chain at every
// such pose.
#define YM_CHAIN_GUARD 1e-9
#define YM_CHAIN_POSE_LIMIT 1.0e4
#define YM_CHAIN_HEADING_LIMIT 1.0e3 // (a heading of 1000 rad costs a beam angle 1e-13 rad of rounding: 3e-12 m at 30 m)
template <int NT, bool GUARD = false>
__device__ __forceinline__ int mark_chain(const PrepLds &l, int np, bool yag) {
    const int tid = threadIdx.x;
    const double min_sq = yag ? 0.2 * 0.2 : 0.1 * 0.1;
    int near = 0;
    for (int i = tid; i < np; i += NT) {
        const double fx = l.sx[i], fy = l.sy[i];
        int j = i + 1;
        for (; j < np; j++) {
            const double dx = fx - l.sx[j], dy = fy - l.sy[j];
            const double d2 = dx * dx + dy * dy;
            if (GUARD) near |= fabs(d2 - min_sq) <= YM_CHAIN_GUARD ? 1 : 0;
            if (d2 > min_sq) break;
        }
        l.nxt[i] = j;
        l.chain[i] = 0;
    }
    int unsafe = 0;
    if (GUARD) unsafe = __syncthreads_or(near);
    else __syncthreads();
    constexpr int SEG = 64;
    const int nseg = (np + SEG - 1) / SEG;
    for (int i = tid; i < np; i += NT) {
        const int seg_end = min(np, (i / SEG + 1) * SEG);
        int j = l.nxt[i];
        while (j < seg_end) j = l.nxt[j];
        l.ex[i] = j;
    }
    for (int i = tid; i < nseg; i += NT) l.ent[i] = -1;
    __syncthreads();
    if (tid == 0)
        for (int cur = 0; cur < np; cur = l.ex[cur]) l.ent[cur / SEG] = cur;
    __syncthreads();
    for (int sgi = tid; sgi < nseg; sgi += NT) {
        int c = l.ent[sgi];
        if (c >= 0) {
            const int seg_end = min(np, (sgi + 1) * SEG);
            for (; c < seg_end; c = l.nxt[c]) l.chain[c] = 1;
        }
    }
    __syncthreads();
    return unsafe;
}

// per point: the chain node that decides it (karto: the last node at or before i; yagpy: before i, none for point 0)
// and where that node's run ends (np = it never does)
__device__ __forceinline__ int2 gov_walk(const PrepLds &l, int i, int np, bool yag) {
    int s = yag ? i - 1 : i;
    if (s >= 0)
        while (!l.chain[s]) s--;
    return make_int2(s, s >= 0 ? l.nxt[s] : np);
}

// a projected base scan -> its slot of the matcher's point cache
template <int NT>
__device__ __forceinline__ void store_cache(const YmScanRef &sr, const PrepLds &l, int np, bool yag) {
    double2 *cpts = reinterpret_cast<double2 *>(sr.cache + YM_CACHE_HEADER);
    YmGov *cgov = reinterpret_cast<YmGov *>(sr.cache + YM_CACHE_HEADER + (size_t)sr.n * 16);
    const int2 *known = reinterpret_cast<const int2 *>(sr.gov);
    for (int i = threadIdx.x; i < np; i += NT) {
        cpts[i] = make_double2(l.sx[i], l.sy[i]);
        cgov[i] = ym_gov_pack(known ? known[i] : gov_walk(l, i, np, yag));
    }
    if (threadIdx.x == 0) *reinterpret_cast<int *>(sr.cache) = np;
}

// sensor-frame coordinates of a projected query (karto: Transform(pose).InverseTransformPose; yagpy: points_local)
template <int NT>
__device__ __forceinline__ void store_query_local(const YmScanRef &sr, const PrepLds &l, int np, bool yag, double2 *ql) {
    const bool identity = yag || (sr.pose[0] == 0.0 && sr.pose[1] == 0.0 && sr.pose[2] == 0.0);
    const double cr = cos(0.0 - sr.pose[2]), sn = sin(0.0 - sr.pose[2]);
    for (int i = threadIdx.x; i < np; i += NT) {
        double2 v;
        if (identity) {
            v = make_double2(l.sx[i], l.sy[i]);
        } else {
            const double dx = l.sx[i] - sr.pose[0], dy = l.sy[i] - sr.pose[1];
            v = make_double2(cr * dx + (0.0 - sn) * dy, sn * dx + cr * dy);
        }
        ql[i] = v;
    }
}

// everything of an item that depends on its query's pose and the lattice, but not on the query's readings:
// state, (cos, sin) per coarse angle (GridIndexLookup::ComputeOffsets), hypothesis cells
// (np < 0: the number of point readings is written by someone else -- prepare_kernel's query block)
template <int NT>
__device__ __forceinline__ void init_item(const PrepareArgs &a, int b, const YmItem &it, const YmScanRef &sr, int np, int qslot,
                                          const double2 *ql, double off_x, double off_y) {
    const int tid = threadIdx.x;
    if (tid == 0) {
        YmItemState &st = a.states[b];
        st.pose[0] = sr.pose[0]; st.pose[1] = sr.pose[1]; st.pose[2] = sr.pose[2];
        st.center[0] = sr.pose[0]; st.center[1] = sr.pose[1]; st.center[2] = sr.pose[2];
        st.off_x = off_x;
        st.off_y = off_y;
        if (np >= 0) st.nq = np;
        st.status = 0;
        st.regular[0] = st.regular[1] = 0;
        st.base_count = it.base_count;
        st.qslot = qslot;
        st.ql = ql;
    }
    // one fp64 sin/cos per coarse angle; the cell offsets themselves are computed by the correlate blocks that
    // consume them
    if (tid < a.lat.nt) {
        const double angle = (sr.pose[2] - a.lat.angle_off) + tid * a.lat.angle_res;
        a.ctrig[(size_t)b * a.nt_stride + tid] = make_double2(cos(angle), sin(angle));
    }
    for (int i = tid; i < a.lat.nx * a.lat.ny; i += NT) a.probs[(size_t)b * a.lat.nx * a.lat.ny + i] = 0.0; // (score_hyp_kernel: atomic max)
    // coarse hypothesis cells + regularity flag
    int32_t *cx = a.hypcell + (size_t)b * 2 * a.dim_stride;
    int32_t *cy = cx + a.dim_stride;
    for (int i = tid; i < a.lat.nx; i += NT) cx[i] = hyp_cell(sr.pose[0], -a.lat.off_x, i, a.lat.step_x, off_x, a.g);
    for (int i = tid; i < a.lat.ny; i += NT) cy[i] = hyp_cell(sr.pose[1], -a.lat.off_y, i, a.lat.step_y, off_y, a.g);
    __syncthreads();
    {
        const int stx = kt_round_int(a.lat.step_x * a.g.scale), sty = kt_round_int(a.lat.step_y * a.g.scale);
        int ok = a.g.kpitch == 0; // (Karto's linear-index test over the whole storage: the per-cell paths)
        for (int i = tid; i < a.lat.nx; i += NT) ok &= (cx[i] == cx[0] + i * stx);
        for (int i = tid; i < a.lat.ny; i += NT) ok &= (cy[i] == cy[0] + i * sty);
        ok = __syncthreads_and(ok);
        if (tid == 0) a.states[b].regular[0] = ok;
    }
}

// ---- the rules of the cells stage, each stated once.  Window cells and grids are compared bit for bit with the oracle: the fp64
// operations below are the oracle's, in its order.

// world offset of ROI cell (0, 0) along one axis: MatchScan, "set scan pose to be center of grid"
__device__ __forceinline__ double roi_offset(const YmGeom &g, double pose) { return pose - (0.5 * (g.roi_w - 1) * g.res); }

// The query-dependent half of FindValidPoints: a point is kept iff its run's trigger pair (f, t) puts t on the far side of the
// line through the viewpoint and f.
__device__ __forceinline__ bool side_keeps(double vpx, double vpy, const double2 &f, const double2 &t, bool yag) {
    const double fx = f.x, fy = f.y, cx = t.x, cy = t.y;
    const double aa = vpy - fy;
    const double bb = fx - vpx;
    const double cc = fy * vpx - fx * vpy;
    const double ss = cx * aa + cy * bb + cc;
    return yag ? (ss > 0.0) : !(ss < 0.0);
}

// AddScan's cell lookup.  The ROI cell of world point p: Karto's WorldToGrid, or the Python matcher's rint.
// (Into g by reference: with the cell returned by value, or as two ints, the compiler packs a window cell of the register path in
//  three vector instructions instead of two; this way cells_kernel<false> keeps the instruction stream it had before the rule was
//  shared -- scripts/kernel_asm_diff.py tells.)
__device__ __forceinline__ void roi_cell(const PrepareArgs &a, bool yag, const double2 &p, double off_x, double off_y, int2 &g) {
    int gx, gy;
    if (yag) {
        gx = (int)rint((p.x - off_x) / a.g.res);
        gy = (int)rint((p.y - off_y) / a.g.res);
    } else {
        gx = world_to_grid(p.x, off_x, a.g.scale);
        gy = world_to_grid(p.y, off_y, a.g.scale);
    }
    g = make_int2(gx, gy);
}
// ... and its window cell, "no cell" outside the ROI
__device__ __forceinline__ YmCell window_cell(const PrepareArgs &a, bool yag, const double2 &p, double off_x, double off_y) {
    int2 g;
    roi_cell(a, yag, p, off_x, off_y, g);
    return (g.x >= 0 && g.x < a.g.roi_w && g.y >= 0 && g.y < a.g.roi_w) ? ym_cell_pack(g.x + a.g.border - a.g.win_origin, g.y + a.g.border - a.g.win_origin)
                                                                         : ym_cell_none();
}

// where base scan `slot` of item b leaves its cells and the boxes of its chunks (YM_BOX_CELLS consecutive cells share a box)
struct CellSink {
    YmCell *cells;
    int4 *bbox;
    int n_cchunks;
};
__device__ __forceinline__ CellSink cell_sink(const PrepareArgs &a, int b, int slot) {
    CellSink o;
    o.n_cchunks = YM_N_BOXES(a.max_n);
    o.cells = a.cells + ((size_t)b * a.max_base + slot) * a.max_n;
    o.bbox = a.bbox + ((size_t)b * a.max_base + slot) * o.n_cchunks;
    return o;
}
// the tail of reading i: its cell (or "no cell") stored, a chained step's fault raised, and -- a row of 16 lanes covers one chunk,
// so every lane of the row comes here -- the chunk's bounding box: the raster kernel reads a chunk only when this box touches its tile
__device__ __forceinline__ void store_cell(const PrepareArgs &a, const CellSink &o, int i, YmCell w) {
    const int2 c = ym_cell_unpack(w);
    const bool has = c.x != YM_CELL_NONE;
    if (i < a.max_n) o.cells[i] = w;
    if (a.fault && has && (c.x < a.cell_box[0] || c.y < a.cell_box[1] || c.x > a.cell_box[2] || c.y > a.cell_box[3])) atomicCAS(a.fault, 0, a.step);
    const int x0 = row16_reduce(has ? c.x : INT32_MAX, OpMinI()), y0 = row16_reduce(has ? c.y : INT32_MAX, OpMinI());
    const int x1 = row16_reduce(has ? c.x : INT32_MIN, OpMaxI()), y1 = row16_reduce(has ? c.y : INT32_MIN, OpMaxI());
    if ((threadIdx.x & (YM_BOX_CELLS - 1)) == 0 && i / YM_BOX_CELLS < o.n_cchunks) o.bbox[i / YM_BOX_CELLS] = make_int4(x0, y0, x1, y1);
}

// One base scan of one item, just projected (the fused prepare_kernel): kept points become window cells.  PT(i) / GOV(i) read
// point i and its trigger pair from LDS or from the scan's known structure.
template <int NT, typename PT, typename GOV>
__device__ __forceinline__ void prepare_cells(const PrepareArgs &a, int b, int slot, int np, bool yag, double vpx, double vpy,
                                              double off_x, double off_y, PT pt_of, GOV gov_of) {
    const CellSink o = cell_sink(a, b, slot);
    for (int i0 = 0; i0 < o.n_cchunks * YM_BOX_CELLS; i0 += NT) {
        const int i = i0 + (int)threadIdx.x;
        YmCell w = ym_cell_none();
        if (i < np) {
            const int2 g = gov_of(i);
            if (g.x >= 0 && g.y < np && side_keeps(vpx, vpy, pt_of(g.x), pt_of(g.y), yag)) w = window_cell(a, yag, pt_of(i), off_x, off_y);
        }
        store_cell(a, o, i, w);
    }
}

// an unused chain slot of a ragged batch: no points (select_kernel walks every slot's cells), empty boxes
template <int NT>
__device__ __forceinline__ void clear_slot(const PrepareArgs &a, int b, int slot) {
    const CellSink o = cell_sink(a, b, slot);
    for (int i = threadIdx.x; i < a.max_n; i += NT) o.cells[i] = ym_cell_none();
    for (int i = threadIdx.x; i < o.n_cchunks; i += NT) o.bbox[i] = make_int4(INT32_MAX, INT32_MAX, INT32_MIN, INT32_MIN);
}

// the record of a reading past the scan's last: nobody decides it
__device__ __forceinline__ YmGov gov_undecided(int np) { return ym_gov_pack(make_int2(-1, np)); }

// one base scan of one item from the point cache, REGISTER path (the fused prepare_kernel's cache hits, and cells_kernel<false>
// for calls whose scans are too long for the staged path below): no LDS, no barrier.  Two dependent rounds of loads (who decides point i,
// with the point itself -> the two deciding points) are issued for Q chunks of the scan at a time, so a block waits two
// round trips per Q * NT points instead of two per NT.  The kernel is bound by those round trips times the blocks a CU
// holds, not by its bytes: a point is turned into its cell (one register) before its deciding points (eight) are asked for,
// which is what lets Q = 3 keep seven waves per SIMD.
template <int NT>
__device__ __forceinline__ void cells_from_cache(const PrepareArgs &a, int b, int slot, const YmScanRef &sr, const YmScanRef &qr, bool yag) {
    // (cells_kernel on 4096 items of 10 scans of 1081 readings, per launch: Q = 3 265 us at 72 VGPRs, Q = 4 309 at 86, Q = 5 -- one
    //  trip through the loop -- 282 at 100; with the point held until the store Q = 3 took 82 VGPRs and 312 us.  profiles/cells_packed_study.md)
    constexpr int Q = NT == 256 ? YM_CELLS_Q : 4;
    const double2 *__restrict__ cpts = reinterpret_cast<const double2 *>(sr.cache + YM_CACHE_HEADER);
    const YmGov *__restrict__ cgov = reinterpret_cast<const YmGov *>(sr.cache + YM_CACHE_HEADER + (size_t)sr.n * 16);
    const int np = *reinterpret_cast<const int *>(sr.cache);
    const double off_x = roi_offset(a.g, qr.pose[0]), off_y = roi_offset(a.g, qr.pose[1]);
    const double vpx = qr.pose[0], vpy = qr.pose[1];
    const int tid = threadIdx.x;
    const CellSink o = cell_sink(a, b, slot);
    const int n_pad = o.n_cchunks * YM_BOX_CELLS;
    for (int i0 = 0; i0 < n_pad; i0 += Q * NT) {
        YmGov g[Q]; // (kept as loaded -- one register a chunk with the packed records -- and taken apart where it is used)
        YmCell cw[Q];
        double2 f[Q], t[Q];
        {
            double2 p[Q];
#pragma unroll
            for (int q = 0; q < Q; q++) {
                const int i = i0 + q * NT + tid;
                g[q] = i < np ? cgov[i] : gov_undecided(np);
                p[q] = cpts[i < np ? i : 0];
            }
            // where the point lies, before the deciding points are asked for: a cell is one register (two in the wide build), the
            // point was four, and the registers a chunk holds at its widest decide how many chunks a SIMD keeps in flight
#pragma unroll
            for (int q = 0; q < Q; q++) cw[q] = window_cell(a, yag, p[q], off_x, off_y);
        }
        __builtin_amdgcn_sched_barrier(0); // (the deciding points' loads are not to be issued while the points are still held)
#pragma unroll
        for (int q = 0; q < Q; q++) {
            const int2 st = ym_gov_unpack(g[q]);
            const bool decided = st.x >= 0 && st.y < np;
            f[q] = cpts[decided ? st.x : 0];
            t[q] = cpts[decided ? st.y : 0];
        }
#pragma unroll
        for (int q = 0; q < Q; q++) {
            const int i = i0 + q * NT + tid;
            if (i0 + q * NT >= n_pad) break; // block-uniform
            const int2 st = ym_gov_unpack(g[q]);
            const bool keep = i < np && st.x >= 0 && st.y < np && side_keeps(vpx, vpy, f[q], t[q], yag);
            store_cell(a, o, i, keep ? cw[q] : ym_cell_none());
        }
    }
}

// The same cells and boxes with the second round of loads taken out of the vector memory pipeline (cells_kernel<true>, calls whose
// longest scan has at most YM_CELLS_STAGED_MAX_N readings).  The deciding points of a scan's readings are points of the same
// scan, and the block loads every one of them anyway.  Round one: the loads of the point and of who decides it, for all chunks of
// a group (YM_CELLS_GROUP chunks: a 1081-reading scan is one group) at once; a point that arrives becomes its cell -- one register
// -- and goes to LDS at its index (lp, 16 bytes per reading).  One barrier.  Round two, chunk by chunk: the deciding pair from
// LDS, the side test, the store, the box.  A block waits ONE round trip to
// memory per scan instead of two per Q chunks, and holds the eight registers of a deciding pair only for the chunk it is finishing.
// A scan of more than one group stages all its points first; the groups after the first then fetch their deciding records in
// round two (one more round trip per group) and take their own points back from LDS.
template <int NT>
__device__ __forceinline__ void cells_from_cache_staged(const PrepareArgs &a, int b, int slot, const YmScanRef &sr, const YmScanRef &qr, bool yag,
                                                        double2 *lp /* LDS, [max_n] */) {
    constexpr int G = YM_CELLS_GROUP;
    // The cache's records through GLOBAL loads.  A pointer read from the scan table is a flat address to the compiler, and a flat
    // load counts against the LDS counter as well as the memory counter: on this path, which waits on LDS, that cost 17 of 209 us.
    typedef const __attribute__((address_space(1))) double *global_f64;
    typedef const __attribute__((address_space(1))) YmGov *global_gov;
    const global_f64 cpts = (global_f64)reinterpret_cast<const double *>(sr.cache + YM_CACHE_HEADER);
    const global_gov cgov = (global_gov)reinterpret_cast<const YmGov *>(sr.cache + YM_CACHE_HEADER + (size_t)sr.n * 16);
    auto point = [&](int i) { return make_double2(cpts[2 * (size_t)i], cpts[2 * (size_t)i + 1]); }; // (one 16-byte load)
    const int np = *reinterpret_cast<const int *>(sr.cache);
    const double off_x = roi_offset(a.g, qr.pose[0]), off_y = roi_offset(a.g, qr.pose[1]);
    const double vpx = qr.pose[0], vpy = qr.pose[1];
    const int tid = threadIdx.x;
    const CellSink o = cell_sink(a, b, slot);
    const int n_pad = o.n_cchunks * YM_BOX_CELLS;
    // round one.  The first group: points and deciding records; what stays in registers is the record and the cell
    YmGov g[G];
    YmCell cw[G];
    {
        double2 p[G];
#pragma unroll
        for (int q = 0; q < G; q++) {
            const int i = q * NT + tid;
            g[q] = i < np ? cgov[i] : gov_undecided(np);
            p[q] = point(i < np ? i : 0);
        }
#pragma unroll
        for (int q = 0; q < G; q++) {
            const int i = q * NT + tid;
            if (i < np) lp[i] = p[q]; // (np <= sr.n <= max_n)
            cw[q] = window_cell(a, yag, p[q], off_x, off_y);
        }
    }
    // ... the groups after it (scans of more than G * NT readings): their points only
    for (int i = G * NT + tid; i < np; i += NT) lp[i] = point(i);
    __syncthreads();
    // round two
    auto finish = [&](int i, YmGov gv, YmCell cell) { // chunk by chunk
        const int2 st = ym_gov_unpack(gv);
        const bool keep = i < np && st.x >= 0 && st.y < np && side_keeps(vpx, vpy, lp[st.x], lp[st.y], yag);
        store_cell(a, o, i, keep ? cell : ym_cell_none());
    };
#pragma unroll
    for (int q = 0; q < G; q++)
        if (q * NT < n_pad) finish(q * NT + tid, g[q], cw[q]); // block-uniform
    for (int i0 = G * NT; i0 < n_pad; i0 += G * NT) {
        YmGov g2[G];
#pragma unroll
        for (int q = 0; q < G; q++) {
            const int i = i0 + q * NT + tid;
            g2[q] = i < np ? cgov[i] : gov_undecided(np);
        }
#pragma unroll
        for (int q = 0; q < G; q++) {
            const int i = i0 + q * NT + tid;
            if (i0 + q * NT < n_pad) finish(i, g2[q], i < np ? window_cell(a, yag, lp[i], off_x, off_y) : ym_cell_none());
        }
    }
}

// scan si of the call, at the pose the device holds for it (a chained step's pose comes from the step before: pose_dev)
__device__ __forceinline__ YmScanRef call_scan(const PrepareArgs &a, int si) {
    YmScanRef sr = a.use_inline ? a.inl.scans[si] : a.scans[si];
    if (sr.pose_dev) { sr.pose[0] = sr.pose_dev[0]; sr.pose[1] = sr.pose_dev[1]; sr.pose[2] = sr.pose_dev[2]; }
    return sr;
}

// "project this scan": its point readings -> l.sx, l.sy, their number returned.  A base scan at its pose; a query too, except in
// the Python matcher's semantics, which match the query's sensor-frame points (identity pose).  With the scan's structure known
// (cidx, and with it gov: trusted at this pose) the indexed form, with_gov: its deciding pairs into LDS beside the points.
__device__ __forceinline__ bool scan_indexed(const YmScanRef &sr) { return sr.cidx != nullptr && sr.n > 0; }
template <int NT>
__device__ __forceinline__ int project_scan(const YmScanRef &sr, bool is_query, bool yag, const PrepLds &l, int *s_cnt, bool with_gov) {
    const double px = (is_query && yag) ? 0.0 : sr.pose[0];
    const double py = (is_query && yag) ? 0.0 : sr.pose[1];
    const double pt = (is_query && yag) ? 0.0 : sr.pose[2];
    return scan_indexed(sr) ? project_points_indexed<NT>(sr, px, py, pt, l, with_gov) : project_points<NT>(sr, px, py, pt, yag, l.sx, l.sy, s_cnt);
}

// ---- K1, fused form (a few items): grid (max_base + 2, B), NT threads, dynamic LDS = YM_PREP_LDS_BYTES(max_n).
// blockIdx.x == 0: the query scan; blockIdx.x == 1 + j: base scan j of the item's chain; the last block: the item's
// state, coarse-angle table and hypothesis cells.  A base scan whose slot of
// the point cache is current takes the short path; otherwise it is projected here (and its slot filled).
template <int NT>
__global__ __launch_bounds__(NT) void prepare_kernel(PrepareArgs a) {
    extern __shared__ __attribute__((aligned(16))) unsigned char lds_raw[];
    __shared__ int s_cnt[(YM_MAX_BEAMS / NT + 1) * (NT / 64)];
    if (a.stamps && threadIdx.x == 0 && blockIdx.x == 0 && blockIdx.y == 0) a.stamps[28] = wall_clock64() - a.stamps[19]; // idle since the previous call's end
    YM_STAMP(a, 0);
    const int b = blockIdx.y;
    if (a.tile_max_zero && blockIdx.x == 0 && b == 0 && threadIdx.x == 0) *a.tile_max_zero = 0;
    const YmItem it = a.use_inline ? a.inl.item : a.items[b];
    const bool is_query = blockIdx.x == 0;
    const int slot = (int)blockIdx.x - 1;
    if ((int)blockIdx.x == a.max_base + 1) {
        // the item's block: everything that depends on the query's POSE and the lattice but not on its readings (state,
        // (cos, sin) per coarse angle -- fp64 sin / cos on a handful of lanes is a 1.3 us chain --, hypothesis cells, the
        // cleared maxima) runs beside the query's projection instead of after it
        const YmScanRef qr = call_scan(a, it.query);
        init_item<NT>(a, b, it, qr, -1, b, a.qlocal + (size_t)b * a.max_n, roi_offset(a.g, qr.pose[0]), roi_offset(a.g, qr.pose[1]));
        YM_STAMP_B1(a, 21);
        return;
    }
    if (!is_query && slot >= it.base_count) {
        clear_slot<NT>(a, b, slot);
        return;
    }
    const int si = is_query ? it.query : it.base_begin + slot;
    YmScanRef sr = call_scan(a, si);
    const YmScanRef qr = call_scan(a, it.query);
    if (a.fault && *a.fault) { // a chained step after a fault: nothing to do (the host repeats it); leave an empty problem
        if (!is_query) { clear_slot<NT>(a, b, slot); return; }
        sr.n = 0;
    }
    const bool yag = a.g.semantics == 1;
    if (!is_query && sr.cache && !sr.stale) {
        cells_from_cache<NT>(a, b, slot, sr, qr, yag);
        return;
    }
    const PrepLds l = prep_lds(lds_raw, a.max_n);
    const int np = project_scan<NT>(sr, is_query, yag, l, s_cnt, !is_query);
    YM_STAMP(a, 1);
    YM_STAMP_B1(a, 20);
    if (is_query) {
        store_query_local<NT>(sr, l, np, yag, a.qlocal + (size_t)b * a.max_n);
        if (threadIdx.x == 0) { a.qnp[b] = np; a.states[b].nq = np; } // (the rest of the state: the item's block)
        YM_STAMP(a, 2);
        YM_STAMP(a, 18);
        return;
    }
    const int2 *known = reinterpret_cast<const int2 *>(sr.gov); // the chain structure, when it is known to hold at this pose
    if (!known) mark_chain<NT>(l, np, yag);
    YM_STAMP_B1(a, 22);
    if (sr.cache) store_cache<NT>(sr, l, np, yag);
    const double off_x = roi_offset(a.g, qr.pose[0]), off_y = roi_offset(a.g, qr.pose[1]);
    auto pt_of = [&](int i) { return make_double2(l.sx[i], l.sy[i]); };
    if (scan_indexed(sr)) // (the deciding pairs came into LDS with the points)
        prepare_cells<NT>(a, b, slot, np, yag, qr.pose[0], qr.pose[1], off_x, off_y, pt_of, [&](int i) { return make_int2(l.nxt[i], l.ex[i]); });
    else if (known)
        prepare_cells<NT>(a, b, slot, np, yag, qr.pose[0], qr.pose[1], off_x, off_y, pt_of, [&](int i) { return known[i]; });
    else
        prepare_cells<NT>(a, b, slot, np, yag, qr.pose[0], qr.pose[1], off_x, off_y, pt_of, [&](int i) { return gov_walk(l, i, np, yag); });
    YM_STAMP_B1(a, 23);
}

// ---- K0 structure: grid (2), once per scan (ym_scan_create).  Block 0: Karto's rules, block 1: the Python matcher's.
// The trigger chain of the valid-point filter (which readings start a run, and where each run ends) depends on the
// readings' mutual distances only; computed here at the identity pose with a guard band around the distance threshold
// (mark_chain<GUARD>), it is what any pose within YM_CHAIN_POSE_LIMIT gives, bit for bit, unless a test was near the
// threshold -- then info says so and the matcher recomputes the chain from the projected points at every pose, as before.
struct StructureArgs {
    YmScanRef sr;       // ranges + sensor parameters
    int32_t *gov[2];    // [n][2] per semantics: for compacted point i the chain node that decides it and where its run ends
    int32_t *cidx[2];   // [n] per semantics: beam -> index of its point reading among the compacted ones, or -1
    int32_t *info;      // [2][2]: number of point readings, 1 = a distance test was within the guard band
    double *ranges_out; // null, or where block 0 copies the readings (sr.ranges is then the pinned host buffer they were staged in:
                        // the one launch is the upload)
    uint32_t *done;     // null, or [2] (pinned host memory): each block stores `serial` here when everything it writes is visible
    uint32_t serial;
    uint32_t pad;
};
template <int NT>
__device__ __forceinline__ void structure_body(const StructureArgs &a, int sem, unsigned char *lds_raw, int *s_cnt) {
    const bool yag = sem == 1;
    const PrepLds l = prep_lds(lds_raw, a.sr.n);
    // (no array of the argument record is indexed by a run-time value: that would put the record into scratch memory)
    const int np = project_points<NT>(a.sr, 0.0, 0.0, 0.0, yag, l.sx, l.sy, s_cnt, yag ? a.cidx[1] : a.cidx[0]);
    const int unsafe = mark_chain<NT, true>(l, np, yag);
    int2 *gov = reinterpret_cast<int2 *>(yag ? a.gov[1] : a.gov[0]);
    for (int i = threadIdx.x; i < np; i += NT) gov[i] = gov_walk(l, i, np, yag);
    if (a.ranges_out && sem == 0)
        for (int i = threadIdx.x; i < a.sr.n; i += NT) a.ranges_out[i] = a.sr.ranges[i];
    if (threadIdx.x == 0) { a.info[2 * sem] = np; a.info[2 * sem + 1] = unsafe; }
    if (a.done) {
        __syncthreads(); // every lane's stores are issued and waited for ...
        if (threadIdx.x == 0) {
            __threadfence_system(); // ... and written back before the host (and the kernels it launches next) can see the word
            __hip_atomic_store(a.done + sem, a.serial, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
        }
    }
}
// one scan (ym_scan_create): grid (2) = one block per semantics
template <int NT>
__global__ __launch_bounds__(NT) void structure_kernel(StructureArgs a) {
    extern __shared__ __attribute__((aligned(16))) unsigned char lds_raw[];
    __shared__ int s_cnt[(YM_MAX_BEAMS / NT + 1) * (NT / 64)];
    structure_body<NT>(a, (int)blockIdx.x, lds_raw, s_cnt);
}
// many scans (ym_scans_create): grid (2, scans), the argument records in device memory; completion by stream order (done == null)
template <int NT>
__global__ __launch_bounds__(NT) void structure_many_kernel(const StructureArgs *table) {
    extern __shared__ __attribute__((aligned(16))) unsigned char lds_raw[];
    __shared__ int s_cnt[(YM_MAX_BEAMS / NT + 1) * (NT / 64)];
    const StructureArgs a = table[blockIdx.y];
    structure_body<NT>(a, (int)blockIdx.x, lds_raw, s_cnt);
}

// ---- K1 for batches, first half: the heavy, query-independent work ONCE per distinct scan of the call.
// grid (n_jobs), 256 threads, dynamic LDS = YM_PREP_LDS_BYTES(max_n).  A query job projects the query and leaves its
// sensor-frame points in its query slot; a base job projects a base scan whose cache slot is stale and fills it.
#define YM_POINTS_THREADS 256
__global__ __launch_bounds__(YM_POINTS_THREADS) void points_kernel(PrepareArgs a) {
    constexpr int NT = YM_POINTS_THREADS;
    extern __shared__ __attribute__((aligned(16))) unsigned char lds_raw[];
    __shared__ int s_cnt[(YM_MAX_BEAMS / NT + 1) * (NT / 64)];
    const int job = a.jobs[blockIdx.x];
    const bool is_query = job < 0;
    const YmScanRef sr = a.scans[job & 0x7fffffff];
    const bool yag = a.g.semantics == 1;
    const PrepLds l = prep_lds(lds_raw, a.max_n);
    const int np = project_scan<NT>(sr, is_query, yag, l, s_cnt, false);
    if (is_query) { // into the scan's query slot of the point cache, else into the call's own buffer
        const int qs = a.job_slot[blockIdx.x];
        store_query_local<NT>(sr, l, np, yag, sr.qcache ? reinterpret_cast<double2 *>(sr.qcache + YM_CACHE_HEADER) : a.qlocal + (size_t)qs * a.max_n);
        if (threadIdx.x == 0) *(sr.qcache ? reinterpret_cast<int *>(sr.qcache) : a.qnp + qs) = np;
        return;
    }
    if (!sr.gov) mark_chain<NT>(l, np, yag);
    store_cache<NT>(sr, l, np, yag);
}

// ---- K1 for batches, second half: grid (max_base + 1, B), 256 threads.  Block 0 of an item sets the
// item up around its query's slot; block 1 + j turns base scan j's cached points into this item's cells.
// STAGED (the host: max_n <= YM_CELLS_STAGED_MAX_N): dynamic LDS = YM_CELLS_STAGED_LDS_BYTES(max_n), a scan's points staged there
// (cells_from_cache_staged); otherwise no dynamic LDS and the register path.  Block 0 and the cleared slots are the same in both
// and use none of it.
template <bool STAGED>
__global__ __launch_bounds__(256) void cells_kernel(PrepareArgs a) {
    extern __shared__ __attribute__((aligned(16))) unsigned char lds_raw[];
    constexpr int NT = 256;
    const int b = blockIdx.y;
    if (a.tile_max_zero && blockIdx.x == 0 && b == 0 && threadIdx.x == 0) *a.tile_max_zero = 0;
    const YmItem it = a.items[b];
    const int slot = (int)blockIdx.x - 1;
    const YmScanRef qr = a.scans[it.query];
    if (blockIdx.x == 0) {
        const int qs = it.pad; // query slot, set by the host
        const double2 *ql = qr.qcache ? reinterpret_cast<const double2 *>(qr.qcache + YM_CACHE_HEADER) : a.qlocal + (size_t)qs * a.max_n;
        init_item<NT>(a, b, it, qr, qr.qcache ? *reinterpret_cast<const int *>(qr.qcache) : a.qnp[qs], qs, ql,
                      roi_offset(a.g, qr.pose[0]), roi_offset(a.g, qr.pose[1]));
        return;
    }
    if (slot >= it.base_count) {
        clear_slot<NT>(a, b, slot);
        return;
    }
    if (STAGED) cells_from_cache_staged<NT>(a, b, slot, a.scans[it.base_begin + slot], qr, a.g.semantics == 1, reinterpret_cast<double2 *>(lds_raw));
    else cells_from_cache<NT>(a, b, slot, a.scans[it.base_begin + slot], qr, a.g.semantics == 1);
}

// ================================================================== K1c tiles: the raster kernel's work list (batches)
// One raster block per tile of the window lets ~3 of 4 blocks find out, after a round trip through the chunk boxes
// and a barrier, that they have nothing to do; on a batch that was most of the raster's time.  For batches this
// kernel (one block per item) turns the item's chunk boxes into the list of tiles that have work: a tile bitmap in
// LDS (every box marks the few tiles its smear halo reaches), compacted together with the tiles that hold stale
// bytes from an earlier call and only need clearing.  The raster kernel then runs one block per list entry.
// (Doing this in the last prepare block to finish needs a device-scope release per block, which on this part
// writes the XCD's L2 back: measured 98 -> 771 us for the prepare kernel.  A kernel boundary is cheaper.)
// The one block of an item is a chain of short phases, so what it waits for is round trips to memory: ONE now.  The
// item's boxes and the tile_zero bytes of the launched rectangle depend on nothing the kernel computes and are loaded
// together before the first barrier; a thread keeps its first YM_TILES_KEEP boxes in registers for the second pass
// (the hit slots) and re-reads only what lies beyond them, as it reads tile_zero bytes beyond its first YM_TILES_KEEP_Z.
#define YM_TILES_THREADS 256
#define YM_TILES_KEEP 3      // chunk boxes a thread keeps in registers between the two passes (the metric's 680 boxes: three a thread)
#define YM_TILES_KEEP_Z 2    // tile_zero bytes a thread loads with them (tiles of the launched rectangle, 256 a round)
struct TilesArgs {
    const int4 *bbox;        // [B][max_base][YM_N_BOXES(max_n)]
    uint32_t *tile_list;     // [B][tile_cap] tile index (tiy * tiles_x + tix), | 0x8000 = only needs clearing, | hits << 16 (0xffff =
                             // more than YM_TILE_HITS: the raster block walks the item's boxes)
    int32_t *tile_count;     // [B]
    int32_t *tile_max;       // longest list of the call (zeroed by the host before the launch)
    const uint8_t *tile_zero;// [B][tiles_y][tiles_x] 1 = the tile's memory is known to hold zeros
    int32_t max_n, max_base, half_kernel;
    int32_t tiles_x, tiles_y, tile_cap;
    int32_t launch[4];       // tile rectangle (x0, y0, x1, y1) the raster covers in this call
    // per LIST ENTRY the chunks that reach its tile, so that a raster block neither scans every box of the item nor looks
    // anything up before it can load them (their address depends on the entry's position alone):
    uint16_t *hits;          // [B][tile_cap][YM_TILE_HITS] index of the chunk's first cell in the item's cells; null = no lists (the raster walks the boxes)
    int32_t tile_h;          // rows per tile in this call (YM_TILE_H or YM_TILE_H_TALL)
    int32_t hit_limit;       // hit slots in use, <= YM_TILE_HITS (tests lower it)
};
// grid (B), dynamic LDS = 4 * ceil(tiles_x * tiles_y / 32) bytes (+ 8 bytes per tile of the rectangle with hit lists)
__global__ __launch_bounds__(YM_TILES_THREADS) void tiles_kernel(TilesArgs a) {
    extern __shared__ unsigned tile_bits[];
    __shared__ int s_n;
    constexpr int NT = YM_TILES_THREADS;
    const int tid = threadIdx.x, b = blockIdx.x;
    const int ntiles = a.tiles_x * a.tiles_y, nwords = (ntiles + 31) / 32;
    const int h = a.half_kernel;
    const int lx0 = a.launch[0], ly0 = a.launch[1], lx1 = a.launch[2], ly1 = a.launch[3];
    const int ltx = lx1 - lx0 + 1, lty = ly1 - ly0 + 1, nsub = ltx * lty;
    int *cnt = reinterpret_cast<int *>(tile_bits + nwords); // [nsub] hits per tile of the rectangle
    int *fill = cnt + nsub;                                 // [nsub] list position << 16 | hit slots filled
    // everything the kernel reads that depends on nothing it computes, in ONE round of loads ahead of the first barrier: the
    // thread's first YM_TILES_KEEP boxes (kept for the second pass) and the tile_zero bytes of its first YM_TILES_KEEP_Z tiles
    const int n_boxes = a.max_base * YM_N_BOXES(a.max_n);
    const int4 *bbox = a.bbox + (size_t)b * n_boxes;
    const uint8_t *tz = a.tile_zero + (size_t)b * ntiles;
    int4 mine[YM_TILES_KEEP];
    uint8_t zero_of[YM_TILES_KEEP_Z];
#pragma unroll
    for (int k = 0; k < YM_TILES_KEEP; k++) {
        const int c = k * NT + tid;
        mine[k] = c < n_boxes ? bbox[c] : make_int4(INT32_MAX, INT32_MAX, INT32_MIN, INT32_MIN);
    }
#pragma unroll
    for (int k = 0; k < YM_TILES_KEEP_Z; k++) {
        const int i = k * NT + tid;
        zero_of[k] = i < nsub ? tz[(ly0 + i / ltx) * a.tiles_x + lx0 + i % ltx] : (uint8_t)1;
    }
    for (int i = tid; i < nwords; i += NT) tile_bits[i] = 0u;
    if (a.hits)
        for (int i = tid; i < nsub; i += NT) cnt[i] = 0;
    if (tid == 0) s_n = 0;
    __syncthreads();
    const int th_shift = a.tile_h == YM_TILE_H_TALL ? 6 : 5; // (tile heights are 32 or 64: a runtime division costs ~25 instructions)
    static_assert(YM_TILE_H == 32 && YM_TILE_H_TALL == 64, "tile heights as shifts");
    auto mark = [&](const int4 &bb) {
        if (bb.x > bb.z) return;
        // tiles whose halo-extended rectangle [t*T - h, t*T + T + h - 1] meets the box (the raster kernel's own test)
        const int tx0 = max(lx0, max(bb.x - h, 0) / YM_TILE_W), tx1 = min(lx1, (bb.z + h) / YM_TILE_W);
        const int ty0 = max(ly0, max(bb.y - h, 0) >> th_shift), ty1 = min(ly1, (bb.w + h) >> th_shift);
        for (int ty = ty0; ty <= ty1; ty++)
            for (int tx = tx0; tx <= tx1; tx++) {
                const int t = ty * a.tiles_x + tx;
                atomicOr(&tile_bits[t >> 5], 1u << (t & 31));
                if (a.hits) atomicAdd(&cnt[(ty - ly0) * ltx + (tx - lx0)], 1);
            }
    };
#pragma unroll
    for (int k = 0; k < YM_TILES_KEEP; k++) mark(mine[k]);
    for (int c = YM_TILES_KEEP * NT + tid; c < n_boxes; c += NT) mark(bbox[c]);
    __syncthreads();
    uint32_t *list = a.tile_list + (size_t)b * a.tile_cap;
    auto enlist = [&](int i, bool zero) {
        const int ty = ly0 + i / ltx, tx = lx0 + i % ltx, t = ty * a.tiles_x + tx;
        const bool hit = (tile_bits[t >> 5] >> (t & 31)) & 1u;
        if (hit || !zero) {
            const int at = atomicAdd(&s_n, 1);
            const uint32_t nh = !a.hits ? 0xffffu : cnt[i] > a.hit_limit ? 0xffffu : (uint32_t)cnt[i];
            list[at] = (uint32_t)(t | (hit ? 0 : 0x8000)) | nh << 16;
            if (a.hits) fill[i] = at << 16;
        }
    };
#pragma unroll
    for (int k = 0; k < YM_TILES_KEEP_Z; k++)
        if (k * NT + tid < nsub) enlist(k * NT + tid, zero_of[k] != 0);
    for (int i = YM_TILES_KEEP_Z * NT + tid; i < nsub; i += NT) enlist(i, tz[(ly0 + i / ltx) * a.tiles_x + lx0 + i % ltx] != 0);
    __syncthreads();
    if (tid == 0) {
        a.tile_count[b] = s_n;
        if (s_n > *reinterpret_cast<volatile int32_t *>(a.tile_max)) atomicMax(a.tile_max, s_n); // (few blocks raise it)
    }
    if (!a.hits) return;
    // the hit slots: every box again -- the kept ones from their registers, the rest re-read --, to the entries of the tiles it
    // reaches (in any order: the raster ORs bits)
    uint16_t *hits = a.hits + (size_t)b * a.tile_cap * YM_TILE_HITS;
    const int n_cchunks = YM_N_BOXES(a.max_n);
    auto scatter = [&](int c, const int4 &bb) {
        if (bb.x > bb.z) return;
        const int slot = c / n_cchunks;
        const uint16_t first_cell = (uint16_t)(slot * a.max_n + (c - slot * n_cchunks) * YM_BOX_CELLS); // (the host: max_base * max_n < 65536)
        const int tx0 = max(lx0, max(bb.x - h, 0) / YM_TILE_W), tx1 = min(lx1, (bb.z + h) / YM_TILE_W);
        const int ty0 = max(ly0, max(bb.y - h, 0) >> th_shift), ty1 = min(ly1, (bb.w + h) >> th_shift);
        for (int ty = ty0; ty <= ty1; ty++)
            for (int tx = tx0; tx <= tx1; tx++) {
                const int i = (ty - ly0) * ltx + (tx - lx0);
                if (cnt[i] > a.hit_limit) continue;
                const int old = atomicAdd(&fill[i], 1);
                hits[(size_t)(old >> 16) * YM_TILE_HITS + (old & 0xffff)] = first_cell;
            }
    };
#pragma unroll
    for (int k = 0; k < YM_TILES_KEEP; k++) scatter(k * NT + tid, mine[k]);
    for (int c = YM_TILES_KEEP * NT + tid; c < n_boxes; c += NT) scatter(c, bbox[c]);
}

}  // namespace ym
