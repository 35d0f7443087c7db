// ym_abi_locate.hpp -- C ABI: locate a scan set anywhere in a resident map (ym_locator_*; ym_k_locate.hpp)
// Part of yagmatch.hip (included inside its extern "C" block); not a header of its own.
struct LocLevelHost {
    uint8_t *p = nullptr;
    int pitch = 0, rows = 0, margin = 0;
};

struct ym_locator {
    ym_matcher *m;       // resolution and stream; the matcher outlives the locator
    int device;
    int width, height, levels;
    int64_t max_nodes;
    size_t bytes = 0;    // device memory the handle holds
    DevBuf<uint8_t> d_pyr;    // level 0 (a copy of the map's byte grid), then levels 1 .. L with their low-side margins
    LocLevelHost level[ym::kLocMaxLevels + 1];
    DevBuf<uint64_t> d_front[2];  // the frontier, ping-pong: max_nodes + kLocMaxTop entries each
    DevBuf<uint64_t> d_beam;      // the probe's nodes, ping-pong: 4 kLocMaxTop entries each
    DevBuf<ym::LocState> d_state;
    DevBuf<YmItemState> d_item;   // map_points_kernel leaves the number of points here
    DevBuf<unsigned char> scans_dev;
    DevBuf<double2> pts, dirs;
    DevBuf<uint32_t> offsets;
};

// cells of the map covered by the first i top-level nodes of one heading, in (Y, X) order
static uint64_t locator_cells_before(const ym_locator *lc, uint64_t i) {
    const uint64_t side = 1ull << lc->levels, W = (uint64_t)lc->width, H = (uint64_t)lc->height;
    const uint64_t tx_n = (W + side - 1) / side;
    const uint64_t ty = i / tx_n, tx = i % tx_n;
    const uint64_t y0 = std::min(ty * side, H), ch = std::min(side, H - y0);
    return W * y0 + ch * std::min(tx * side, W);
}

ym_locator *ym_locator_create(ym_matcher *m, const ym_map *mp, int levels, int64_t max_nodes) {
    if (!m || !mp) { set_err(YM_ERR_INVALID, "null argument"); return nullptr; }
    if (m->cfg.semantics != YM_SEM_YAGPY) { set_err(YM_ERR_UNSUPPORTED, "ym_locator_create needs a YM_SEM_YAGPY matcher"); return nullptr; }
    if (mp->device != m->device) { set_err(YM_ERR_INVALID, "map lives on another device"); return nullptr; }
    const int W = mp->width, H = mp->height;
    if (W > 65536 || H > 65536) { set_err(YM_ERR_UNSUPPORTED, "map of %d x %d cells: at most 65536 per axis", W, H); return nullptr; }
    if (levels > ym::kLocMaxLevels) { set_err(YM_ERR_INVALID, "levels = %d: at most %d", levels, ym::kLocMaxLevels); return nullptr; }
    if (levels < 0) { // the largest L with 2^L <= min(W, H) / 4, at most 6
        levels = 0;
        while (levels < 6 && (4 << (levels + 1)) <= std::min(W, H)) levels++;
    } else if ((1 << levels) > std::min(W, H)) {
        set_err(YM_ERR_INVALID, "levels = %d: a top-level node of %d cells is wider than the %d x %d map", levels, 1 << levels, W, H);
        return nullptr;
    }
    if (max_nodes <= 0) max_nodes = (int64_t)1 << 25;
    if (max_nodes > ((int64_t)1 << 30)) { set_err(YM_ERR_INVALID, "max_nodes = %lld: at most 2^30", (long long)max_nodes); return nullptr; }
    const int64_t side = (int64_t)1 << levels;
    if (std::min<int64_t>(side, W) * std::min<int64_t>(side, H) > max_nodes) { // before anything is launched
        set_err(YM_ERR_INVALID, "one top-level node expands to %lld cells, max_nodes is %lld",
                (long long)(std::min<int64_t>(side, W) * std::min<int64_t>(side, H)), (long long)max_nodes);
        return nullptr;
    }
    DevGuard guard(m->device);
    if (guard.status() != YM_OK) return nullptr;
    ym_locator *lc = new ym_locator();
    lc->m = m; lc->device = m->device; lc->width = W; lc->height = H; lc->levels = levels; lc->max_nodes = max_nodes;
    size_t pyr_bytes = 0, at[ym::kLocMaxLevels + 1];
    for (int j = 0; j <= levels; j++) {
        LocLevelHost &lv = lc->level[j];
        lv.margin = (1 << j) - 1; lv.pitch = W + lv.margin; lv.rows = H + lv.margin;
        at[j] = pyr_bytes;
        pyr_bytes += align_up((size_t)lv.pitch * lv.rows, 256);
    }
    // (the probe's keys of up to 4 kLocMaxTop beam children go through the second buffer too, whatever max_nodes is)
    const size_t front_n = (size_t)std::max<int64_t>(max_nodes, 4 * ym::kLocMaxTop) + ym::kLocMaxTop;
    lc->bytes = pyr_bytes + 2 * front_n * sizeof(uint64_t) + 8 * ym::kLocMaxTop * sizeof(uint64_t) + sizeof(ym::LocState) + sizeof(YmItemState);
    auto setup = [&]() -> int {
        int rc;
        if ((rc = lc->d_pyr.alloc(pyr_bytes)) || (rc = lc->d_front[0].alloc(front_n)) || (rc = lc->d_front[1].alloc(front_n)) ||
            (rc = lc->d_beam.alloc(8 * ym::kLocMaxTop)) || (rc = lc->d_state.alloc(1)) || (rc = lc->d_item.alloc(1)))
            return rc;
        for (int j = 0; j <= levels; j++) lc->level[j].p = lc->d_pyr.p + at[j];
        hipStream_t st = m->stream;
        HIP_TRY(hipMemcpyAsync(lc->level[0].p, mp->d_g8.p, (size_t)W * H, hipMemcpyDeviceToDevice, st));
        for (int j = 1; j <= levels; j++) {
            const LocLevelHost &s = lc->level[j - 1], &d = lc->level[j];
            hipLaunchKernelGGL(ym::loc_pyramid_kernel, dim3((d.pitch + 63) / 64, (d.rows + 3) / 4), dim3(256), 0, st, s.p, s.pitch, s.rows, s.margin,
                               d.p, d.pitch, d.rows, d.margin, 1 << (j - 1));
        }
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipStreamSynchronize(st));
        return YM_OK;
    };
    if (setup() != YM_OK) { delete lc; return nullptr; } // (the error text is set)
    return lc;
}

int ym_locator_get_info(const ym_locator *lc, ym_locator_info *info) {
    if (!lc || !info) return set_err(YM_ERR_INVALID, "null argument");
    info->width = lc->width; info->height = lc->height; info->levels = lc->levels; info->reserved = 0;
    info->max_nodes = lc->max_nodes; info->bytes = (int64_t)lc->bytes;
    return YM_OK;
}

int ym_locator_read_level(const ym_locator *lc, int level, uint8_t *out, int64_t n) {
    if (!lc || !out) return set_err(YM_ERR_INVALID, "null argument");
    if (level < 0 || level > lc->levels) return set_err(YM_ERR_INVALID, "level %d: the pyramid has levels 0 .. %d", level, lc->levels);
    const size_t need = (size_t)lc->width * lc->height;
    if (n < 0 || (size_t)n < need) return set_err(YM_ERR_INVALID, "buffer too small: need %zu bytes", need);
    DEV_GUARD(lc->device);
    const LocLevelHost &lv = lc->level[level];
    std::vector<uint8_t> tmp(need);
    HIP_TRY(hipMemcpy2D(tmp.data(), lc->width, lv.p + (size_t)lv.margin * lv.pitch + lv.margin, lv.pitch, lc->width, lc->height, hipMemcpyDeviceToHost));
    std::memcpy(out, tmp.data(), need);
    return YM_OK;
}

// what both locate calls check alike, and the point set and offset table they search with
struct LocQuery {
    int nq = 0, stride = 1;
    int32_t s_min = 0;
};

// an exclusion list (ym_locator_locate_places); empty for ym_locator_locate
struct LocExclude {
    int n = 0;
    int64_t sep_cells2 = 0;
    int32_t sep_headings = 0, circular = 0;
    int32_t pick[ym::kLocMaxExcl][3]; // k, cx, cy
};

// ---- the argument checks of the locate calls, then the point set, exactly as ym_match_map builds it (every query's readings
// at its own pose minus the mean query position), and the offset table.  Writes nothing the caller sees; the caller holds the
// device guard.
static int locator_prepare(ym_locator *lc, const ym_scan *const *queries, int n_queries, const double *dir_cs, int n_angles, int point_stride,
                           double min_response, LocQuery *q) {
    ym_matcher *m = lc->m;
    if (n_queries <= 0 || n_queries > 64) return set_err(YM_ERR_INVALID, "n_queries must be in [1, 64]");
    if (n_angles < 1 || n_angles > 65536) return set_err(YM_ERR_INVALID, "n_angles = %d: 1 .. 65536", n_angles);
    if (point_stride < 1) return set_err(YM_ERR_INVALID, "point_stride = %d leaves no point", point_stride);
    if (!(min_response >= 0.0)) return set_err(YM_ERR_INVALID, "min_response must be >= 0");
    int total = 0, max_n = 1;
    double sx = 0, sy = 0;
    for (int i = 0; i < n_queries; i++) {
        if (!queries[i] || queries[i]->device != lc->device) return set_err(YM_ERR_INVALID, "query %d is null or lives on another device", i);
        sx = i == 0 ? queries[i]->pose[0] : sx + queries[i]->pose[0];
        sy = i == 0 ? queries[i]->pose[1] : sy + queries[i]->pose[1];
        total += queries[i]->n;
        max_n = std::max(max_n, queries[i]->n);
    }
    const int W = lc->width, H = lc->height;
    if ((double)n_angles * W * H > (double)ym::kLocIndexMask)
        return set_err(YM_ERR_UNSUPPORTED, "%d headings of a %d x %d map: more than 2^40 hypotheses", n_angles, W, H);
    hipStream_t st = m->stream;
    int rc;
    const double ox_real = sx / (double)n_queries, oy_real = sy / (double)n_queries;
    std::vector<YmScanRef> hs(n_queries);
    for (int i = 0; i < n_queries; i++) hs[i] = scan_ref(queries[i]);
    if ((rc = lc->scans_dev.ensure(sizeof(YmScanRef) * n_queries)) || (rc = lc->pts.ensure((size_t)std::max(total, 1))) ||
        (rc = lc->dirs.ensure((size_t)n_angles)))
        return rc;
    HIP_TRY(hipMemcpyAsync(lc->scans_dev.p, hs.data(), sizeof(YmScanRef) * n_queries, hipMemcpyHostToDevice, st));
    HIP_TRY(hipMemcpyAsync(lc->dirs.p, dir_cs, sizeof(double) * 2 * n_angles, hipMemcpyHostToDevice, st));
    HIP_TRY(hipMemsetAsync(lc->d_item.p, 0, sizeof(YmItemState), st));
    ym::MapPointsArgs pa;
    pa.scans = reinterpret_cast<const YmScanRef *>(lc->scans_dev.p); pa.n_scans = n_queries; pa.max_n = max_n;
    pa.ox_real = ox_real; pa.oy_real = oy_real; pa.out = lc->pts.p; pa.state = lc->d_item.p;
    (void)hipFuncSetAttribute(reinterpret_cast<const void *>(ym::map_points_kernel), hipFuncAttributeMaxDynamicSharedMemorySize,
                              (int)YM_PREP_LDS_BYTES(YM_MAX_BEAMS));
    hipLaunchKernelGGL(ym::map_points_kernel, dim3(1), dim3(1024), YM_PREP_LDS_BYTES(max_n), st, pa);
    HIP_TRY(hipGetLastError());
    int32_t n_points = 0;
    HIP_TRY(hipMemcpyAsync(&n_points, &lc->d_item.p->nq, sizeof n_points, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    if (n_points < 1 || n_points > total) return set_err(YM_ERR_INVALID, "the query scans hold no valid reading");
    const int stride = point_stride, nq = (n_points + stride - 1) / stride;
    if (nq > 65536) return set_err(YM_ERR_UNSUPPORTED, "%d points: at most 65536 (raise point_stride)", nq);
    if ((double)nq * n_angles * sizeof(uint32_t) > 1.0e9) return set_err(YM_ERR_UNSUPPORTED, "offset table of %d headings x %d points exceeds 1 GB", n_angles, nq);
    // ---- the offset table and the empty search state
    if ((rc = lc->offsets.ensure((size_t)nq * n_angles))) return rc;
    ym::LocState init;
    std::memset(&init, 0, sizeof init);
    init.tau = -1;
    HIP_TRY(hipMemcpyAsync(lc->d_state.p, &init, sizeof init, hipMemcpyHostToDevice, st));
    const double res = m->cfg.resolution;
    hipLaunchKernelGGL(ym::loc_offsets_kernel, dim3((unsigned)(((size_t)nq * n_angles + 255) / 256)), dim3(256), 0, st, lc->pts.p, stride, nq,
                       lc->dirs.p, n_angles, res, lc->offsets.p, lc->d_state.p);
    HIP_TRY(hipGetLastError());
    uint32_t bad = 0;
    HIP_TRY(hipMemcpyAsync(&bad, &lc->d_state.p->bad_offset, sizeof bad, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    if (bad) return set_err(YM_ERR_UNSUPPORTED, "a point lies more than 32767 cells from the set's centre");
    const double s_min_d = std::ceil(min_response * 100.0 * (double)nq);
    q->nq = nq; q->stride = stride;
    q->s_min = s_min_d > 2.0e9 ? INT32_MAX : (int32_t)s_min_d;
    return YM_OK;
}

// ---- one search: the top_k best hypotheses that are near no pick of `ex`, from an empty search state (tau and the top list
// start empty: nothing is carried from an earlier search; a search with picks resets the state itself).  Chunks of top-level nodes in (k, Y, X) order, each expanded level
// by level inside the frontier buffers.  sts gains this search's chunks and nodes; fin is the state read back at the end.
static int locator_search(ym_locator *lc, int n_angles, const LocQuery &q, int top_k, const LocExclude &ex, ym_locate_stats *sts_io, ym::LocState *fin_out) {
    ym_locate_stats &sts = *sts_io;
    ym::LocState &fin = *fin_out;
    const int W = lc->width, H = lc->height, L = lc->levels, nq = q.nq;
    const int32_t s_min = q.s_min;
    hipStream_t st = lc->m->stream;
    if (ex.n > 0) { // (the first search of a call finds the empty state locator_prepare left)
        ym::LocState init;
        std::memset(&init, 0, sizeof init);
        init.tau = -1;
        for (int e = 0; e < ex.n; e++) { init.excl[e][0] = ex.pick[e][0]; init.excl[e][1] = ex.pick[e][1]; init.excl[e][2] = ex.pick[e][2]; }
        HIP_TRY(hipMemcpyAsync(lc->d_state.p, &init, sizeof init, hipMemcpyHostToDevice, st));
    }
    const uint64_t side = 1ull << L;
    const uint64_t tx_n = ((uint64_t)W + side - 1) / side, ty_n = ((uint64_t)H + side - 1) / side, per = tx_n * ty_n;
    const uint64_t n_top_nodes = per * (uint64_t)n_angles, cells_per = (uint64_t)W * H;
    auto cells_before = [&](uint64_t t) { return (t / per) * cells_per + locator_cells_before(lc, t % per); };
    const uint32_t cap = (uint32_t)(lc->max_nodes + ym::kLocMaxTop);
    const size_t lds = (size_t)std::min(nq, ym::kLocTile) * sizeof(uint32_t);
    int known = 0; // entries of the device's top list
    uint32_t counters[2]; // n_out, overflow
    auto score_args = [&](int j, const uint64_t *in, uint32_t n, uint64_t *outp) {
        const LocLevelHost &lv = lc->level[j];
        ym::LocScoreArgs a;
        a.in = in; a.n_in = n; a.out = outp; a.out_cap = cap;
        a.offsets = lc->offsets.p; a.nq = nq;
        a.lvl = lv.p; a.pitch = lv.pitch; a.rows = lv.rows; a.margin = lv.margin;
        a.level = j; a.W = W; a.H = H; a.s_min = s_min; a.st = lc->d_state.p;
        a.n_excl = ex.n; a.sep_headings = ex.sep_headings; a.circular = ex.circular; a.n_angles = n_angles; a.sep_cells2 = ex.sep_cells2;
        return a;
    };
    // the `want` largest of n unique keys, ranked, into the list `dest` names (loc_sel_rank_kernel)
    auto select = [&](const uint64_t *keys, uint32_t n, uint32_t want, int dest) {
        const unsigned blocks = std::min<unsigned>((n + 255) / 256, 2048u);
        for (int shift = 56; shift >= 0; shift -= 8) {
            hipLaunchKernelGGL(ym::loc_sel_hist_kernel, dim3(blocks), dim3(256), 0, st, keys, n, shift, lc->d_state.p);
            hipLaunchKernelGGL(ym::loc_sel_pick_kernel, dim3(1), dim3(64), 0, st, shift, want, lc->d_state.p);
        }
        hipLaunchKernelGGL(ym::loc_sel_collect_kernel, dim3(blocks), dim3(256), 0, st, keys, n, lc->d_state.p);
        hipLaunchKernelGGL(ym::loc_sel_rank_kernel, dim3(1), dim3(64), 0, st, top_k, dest, lc->d_state.p);
    };
    for (uint64_t t0 = 0; t0 < n_top_nodes;) {
        uint64_t lo = t0 + 1, hi = n_top_nodes; // the largest t1 with cells [t0, t1) <= max_nodes (t0 + 1 always fits: checked at create)
        const uint64_t c0 = cells_before(t0);
        while (lo < hi) {
            const uint64_t mid = lo + (hi - lo + 1) / 2;
            if (cells_before(mid) - c0 <= (uint64_t)lc->max_nodes) lo = mid; else hi = mid - 1;
        }
        const uint64_t t1 = lo;
        uint32_t n = (uint32_t)(t1 - t0);
        sts.chunks++;
        hipLaunchKernelGGL(ym::loc_top_nodes_kernel, dim3((n + 255) / 256), dim3(256), 0, st, t0, n, (uint32_t)tx_n, (uint32_t)ty_n, L, lc->d_front[0].p);
        // ---- the probe: a beam of the kLocMaxTop best-bounded nodes followed down to level 0, where its top_k best exact scores
        // raise tau before the exact pass starts (without it a chunk's first leaves are reached with nothing pruned)
        if (L > 0) {
            const uint64_t *pin = lc->d_front[0].p;
            uint32_t pn = n;
            for (int j = L; j >= 0 && pn > 0; j--) {
                ym::loc_launch_score<2>(score_args(j, pin, pn, lc->d_front[1].p), lds, st);
                sts.probe_nodes += pn;
                select(lc->d_front[1].p, pn, std::min<uint32_t>(j == 0 ? (uint32_t)top_k : (uint32_t)ym::kLocMaxTop, pn), j == 0 ? 2 : 1);
                HIP_TRY(hipGetLastError());
                if (j == 0) break;
                uint64_t *next = lc->d_beam.p + (size_t)((L - j) & 1) * 4 * ym::kLocMaxTop;
                hipLaunchKernelGGL(ym::loc_probe_expand_kernel, dim3(1), dim3(64), 0, st, lc->d_state.p, pin, j, W, H, next);
                HIP_TRY(hipMemcpyAsync(counters, &lc->d_state.p->n_out, sizeof counters, hipMemcpyDeviceToHost, st));
                HIP_TRY(hipStreamSynchronize(st));
                if (counters[0] > 4u * ym::kLocMaxTop) return set_err(YM_ERR_UNSUPPORTED, "the probe's beam outgrew its buffer (a defect: please report)");
                pin = next;
                pn = counters[0];
            }
        }
        // ---- the exact pass
        int cur = 0;
        for (int j = L; j >= 0 && n > 0; j--) {
            const ym::LocScoreArgs a = score_args(j, lc->d_front[cur].p, n, lc->d_front[cur ^ 1].p);
            hipLaunchKernelGGL(ym::loc_begin_kernel, dim3(1), dim3(64), 0, st, lc->d_state.p, a.out, j == 0 ? 1 : 0);
            if (j > 0) ym::loc_launch_score<0>(a, lds, st);
            else ym::loc_launch_score<1>(a, lds, st);
            HIP_TRY(hipGetLastError());
            HIP_TRY(hipMemcpyAsync(counters, &lc->d_state.p->n_out, sizeof counters, hipMemcpyDeviceToHost, st));
            HIP_TRY(hipStreamSynchronize(st));
            if (counters[1] || counters[0] > cap) return set_err(YM_ERR_UNSUPPORTED, "the frontier outgrew its buffers at level %d (a defect: please report)", j);
            sts.nodes[j] += n;
            n = counters[0];
            cur ^= 1;
            if (j == 0 && n > (uint32_t)known) { // new leaves beside the `known` best so far: the best top_k of all
                known = (int)std::min<uint32_t>((uint32_t)top_k, n);
                select(lc->d_front[cur].p, n, (uint32_t)known, 0);
                HIP_TRY(hipGetLastError());
            }
        }
        t0 = t1;
    }
    HIP_TRY(hipMemcpyAsync(&fin, lc->d_state.p, sizeof fin, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    if (fin.n_top != known || fin.n_top > top_k) return set_err(YM_ERR_UNSUPPORTED, "the top-K merge kept %d of %d candidates (a defect: please report)", fin.n_top, known);
    return YM_OK;
}

// a key of the top list as the candidate the calls return
static ym_locate_candidate locator_candidate(const ym_locator *lc, uint64_t key, double ox, double oy, const double *dir_cs, int nq) {
    const uint64_t index = ym::kLocIndexMask - (key & ym::kLocIndexMask), cells_per = (uint64_t)lc->width * lc->height;
    const double res = lc->m->cfg.resolution;
    ym_locate_candidate c;
    std::memset(&c, 0, sizeof c);
    c.score = (int32_t)(key >> 40);
    c.index = (int64_t)index;
    c.k = (int32_t)(index / cells_per);
    c.cy = (int32_t)((index % cells_per) / (uint64_t)lc->width);
    c.cx = (int32_t)(index % (uint64_t)lc->width);
    c.response = (double)c.score / (100.0 * (double)nq);
    c.pose[0] = ox + c.cx * res; c.pose[1] = oy + c.cy * res;
    c.pose[2] = std::atan2(dir_cs[2 * c.k + 1], dir_cs[2 * c.k]);
    return c;
}

// the nq points the search used, read back for points_out
static int locator_read_points(ym_locator *lc, const LocQuery &q, std::vector<double> *pts_host) {
    pts_host->resize((size_t)2 * q.nq);
    HIP_TRY(hipMemcpy2D(pts_host->data(), sizeof(double2), lc->pts.p, sizeof(double2) * q.stride, sizeof(double2), q.nq, hipMemcpyDeviceToHost));
    return YM_OK;
}

int ym_locator_locate(ym_locator *lc, double ox, double oy, const ym_scan *const *queries, int n_queries, const double *dir_cs, int n_angles,
                      const ym_locate_opts *opts, ym_locate_candidate *out, int *n_found, double *points_out, ym_locate_stats *stats) {
    if (!lc || !queries || !dir_cs || !out || !n_found) return set_err(YM_ERR_INVALID, "null argument");
    ym_locate_opts o;
    if (opts) o = *opts;
    else { o.top_k = 16; o.point_stride = 1; o.min_response = 0.0; }
    if (o.top_k < 1 || o.top_k > ym::kLocMaxTop) return set_err(YM_ERR_INVALID, "top_k = %d: 1 .. %d", o.top_k, ym::kLocMaxTop);
    LocQuery q;
    int rc;
    DEV_GUARD(lc->device);
    if ((rc = locator_prepare(lc, queries, n_queries, dir_cs, n_angles, o.point_stride, o.min_response, &q))) return rc;
    ym_locate_stats sts;
    std::memset(&sts, 0, sizeof sts);
    sts.nq = q.nq;
    ym::LocState fin;
    if ((rc = locator_search(lc, n_angles, q, o.top_k, LocExclude(), &sts, &fin))) return rc;
    std::vector<double> pts_host;
    if (points_out && (rc = locator_read_points(lc, q, &pts_host))) return rc;
    // ---- everything succeeded: the outputs
    for (int i = 0; i < fin.n_top; i++) out[i] = locator_candidate(lc, fin.top[i], ox, oy, dir_cs, q.nq);
    *n_found = fin.n_top;
    if (points_out) std::memcpy(points_out, pts_host.data(), sizeof(double) * pts_host.size());
    if (stats) {
        for (int j = 0; j <= ym::kLocMaxLevels; j++) sts.survivors[j] = (int64_t)fin.survivors[j];
        *stats = sts;
    }
    return YM_OK;
}

// ---- the n_places best places: place i + 1 is the best hypothesis near none of places 1 .. i, one search each
int ym_locator_locate_places(ym_locator *lc, double ox, double oy, const ym_scan *const *queries, int n_queries, const double *dir_cs, int n_angles,
                             const ym_locate_places_opts *opts, ym_locate_candidate *out, int *n_found, double *points_out,
                             ym_locate_places_stats *stats) {
    if (!lc || !queries || !dir_cs || !opts || !out || !n_found) return set_err(YM_ERR_INVALID, "null argument");
    const ym_locate_places_opts o = *opts;
    if (o.n_places < 1 || o.n_places > ym::kLocMaxExcl + 1) return set_err(YM_ERR_INVALID, "n_places = %d: 1 .. %d", o.n_places, ym::kLocMaxExcl + 1);
    if (o.sep_cells2 < 0 || o.sep_headings < 0) return set_err(YM_ERR_INVALID, "a separation must be >= 0");
    if (o.circular != 0 && o.circular != 1) return set_err(YM_ERR_INVALID, "circular = %d: 0 or 1", o.circular);
    LocQuery q;
    int rc;
    DEV_GUARD(lc->device);
    if ((rc = locator_prepare(lc, queries, n_queries, dir_cs, n_angles, o.point_stride, o.min_response, &q))) return rc;
    ym_locate_places_stats ps;
    std::memset(&ps, 0, sizeof ps);
    ps.nq = q.nq;
    LocExclude ex;
    ex.sep_cells2 = o.sep_cells2; ex.sep_headings = o.sep_headings; ex.circular = o.circular;
    std::vector<ym_locate_candidate> found;
    while ((int)found.size() < o.n_places) { // at most 16 searches
        ym_locate_stats sts;
        std::memset(&sts, 0, sizeof sts);
        ym::LocState fin;
        ex.n = (int)found.size();
        if ((rc = locator_search(lc, n_angles, q, 1, ex, &sts, &fin))) return rc;
        int64_t scored = sts.probe_nodes;
        for (int j = 0; j <= ym::kLocMaxLevels; j++) scored += sts.nodes[j];
        ps.round_nodes[ps.rounds++] = scored;
        ps.chunks += sts.chunks; ps.nodes += scored - sts.probe_nodes; ps.probe_nodes += sts.probe_nodes;
        ps.excluded_leaves += (int64_t)fin.excluded_leaves; ps.excluded_nodes += (int64_t)fin.excluded_nodes;
        if (fin.n_top < 1) break; // no hypothesis is left
        const ym_locate_candidate c = locator_candidate(lc, fin.top[0], ox, oy, dir_cs, q.nq);
        if (ex.n < ym::kLocMaxExcl) { ex.pick[ex.n][0] = c.k; ex.pick[ex.n][1] = c.cx; ex.pick[ex.n][2] = c.cy; }
        found.push_back(c);
    }
    std::vector<double> pts_host;
    if (points_out && (rc = locator_read_points(lc, q, &pts_host))) return rc;
    // ---- everything succeeded: the outputs
    for (size_t i = 0; i < found.size(); i++) out[i] = found[i];
    *n_found = (int)found.size();
    if (points_out) std::memcpy(points_out, pts_host.data(), sizeof(double) * pts_host.size());
    if (stats) *stats = ps;
    return YM_OK;
}

void ym_locator_destroy(ym_locator *lc) {
    if (!lc) return;
    DevGuard guard(lc->device);
    delete lc;
}
