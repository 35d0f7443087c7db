// ym_abi_maptrack.hpp -- C ABI: localization mode.  N independent scan sets against one resident map in one enqueue
// (ym_match_map_many), scan streams followed through the map step by step (ym_map_track).  DESIGN.md section 13.
// Part of yagmatch.hip (included inside its extern "C" block); not a header of its own.

// Scratch of one chunk of a map batch: per item a score volume (fp64) and, unless the whole call keeps its sums, the two sum
// volumes (uint32): 16 bytes per hypothesis of the padded lattice, about 1 MB per item with the reference's constants.
static const size_t kMapBatchScratchBytes = (size_t)256 << 20;
// calls of up to this many items keep the integer sums of every item for ym_debug_map_sums; larger ones those of their last chunk
static const int kMapKeepSumsItems = 128;

int ym_match_map_many(ym_matcher *m, const ym_map *mp, double ox, double oy, const ym_scan *const *queries, const int32_t *set_offsets,
                      int n_items, int penalize, int refine, const ym_map_search *coarse, ym_result *results) {
    if (!m || !mp || !queries || !set_offsets || !results) return set_err(YM_ERR_INVALID, "null argument");
    if (m->cfg.semantics != YM_SEM_YAGPY) return set_err(YM_ERR_UNSUPPORTED, "ym_match_map_many needs a YM_SEM_YAGPY matcher");
    if (n_items <= 0 || n_items > (1 << 20)) return set_err(YM_ERR_INVALID, "n_items must be in [1, 2^20]");
    if (mp->device != m->device) return set_err(YM_ERR_INVALID, "map lives on another device");
    if (set_offsets[0] < 0) return set_err(YM_ERR_INVALID, "set_offsets[0] is negative");
    DEV_GUARD(m->device);
    // per item, exactly as ym_match_map: the search centre is the mean of the query poses (Python's left-to-right sum), heading 0
    std::vector<ym::MapItemDesc> items((size_t)n_items);
    int max_n = 1;
    size_t total_pts = 0;
    const int s0 = set_offsets[0];
    for (int b = 0; b < n_items; b++) {
        const int lo = set_offsets[b], nq = set_offsets[b + 1] - lo;
        if (nq <= 0 || nq > 64) return set_err(YM_ERR_INVALID, "item %d: a set holds 1 to 64 scans, not %d", b, nq);
        double sx = 0, sy = 0;
        int total = 0;
        for (int i = 0; i < nq; i++) {
            const ym_scan *q = queries[lo + i];
            if (!q || q->device != m->device) return set_err(YM_ERR_INVALID, "item %d: query %d is null or lives on another device", b, i);
            sx = i == 0 ? q->pose[0] : sx + q->pose[0];
            sy = i == 0 ? q->pose[1] : sy + q->pose[1];
            total += q->n;
            max_n = std::max(max_n, q->n);
        }
        items[b].scan_begin = lo - s0; items[b].n_scans = nq;
        items[b].out_off = (int64_t)total_pts;
        items[b].ox_real = sx / (double)nq; items[b].oy_real = sy / (double)nq;
        total_pts += (size_t)std::max(total, 1);
    }
    const int n_scans = set_offsets[n_items] - s0;
    ym_map_search cs;
    if (coarse) cs = *coarse;
    else { cs.xy_search = 0.25; cs.xy_step = 0.01; cs.angle_search = 0.1; cs.angle_step = 0.01; cs.grid_resolution = 0.05; cs.penalize = 0; cs.reserved = 0; }
    if (!(cs.xy_step > 0) || !(cs.angle_step > 0) || !(cs.grid_resolution > 0) || !(cs.xy_search > 0) || !(cs.angle_search > 0))
        return set_err(YM_ERR_INVALID, "bad coarse search parameters");
    const double res = m->cfg.resolution;
    // (the padded lattice of ym_match_map: yag_setup_kernel clamps np.arange's lengths to it, so the two calls must agree on it)
    const int maxd = std::max({8, (int)std::ceil(2 * cs.xy_search / cs.xy_step) + 2, (int)std::ceil(4 * res / res) + 2});
    const int maxt = std::max({13, (int)std::ceil(2 * cs.angle_search / cs.angle_step) + 2});
    if (maxd > YM_YAG_MAX_DIM || maxt > YM_YAG_MAX_NT)
        return set_err(YM_ERR_UNSUPPORTED, "map search lattice %d x %d x %d exceeds the built-in limit", maxd, maxd, maxt);
    const size_t vol = (size_t)maxt * maxd * maxd;
    const bool keep_all = n_items <= kMapKeepSumsItems;
    int chunk = (int)std::min<size_t>((size_t)n_items, std::max<size_t>(1, kMapBatchScratchBytes / (16 * vol)));
    if (m->map_chunk_forced > 0) chunk = std::min(n_items, m->map_chunk_forced);
    const size_t sums_items = keep_all ? (size_t)n_items : (size_t)chunk;
    int rc;
    Slot &slot = m->slots[kAsyncSlots];
    if (slot.in_flight) return set_err(YM_ERR_BUSY, "the synchronous slot is in flight");
    if ((rc = m->states.ensure((size_t)n_items))) return rc;
    if ((rc = m->map_pts.ensure(total_pts))) return rc;
    if ((rc = m->yaxes.ensure((size_t)chunk * 3 * YM_YAG_MAX_DIM))) return rc;
    if ((rc = m->sums.ensure(2 * sums_items * vol))) return rc;
    if ((rc = m->resp.ensure((size_t)chunk * vol))) return rc;
    if (!m->yag_counters.p) {
        if ((rc = m->yag_counters.ensure(8))) return rc;
        HIP_TRY(hipMemsetAsync(m->yag_counters.p, 0, m->yag_counters.cap * sizeof(unsigned long long), m->stream));
    }
    const size_t scans_bytes = align_up(sizeof(YmScanRef) * (size_t)n_scans, 16);
    const size_t items_bytes = align_up(sizeof(ym::MapItemDesc) * (size_t)n_items, 16);
    const size_t states_bytes = sizeof(YmItemState) * (size_t)n_items;
    if ((rc = slot.desc.ensure(scans_bytes + items_bytes + states_bytes))) return rc;
    if ((rc = slot.result.ensure(states_bytes))) return rc;
    if ((rc = m->desc_dev.ensure(scans_bytes + items_bytes))) return rc;
    slot.desc_live_bytes = 0; // (the slot's pinned descriptor buffer is rewritten here)
    YmScanRef *hs = reinterpret_cast<YmScanRef *>(slot.desc.p);
    std::memset(hs, 0, scans_bytes);
    for (int i = 0; i < n_scans; i++) hs[i] = scan_ref(queries[s0 + i]);
    std::memcpy(slot.desc.p + scans_bytes, items.data(), sizeof(ym::MapItemDesc) * (size_t)n_items);
    YmItemState *st0 = reinterpret_cast<YmItemState *>(slot.desc.p + scans_bytes + items_bytes);
    std::memset(st0, 0, states_bytes);
    for (int b = 0; b < n_items; b++) {
        st0[b].pose[0] = st0[b].center[0] = items[b].ox_real; st0[b].pose[1] = st0[b].center[1] = items[b].oy_real;
        st0[b].off_x = ox; st0[b].off_y = oy;
        st0[b].ql = m->map_pts.p + items[b].out_off;
    }
    hipStream_t st = m->stream;
    HIP_TRY(hipMemcpyAsync(m->desc_dev.p, slot.desc.p, scans_bytes + items_bytes, hipMemcpyHostToDevice, st));
    HIP_TRY(hipMemcpyAsync(m->states.p, st0, states_bytes, hipMemcpyHostToDevice, st));
    ym::MapPointsManyArgs pa;
    std::memset(&pa, 0, sizeof pa);
    pa.scans = reinterpret_cast<const YmScanRef *>(m->desc_dev.p);
    pa.items = reinterpret_cast<const ym::MapItemDesc *>(m->desc_dev.p + scans_bytes);
    pa.max_n = max_n; pa.out = m->map_pts.p; pa.states = m->states.p;
    (void)hipFuncSetAttribute(reinterpret_cast<const void *>(ym::map_points_many_kernel), hipFuncAttributeMaxDynamicSharedMemorySize,
                              (int)YM_PREP_LDS_BYTES(YM_MAX_BEAMS));
    hipLaunchKernelGGL(ym::map_points_many_kernel, dim3(n_items), dim3(1024), YM_PREP_LDS_BYTES(max_n), st, pa);
    const int passes = refine ? 2 : 1;
    int first_kept = 0;
    for (int c0 = 0; c0 < n_items; c0 += chunk) {
        const int B = std::min(chunk, n_items - c0);
        first_kept = keep_all ? 0 : c0;
        for (int pass = 0; pass < passes; pass++) {
            ym::YagArgs a;
            std::memset(&a, 0, sizeof a);
            a.g = m->geom; a.pass = pass; a.refine = refine ? 1 : 0;
            a.last = (pass == 1 || !refine) ? 1 : 0;
            if (pass == 0) {
                a.search_xy = cs.xy_search; a.step_xy = cs.xy_step; a.search_t = cs.angle_search; a.step_t = cs.angle_step;
                a.map_res = cs.grid_resolution; a.penalize = cs.penalize ? 1 : 0;
            } else { // scan_matching.py:155-157
                a.search_xy = res * 2; a.step_xy = res; a.search_t = 0.0349 * 0.5; a.step_t = 0.00349;
                a.map_res = res; a.penalize = penalize ? 1 : 0;
            }
            a.coarse_angle_res = m->cfg.coarse_angle_resolution;
            a.states = m->states.p + c0; a.host_out = reinterpret_cast<YmItemState *>(slot.result.dp) + c0;
            a.axes = m->yaxes.p; a.rot = nullptr; // (the kernels rotate the points themselves: the same products and sums)
            a.sums = m->sums.p + (size_t)pass * sums_items * vol + (keep_all ? (size_t)c0 * vol : 0); a.out = m->resp.p;
            a.grid = mp->d_g8.p; a.grid_stride = 0; a.vol_stride = vol;
            a.max_n = 0; a.maxd = maxd; a.maxt = maxt; a.n_items = B;
            a.map_w = mp->width; a.map_h = mp->height; a.map_ox = ox; a.map_oy = oy;
            a.counters = m->yag_counters.p;
            // np.arange's length is within one of ceil(2 search / step): a pass whose every possible length fits yag_map_kernel's
            // limit needs no yag_score_kernel, one whose none does no yag_map_kernel; in between both run and the lengths decide
            const int est = (int)std::ceil(2 * a.search_xy / a.step_xy);
            const bool run_map = est - 1 <= YM_YAG_MAP_DIM, run_score = est + 1 > YM_YAG_MAP_DIM;
            a.map_dim = run_map ? YM_YAG_MAP_DIM : 0;
            // a few items alone leave the device empty: their (item, angle) blocks are split until about four blocks per CU exist
            const int split = std::max(1, std::min(32, 1024 / (B * maxt)));
            a.map_split = split;
            hipLaunchKernelGGL(ym::yag_setup_kernel, dim3(1, B), dim3(256), 0, st, a);
            if (run_map) {
                if (split > 1) HIP_TRY(hipMemsetAsync(a.sums, 0, (size_t)B * vol * sizeof(uint32_t), st));
                hipLaunchKernelGGL(ym::yag_map_kernel, dim3(8 * maxt * ((B + 7) / 8) * split), dim3(256), 0, st, a);
                if (split > 1) hipLaunchKernelGGL(ym::yag_map_score_kernel, dim3((maxd * maxd + 255) / 256, maxt, B), dim3(256), 0, st, a);
            } else if (pass == 0) m->map_fallback_host += B;
            if (run_score) hipLaunchKernelGGL(ym::yag_score_kernel, dim3((maxd * maxd + 255) / 256, maxt, B), dim3(256), 0, st, a);
            hipLaunchKernelGGL(ym::yag_reduce_kernel<1024>, dim3(B), dim3(1024), 0, st, a);
        }
    }
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipStreamSynchronize(st));
    const YmItemState *rs = reinterpret_cast<const YmItemState *>(slot.result.p);
    for (int b = 0; b < n_items; b++) {
        const YmItemState &r = rs[b];
        ym_result *out = results + b;
        std::memset(out, 0, sizeof *out);
        out->response = r.response;
        for (int i = 0; i < 3; i++) out->pose[i] = r.mean[i];
        for (int i = 0; i < 9; i++) out->cov[i] = r.cov[i];
        out->coarse_response = r.ybest[0][0];
        for (int i = 0; i < 3; i++) { out->coarse_dims[i] = r.ydims[0][i]; out->fine_dims[i] = refine ? r.ydims[1][i] : 0; }
        out->hypotheses = (int64_t)r.ydims[0][0] * r.ydims[0][1] * r.ydims[0][2] +
                          (refine ? (int64_t)r.ydims[1][0] * r.ydims[1][1] * r.ydims[1][2] : 0);
        out->n_query_points = r.nq;
        out->status = r.status;
    }
    m->last_valid = false; // the debug getters describe match_scan calls
    m->sets_last.valid = false;
    m->map_last.valid = true; m->map_last.n_items = n_items; m->map_last.first_kept = first_kept; m->map_last.passes = passes;
    m->map_last.vol = vol; m->map_last.pass_offset[0] = 0; m->map_last.pass_offset[1] = sums_items * vol;
    return YM_OK;
}

int ym_map_track(ym_matcher *m, const ym_map *mp, double ox, double oy, ym_scan *const *scans, const double *odom,
                 const int32_t *track_offsets, int n_tracks, int start, int penalize, int refine, const ym_map_search *coarse,
                 double min_response, ym_result *results, int32_t *n_done) {
    if (!m || !mp || !scans || !odom || !track_offsets || !results || !n_done) return set_err(YM_ERR_INVALID, "null argument");
    if (m->cfg.semantics != YM_SEM_YAGPY) return set_err(YM_ERR_UNSUPPORTED, "ym_map_track needs a YM_SEM_YAGPY matcher");
    if (n_tracks <= 0) return set_err(YM_ERR_INVALID, "n_tracks must be at least 1");
    if (start < 1) return set_err(YM_ERR_INVALID, "start must be at least 1: scan 0 of a track carries its pose");
    if (track_offsets[0] < 0) return set_err(YM_ERR_INVALID, "track_offsets[0] is negative");
    int longest = 0;
    for (int r = 0; r < n_tracks; r++) {
        const int len = track_offsets[r + 1] - track_offsets[r];
        if (len < 1) return set_err(YM_ERR_INVALID, "track %d is empty", r);
        for (int i = 0; i < len; i++)
            if (!scans[track_offsets[r] + i]) return set_err(YM_ERR_INVALID, "track %d: null scan %d", r, i);
        longest = std::max(longest, len);
    }
    for (int i = track_offsets[0]; i < track_offsets[n_tracks]; i++) std::memset(&results[i], 0, sizeof results[i]);
    std::vector<int> ended((size_t)n_tracks, 0);
    for (int r = 0; r < n_tracks; r++) n_done[r] = track_offsets[r + 1] - track_offsets[r];
    std::vector<const ym_scan *> step_scans;
    std::vector<int32_t> step_offsets, step_track;
    std::vector<ym_result> step_results;
    std::vector<double> priors;
    for (int i = start; i < longest; i++) {
        step_scans.clear(); step_track.clear(); priors.clear();
        step_offsets.assign(1, 0);
        for (int r = 0; r < n_tracks; r++) {
            const int lo = track_offsets[r], len = track_offsets[r + 1] - lo;
            if (ended[r] || i >= len) continue;
            // graph_slam.py:320-324: prior = last.corrected_pose + (query.odom_pose - last.odom_pose)
            double inv[3], diff[3], prior[3];
            tf_inverse(odom + 3 * (size_t)(lo + i - 1), inv);
            tf_compose(inv, odom + 3 * (size_t)(lo + i), diff);
            tf_compose(scans[lo + i - 1]->pose, diff, prior);
            int rc = ym_scan_set_pose(scans[lo + i], prior[0], prior[1], prior[2]);
            if (rc) return rc;
            step_scans.push_back(scans[lo + i]);
            step_offsets.push_back((int32_t)step_scans.size());
            step_track.push_back(r);
            priors.insert(priors.end(), prior, prior + 3);
        }
        if (step_scans.empty()) break;
        const int n = (int)step_scans.size();
        step_results.resize((size_t)n);
        int rc = ym_match_map_many(m, mp, ox, oy, step_scans.data(), step_offsets.data(), n, penalize, refine, coarse, step_results.data());
        if (rc) return rc;
        for (int j = 0; j < n; j++) {
            const int r = step_track[j], at = track_offsets[r] + i;
            ym_result &R = results[at];
            R = step_results[j];
            if (R.status != 0) { ended[r] = 1; n_done[r] = i; continue; } // (the scan keeps its prior)
            if (R.response < min_response) { R.reserved = 1; continue; }   // dead reckoning: the scan keeps its prior
            // one scan: the set's centre is the scan's own position, so the rigid motion of the set moves it to the corrected
            // centre and turns it by the correction's heading
            if ((rc = ym_scan_set_pose(scans[at], R.pose[0], R.pose[1], priors[3 * (size_t)j + 2] + R.pose[2]))) return rc;
        }
    }
    return YM_OK;
}
