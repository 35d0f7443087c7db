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
    int max_n = 1, rc;
    size_t total_pts = 0;
    const int s0 = set_offsets[0];
    for (int b = 0; b < n_items; b++) {
        const int lo = set_offsets[b], nq = set_offsets[b + 1] - lo;
        if (nq <= 0 || nq > 64) return set_err(YM_ERR_INVALID, "item %d: a set holds 1 to 64 scans, not %d", b, nq);
        if ((rc = yag_item_desc(m, queries, s0, lo, nq, b, &items[b], &total_pts, &max_n))) return rc;
    }
    const int n_scans = set_offsets[n_items] - s0;
    YagBatch S;
    std::memset(&S, 0, sizeof S);
    if ((rc = map_search_params(coarse, &S.coarse)) || (rc = yag_lattice_bound(S.coarse, m->cfg.resolution, "map ", &S.L))) return rc;
    const size_t vol = S.L.vol;
    const bool keep_all = n_items <= kMapKeepSumsItems;
    int chunk = (int)std::min<size_t>((size_t)n_items, std::max<size_t>(1, kMapBatchScratchBytes / (16 * vol)));
    if (m->map_chunk_forced > 0) chunk = std::min(n_items, m->map_chunk_forced);
    const size_t sums_items = keep_all ? (size_t)n_items : (size_t)chunk;
    Slot &slot = m->slots[kAsyncSlots];
    if (slot.in_flight) return set_err(YM_ERR_BUSY, "the synchronous slot is in flight");
    if ((rc = m->states.ensure((size_t)n_items)) || (rc = m->map_pts.ensure(total_pts)) || (rc = m->yaxes.ensure((size_t)chunk * 3 * YM_YAG_MAX_DIM)) ||
        (rc = m->sums.ensure(2 * sums_items * vol)) || (rc = m->resp.ensure((size_t)chunk * vol)) || (rc = yag_counters_ensure(m)))
        return rc;
    const size_t scans_bytes = align_up(sizeof(YmScanRef) * (size_t)n_scans, 16);
    const size_t items_bytes = align_up(sizeof(ym::MapItemDesc) * (size_t)n_items, 16);
    const size_t states_bytes = sizeof(YmItemState) * (size_t)n_items;
    if ((rc = slot.desc.ensure(scans_bytes + items_bytes + states_bytes)) || (rc = slot.result.ensure(states_bytes)) ||
        (rc = m->desc_dev.ensure(scans_bytes + items_bytes)))
        return rc;
    slot.desc_live_bytes = 0; // (the slot's pinned descriptor buffer is rewritten here)
    YmScanRef *hs = reinterpret_cast<YmScanRef *>(slot.desc.p);
    std::memset(hs, 0, scans_bytes);
    for (int i = 0; i < n_scans; i++) hs[i] = scan_ref(queries[s0 + i]);
    std::memcpy(slot.desc.p + scans_bytes, items.data(), sizeof(ym::MapItemDesc) * (size_t)n_items);
    YmItemState *st0 = reinterpret_cast<YmItemState *>(slot.desc.p + scans_bytes + items_bytes);
    const double origin[2] = {ox, oy};
    yag_init_states(m, items, origin, 0, st0);
    hipStream_t st = m->stream;
    HIP_TRY(hipMemcpyAsync(m->desc_dev.p, slot.desc.p, scans_bytes + items_bytes, hipMemcpyHostToDevice, st));
    HIP_TRY(hipMemcpyAsync(m->states.p, st0, states_bytes, hipMemcpyHostToDevice, st));
    enqueue_map_points_many(m, reinterpret_cast<const YmScanRef *>(m->desc_dev.p),
                            reinterpret_cast<const ym::MapItemDesc *>(m->desc_dev.p + scans_bytes), n_items, max_n);
    S.grid = mp->d_g8.p; S.grid_stride = 0; S.map_w = mp->width; S.map_h = mp->height; S.map_ox = ox; S.map_oy = oy;
    S.penalize = penalize; S.refine = refine; S.sums_items = sums_items; S.keep_all = keep_all;
    S.fallback = &m->map_fallback_host; // (need_fast, profile: no -- option 46 and the profiler are the set matcher's)
    const int passes = refine ? 2 : 1;
    int first_kept = 0;
    for (int c0 = 0; c0 < n_items; c0 += chunk) {
        const int B = std::min(chunk, n_items - c0);
        first_kept = keep_all ? 0 : c0;
        for (int pass = 0; pass < passes; pass++)
            if ((rc = enqueue_yag_batch_pass(m, slot, S, c0, B, pass))) return rc;
    }
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipStreamSynchronize(st));
    const YmItemState *rs = reinterpret_cast<const YmItemState *>(slot.result.p);
    for (int b = 0; b < n_items; b++) yag_unpack_result(rs[b], refine, results + b);
    map_last_set(m, n_items, first_kept, passes, vol, sums_items * vol);
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
