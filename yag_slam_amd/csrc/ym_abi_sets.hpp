// ym_abi_sets.hpp -- C ABI: several query scans matched as one point set against a chain of base scans, one item (ym_match_sets) or
// many in one enqueue (ym_match_sets_many).  DESIGN.md section 18.
// Part of yagmatch.hip (included inside its extern "C" block); not a header of its own.

// The grids of one chunk of a set batch: G x G bytes per item (with the reference's default configuration 4051 x 4051 = 16.4 MB)
static const size_t kSetsGridScratchBytes = (size_t)512 << 20;

int ym_match_sets_many(ym_matcher *m, const ym_scan *const *queries, const int32_t *set_offsets, const ym_scan *const *base,
                       const int32_t *chain_offsets, int n_items, int penalize, int refine, ym_result *results) {
    if (!m || !queries || !set_offsets || !base || !chain_offsets || !results) return set_err(YM_ERR_INVALID, "null argument");
    if (n_items <= 0 || n_items > (1 << 20)) return set_err(YM_ERR_INVALID, "n_items must be in [1, 2^20], negative or zero counts are refused");
    if (set_offsets[0] < 0 || chain_offsets[0] < 0) return set_err(YM_ERR_INVALID, "set_offsets[0] or chain_offsets[0] is negative");
    for (int b = 0; b < n_items; b++) {
        const int nq = set_offsets[b + 1] - set_offsets[b], nb = chain_offsets[b + 1] - chain_offsets[b];
        if (nq <= 0) return set_err(YM_ERR_INVALID, "item %d: an empty set (a set holds 1 to 64 scans, not %d)", b, nq);
        if (nq > 64) return set_err(YM_ERR_INVALID, "item %d: a set holds 1 to 64 scans, not %d", b, nq);
        if (nb < 0) return set_err(YM_ERR_INVALID, "item %d: a negative chain length %d", b, nb);
    }
    if (m->cfg.semantics != YM_SEM_YAGPY)
        return set_err(YM_ERR_UNSUPPORTED, "match_scan_sets exists only in the reference's Python matcher: create the matcher with YM_SEM_YAGPY");
    const int q0 = set_offsets[0], c0s = chain_offsets[0];
    const int n_qscans = set_offsets[n_items] - q0, n_bscans = chain_offsets[n_items] - c0s;
    // per item, as scan_matching.py:68-74: the centre is the mean of the query positions (Python's left-to-right sum), heading 0; the
    // grid's corner lies (G - 1) / 2 cells below it; the view-point of the base scans' filter is the LAST query's position (:72-80)
    const YmGeom &g = m->geom;
    const int G = g.roi_w;
    const double res = m->cfg.resolution;
    std::vector<ym::MapItemDesc> items((size_t)n_items);
    std::vector<double> origin((size_t)2 * n_items), view((size_t)2 * n_items);
    int max_nq = 1, max_nb = 1, rc;
    size_t total_pts = 0;
    for (int b = 0; b < n_items; b++) {
        const int lo = set_offsets[b], nq = set_offsets[b + 1] - lo;
        if ((rc = yag_item_desc(m, queries, q0, lo, nq, b, &items[b], &total_pts, &max_nq))) return rc;
        for (int i = chain_offsets[b]; i < chain_offsets[b + 1]; i++) {
            const ym_scan *s = base[i];
            if (!s || s->device != m->device) return set_err(YM_ERR_INVALID, "item %d: base scan %d is null or lives on another device", b, i - chain_offsets[b]);
            max_nb = std::max(max_nb, s->n);
        }
        origin[2 * (size_t)b] = items[b].ox_real - 0.5 * (G - 1) * res;
        origin[2 * (size_t)b + 1] = items[b].oy_real - 0.5 * (G - 1) * res;
        view[2 * (size_t)b] = queries[lo + nq - 1]->pose[0];
        view[2 * (size_t)b + 1] = queries[lo + nq - 1]->pose[1];
    }
    if (max_nq > YM_MAX_BEAMS || max_nb > YM_MAX_BEAMS)
        return set_err(YM_ERR_UNSUPPORTED, "scan has %d readings; limit is %d", std::max(max_nq, max_nb), YM_MAX_BEAMS);
    const int ks = 2 * g.half_kernel + 1;
    if ((double)G * G > 1.0e9) return set_err(YM_ERR_UNSUPPORTED, "a grid of %d x %d cells per item: at most 10^9", G, G);
    if ((rc = map_launch_limits(max_nb, ks, false))) return rc;
    // find_best_pose's arguments (scan_matching.py:100-108); the padded lattice holds np.arange's lengths of both passes
    YagBatch S;
    std::memset(&S, 0, sizeof S);
    S.coarse.xy_search = m->cfg.search_size * 0.5; S.coarse.xy_step = res * 2;
    S.coarse.angle_search = m->cfg.coarse_search_angle_offset * 0.5; S.coarse.angle_step = m->cfg.coarse_angle_resolution;
    S.coarse.grid_resolution = res; S.coarse.penalize = penalize;
    if ((rc = yag_lattice_bound(S.coarse, res, "", &S.L))) return rc;
    const size_t vol = S.L.vol;
    const size_t grid_stride = align_up((size_t)G * G + 64, 256);
    const bool keep_all = n_items <= kMapKeepSumsItems;
    int chunk = (int)std::min<size_t>((size_t)n_items, std::max<size_t>(1, kMapBatchScratchBytes / (16 * vol)));
    chunk = (int)std::min<size_t>((size_t)chunk, std::max<size_t>(1, kSetsGridScratchBytes / grid_stride));
    if (m->sets_chunk_forced > 0) chunk = std::min(n_items, m->sets_chunk_forced);
    const size_t sums_items = keep_all ? (size_t)n_items : (size_t)chunk;
    // the (base scan, item of its chunk) pairs, item by item: a chunk's are consecutive
    std::vector<int32_t> job_begin((size_t)n_items + 1);
    const size_t n_jobs = (size_t)n_bscans;
    DEV_GUARD(m->device);
    Slot &slot = m->slots[kAsyncSlots];
    if (slot.in_flight) return set_err(YM_ERR_BUSY, "the synchronous slot is in flight");
    if ((rc = m->states.ensure((size_t)n_items)) || (rc = m->map_pts.ensure(total_pts)) || (rc = m->yaxes.ensure((size_t)chunk * 3 * YM_YAG_MAX_DIM)) ||
        (rc = m->sums.ensure(2 * sums_items * vol)) || (rc = m->resp.ensure((size_t)chunk * vol)) ||
        (rc = m->sets_grid.ensure((size_t)chunk * grid_stride)) || (rc = m->sets_ktab.ensure((size_t)ks * ks)) || (rc = yag_counters_ensure(m)))
        return rc;
    const size_t qscans_bytes = align_up(sizeof(YmScanRef) * (size_t)n_qscans, 16);
    const size_t bscans_bytes = align_up(sizeof(YmScanRef) * (size_t)std::max(n_bscans, 1), 16);
    const size_t items_bytes = align_up(sizeof(ym::MapItemDesc) * (size_t)n_items, 16);
    const size_t view_bytes = sizeof(double2) * (size_t)n_items;
    const size_t jobs_bytes = align_up(sizeof(int2) * std::max<size_t>(n_jobs, 1), 16);
    const size_t ktab_bytes = align_up((size_t)ks * ks, 16);
    const size_t desc_bytes = qscans_bytes + bscans_bytes + items_bytes + view_bytes + jobs_bytes + ktab_bytes;
    const size_t states_bytes = sizeof(YmItemState) * (size_t)n_items;
    if ((rc = slot.desc.ensure(desc_bytes + states_bytes)) || (rc = slot.result.ensure(states_bytes)) || (rc = m->sets_desc.ensure(desc_bytes)))
        return rc;
    slot.desc_live_bytes = 0; // (the slot's pinned descriptor buffer is rewritten here)
    unsigned char *hd = slot.desc.p;
    std::memset(hd, 0, desc_bytes);
    YmScanRef *hq = reinterpret_cast<YmScanRef *>(hd);
    YmScanRef *hb = reinterpret_cast<YmScanRef *>(hd + qscans_bytes);
    double2 *hv = reinterpret_cast<double2 *>(hd + qscans_bytes + bscans_bytes + items_bytes);
    int2 *hj = reinterpret_cast<int2 *>(hd + qscans_bytes + bscans_bytes + items_bytes + view_bytes);
    for (int i = 0; i < n_qscans; i++) hq[i] = scan_ref(queries[q0 + i]);
    for (int i = 0; i < n_bscans; i++) hb[i] = scan_ref(base[c0s + i]);
    std::memcpy(hd + qscans_bytes + bscans_bytes, items.data(), sizeof(ym::MapItemDesc) * (size_t)n_items);
    {
        size_t j = 0;
        for (int b = 0; b < n_items; b++) {
            hv[b] = make_double2(view[2 * (size_t)b], view[2 * (size_t)b + 1]);
            job_begin[b] = (int32_t)j;
            for (int i = chain_offsets[b]; i < chain_offsets[b + 1]; i++, j++) hj[j] = make_int2(i - c0s, b % chunk);
        }
        job_begin[n_items] = (int32_t)j;
    }
    std::memcpy(hd + desc_bytes - ktab_bytes, m->kernel.data(), (size_t)ks * ks);
    YmItemState *st0 = reinterpret_cast<YmItemState *>(hd + desc_bytes);
    yag_init_states(m, items, origin.data(), 2, st0);
    hipStream_t st = m->stream;
    unsigned char *dd = m->sets_desc.p;
    // ym_profile_read: 0 = the integer sums of both passes (yag_map_kernel or the pair-by-pair kernel), 1 = the grids (clearing and
    // sets_grid_kernel), 2 = the whole call on the device
    hipEvent_t ev_call = nullptr, ev_k = nullptr;
    if ((rc = prof_begin(m, 2, &ev_call))) return rc;
    HIP_TRY(hipMemcpyAsync(dd, hd, desc_bytes, hipMemcpyHostToDevice, st));
    HIP_TRY(hipMemcpyAsync(m->states.p, st0, states_bytes, hipMemcpyHostToDevice, st));
    HIP_TRY(hipMemcpyAsync(m->sets_ktab.p, hd + desc_bytes - ktab_bytes, (size_t)ks * ks, hipMemcpyHostToDevice, st));
    (void)hipFuncSetAttribute(reinterpret_cast<const void *>(ym::sets_grid_kernel<256>), hipFuncAttributeMaxDynamicSharedMemorySize,
                              (int)YM_PREP_LDS_BYTES(YM_MAX_BEAMS));
    enqueue_map_points_many(m, reinterpret_cast<const YmScanRef *>(dd), reinterpret_cast<const ym::MapItemDesc *>(dd + qscans_bytes + bscans_bytes),
                            n_items, max_nq);
    ym::SetsGridArgs ga;
    std::memset(&ga, 0, sizeof ga);
    ga.scans = reinterpret_cast<const YmScanRef *>(dd + qscans_bytes);
    ga.max_n = max_nb; ga.G = G; ga.res = res; ga.ktab = m->sets_ktab.p; ga.ksize = ks;
    ga.grid = m->sets_grid.p; ga.grid_stride = grid_stride;
    S.grid = m->sets_grid.p; S.grid_stride = grid_stride; S.map_w = G; S.map_h = G; S.map_sets = 1; // (the states carry each grid's origin)
    S.penalize = penalize; S.refine = refine; S.sums_items = sums_items; S.keep_all = keep_all;
    S.need_fast = true; S.fallback = &m->sets_fallback_host; S.profile = true; // option 46 = 0 leaves every item to the rule as written
    const int passes = refine ? 2 : 1;
    int first_kept = 0, first_grid = 0;
    for (int c0 = 0; c0 < n_items; c0 += chunk) {
        const int B = std::min(chunk, n_items - c0);
        first_kept = keep_all ? 0 : c0;
        first_grid = c0;
        // the chunk's grids: zeroed, then every (base scan, item) pair stamps its kept readings
        if ((rc = prof_begin(m, 1, &ev_k))) return rc;
        HIP_TRY(hipMemsetAsync(m->sets_grid.p, 0, (size_t)B * grid_stride, st));
        const int nj = job_begin[c0 + B] - job_begin[c0];
        if (nj > 0) {
            ga.jobs = reinterpret_cast<const int2 *>(dd + qscans_bytes + bscans_bytes + items_bytes + view_bytes) + job_begin[c0];
            ga.view = reinterpret_cast<const double2 *>(dd + qscans_bytes + bscans_bytes + items_bytes) + c0;
            ga.states = m->states.p + c0;
            // a few jobs alone leave the device empty: up to eight blocks share a job's rows of taps until about four blocks per CU exist
            const int share = std::max(1, std::min(8, 1024 / nj));
            hipLaunchKernelGGL(ym::sets_grid_kernel<256>, dim3(nj, share), dim3(256), YM_PREP_LDS_BYTES(max_nb), st, ga);
        }
        if ((rc = prof_end(m, ev_k))) return rc;
        for (int pass = 0; pass < passes; pass++)
            if ((rc = enqueue_yag_batch_pass(m, slot, S, c0, B, pass))) return rc;
    }
    if ((rc = prof_end(m, ev_call))) return rc;
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipStreamSynchronize(st));
    const YmItemState *rs = reinterpret_cast<const YmItemState *>(slot.result.p);
    for (int b = 0; b < n_items; b++) yag_unpack_result(rs[b], refine, results + b);
    // the debug getters describe this call: the sums through map_last, grids and query points through sets_last
    map_last_set(m, n_items, first_kept, passes, vol, sums_items * vol);
    m->sets_last.valid = true; m->sets_last.G = G; m->sets_last.first_grid = first_grid; m->sets_last.grid_stride = grid_stride;
    return YM_OK;
}

int ym_match_sets(ym_matcher *m, const ym_scan *const *queries, int n_queries, const ym_scan *const *base, int n_base, int penalize,
                  int refine, ym_result *out) {
    if (!m || !queries || !base || !out) return set_err(YM_ERR_INVALID, "null argument");
    if (n_queries <= 0) return set_err(YM_ERR_INVALID, "an empty set (a set holds 1 to 64 scans, not %d)", n_queries);
    if (n_queries > 64) return set_err(YM_ERR_INVALID, "a set holds 1 to 64 scans, not %d", n_queries);
    if (n_base < 0) return set_err(YM_ERR_INVALID, "n_base must not be negative");
    const int32_t so[2] = {0, n_queries}, co[2] = {0, n_base};
    return ym_match_sets_many(m, queries, so, base, co, 1, penalize, refine, out);
}
