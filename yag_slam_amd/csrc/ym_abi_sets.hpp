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
    int max_nq = 1, max_nb = 1;
    size_t total_pts = 0;
    for (int b = 0; b < n_items; b++) {
        const int lo = set_offsets[b], nq = set_offsets[b + 1] - lo;
        double sx = 0, sy = 0;
        int total = 0;
        for (int i = 0; i < nq; i++) {
            const ym_scan *q = queries[lo + i];
            if (!q || q->device != m->device) return set_err(YM_ERR_INVALID, "item %d: query %d is null or lives on another device", b, i);
            sx = i == 0 ? q->pose[0] : sx + q->pose[0];
            sy = i == 0 ? q->pose[1] : sy + q->pose[1];
            total += q->n;
            max_nq = std::max(max_nq, q->n);
        }
        for (int i = chain_offsets[b]; i < chain_offsets[b + 1]; i++) {
            const ym_scan *s = base[i];
            if (!s || s->device != m->device) return set_err(YM_ERR_INVALID, "item %d: base scan %d is null or lives on another device", b, i - chain_offsets[b]);
            max_nb = std::max(max_nb, s->n);
        }
        items[b].scan_begin = lo - q0; items[b].n_scans = nq;
        items[b].out_off = (int64_t)total_pts;
        items[b].ox_real = sx / (double)nq; items[b].oy_real = sy / (double)nq;
        origin[2 * (size_t)b] = items[b].ox_real - 0.5 * (G - 1) * res;
        origin[2 * (size_t)b + 1] = items[b].oy_real - 0.5 * (G - 1) * res;
        view[2 * (size_t)b] = queries[lo + nq - 1]->pose[0];
        view[2 * (size_t)b + 1] = queries[lo + nq - 1]->pose[1];
        total_pts += (size_t)std::max(total, 1);
    }
    if (max_nq > YM_MAX_BEAMS || max_nb > YM_MAX_BEAMS)
        return set_err(YM_ERR_UNSUPPORTED, "scan has %d readings; limit is %d", std::max(max_nq, max_nb), YM_MAX_BEAMS);
    const int ks = 2 * g.half_kernel + 1;
    if ((double)G * G > 1.0e9) return set_err(YM_ERR_UNSUPPORTED, "a grid of %d x %d cells per item: at most 10^9", G, G);
    if ((double)max_nb * ks * ks > 2.0e9) return set_err(YM_ERR_UNSUPPORTED, "%d beams x %d x %d taps: more than one launch holds", max_nb, ks, ks);
    // find_best_pose's arguments (scan_matching.py:100-108); the padded lattice holds np.arange's lengths of both passes
    const double c_search = m->cfg.search_size * 0.5, c_step = res * 2;
    const double c_tsearch = m->cfg.coarse_search_angle_offset * 0.5, c_tstep = m->cfg.coarse_angle_resolution;
    const int maxd = std::max({8, (int)std::ceil(2 * c_search / c_step) + 2, (int)std::ceil(4 * res / res) + 2});
    const int maxt = std::max({13, (int)std::ceil(2 * c_tsearch / c_tstep) + 2});
    if (maxd > YM_YAG_MAX_DIM || maxt > YM_YAG_MAX_NT)
        return set_err(YM_ERR_UNSUPPORTED, "search lattice %d x %d x %d exceeds the built-in limit", maxd, maxd, maxt);
    const size_t vol = (size_t)maxt * maxd * maxd;
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
    int rc;
    Slot &slot = m->slots[kAsyncSlots];
    if (slot.in_flight) return set_err(YM_ERR_BUSY, "the synchronous slot is in flight");
    if ((rc = m->states.ensure((size_t)n_items))) return rc;
    if ((rc = m->map_pts.ensure(total_pts))) return rc;
    if ((rc = m->yaxes.ensure((size_t)chunk * 3 * YM_YAG_MAX_DIM))) return rc;
    if ((rc = m->sums.ensure(2 * sums_items * vol))) return rc;
    if ((rc = m->resp.ensure((size_t)chunk * vol))) return rc;
    if ((rc = m->sets_grid.ensure((size_t)chunk * grid_stride))) return rc;
    if ((rc = m->sets_ktab.ensure((size_t)ks * ks))) return rc;
    if (!m->yag_counters.p) {
        if ((rc = m->yag_counters.ensure(8))) return rc;
        HIP_TRY(hipMemsetAsync(m->yag_counters.p, 0, m->yag_counters.cap * sizeof(unsigned long long), m->stream));
    }
    const size_t qscans_bytes = align_up(sizeof(YmScanRef) * (size_t)n_qscans, 16);
    const size_t bscans_bytes = align_up(sizeof(YmScanRef) * (size_t)std::max(n_bscans, 1), 16);
    const size_t items_bytes = align_up(sizeof(ym::MapItemDesc) * (size_t)n_items, 16);
    const size_t view_bytes = sizeof(double2) * (size_t)n_items;
    const size_t jobs_bytes = align_up(sizeof(int2) * std::max<size_t>(n_jobs, 1), 16);
    const size_t ktab_bytes = align_up((size_t)ks * ks, 16);
    const size_t desc_bytes = qscans_bytes + bscans_bytes + items_bytes + view_bytes + jobs_bytes + ktab_bytes;
    const size_t states_bytes = sizeof(YmItemState) * (size_t)n_items;
    if ((rc = slot.desc.ensure(desc_bytes + states_bytes))) return rc;
    if ((rc = slot.result.ensure(states_bytes))) return rc;
    if ((rc = m->sets_desc.ensure(desc_bytes))) return rc;
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
    std::memset(st0, 0, states_bytes);
    for (int b = 0; b < n_items; b++) {
        st0[b].pose[0] = st0[b].center[0] = items[b].ox_real; st0[b].pose[1] = st0[b].center[1] = items[b].oy_real;
        st0[b].off_x = origin[2 * (size_t)b]; st0[b].off_y = origin[2 * (size_t)b + 1];
        st0[b].ql = m->map_pts.p + items[b].out_off;
    }
    hipStream_t st = m->stream;
    unsigned char *dd = m->sets_desc.p;
    // ym_profile_read: 0 = the integer sums of both passes (yag_map_kernel or the pair-by-pair kernel), 1 = the grids (clearing and
    // sets_grid_kernel), 2 = the whole call on the device
    hipEvent_t ev_call = nullptr, ev_k = nullptr;
    if ((rc = prof_begin(m, 2, &ev_call))) return rc;
    HIP_TRY(hipMemcpyAsync(dd, hd, desc_bytes, hipMemcpyHostToDevice, st));
    HIP_TRY(hipMemcpyAsync(m->states.p, st0, states_bytes, hipMemcpyHostToDevice, st));
    HIP_TRY(hipMemcpyAsync(m->sets_ktab.p, hd + desc_bytes - ktab_bytes, (size_t)ks * ks, hipMemcpyHostToDevice, st));
    ym::MapPointsManyArgs pa;
    std::memset(&pa, 0, sizeof pa);
    pa.scans = reinterpret_cast<const YmScanRef *>(dd);
    pa.items = reinterpret_cast<const ym::MapItemDesc *>(dd + qscans_bytes + bscans_bytes);
    pa.max_n = max_nq; pa.out = m->map_pts.p; pa.states = m->states.p;
    (void)hipFuncSetAttribute(reinterpret_cast<const void *>(ym::map_points_many_kernel), hipFuncAttributeMaxDynamicSharedMemorySize,
                              (int)YM_PREP_LDS_BYTES(YM_MAX_BEAMS));
    (void)hipFuncSetAttribute(reinterpret_cast<const void *>(ym::sets_grid_kernel<256>), hipFuncAttributeMaxDynamicSharedMemorySize,
                              (int)YM_PREP_LDS_BYTES(YM_MAX_BEAMS));
    hipLaunchKernelGGL(ym::map_points_many_kernel, dim3(n_items), dim3(1024), YM_PREP_LDS_BYTES(max_nq), st, pa);
    ym::SetsGridArgs ga;
    std::memset(&ga, 0, sizeof ga);
    ga.scans = reinterpret_cast<const YmScanRef *>(dd + qscans_bytes);
    ga.max_n = max_nb; ga.G = G; ga.res = res; ga.ktab = m->sets_ktab.p; ga.ksize = ks;
    ga.grid = m->sets_grid.p; ga.grid_stride = grid_stride;
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
        for (int pass = 0; pass < passes; pass++) {
            ym::YagArgs a;
            std::memset(&a, 0, sizeof a);
            a.g = m->geom; a.pass = pass; a.refine = refine ? 1 : 0;
            a.last = (pass == 1 || !refine) ? 1 : 0;
            a.penalize = penalize ? 1 : 0;
            if (pass == 0) { // scan_matching.py:100-103
                a.search_xy = c_search; a.step_xy = c_step; a.search_t = c_tsearch; a.step_t = c_tstep;
            } else { // scan_matching.py:106-108
                a.search_xy = res * 2; a.step_xy = res; a.search_t = 0.0349 * 0.5; a.step_t = 0.00349;
            }
            a.map_res = res;
            a.coarse_angle_res = m->cfg.coarse_angle_resolution;
            a.states = m->states.p + c0; a.host_out = reinterpret_cast<YmItemState *>(slot.result.dp) + c0;
            a.axes = m->yaxes.p; a.rot = nullptr; // (the kernels rotate the points themselves: the same products and sums)
            a.sums = m->sums.p + (size_t)pass * sums_items * vol + (keep_all ? (size_t)c0 * vol : 0); a.out = m->resp.p;
            a.grid = m->sets_grid.p; a.grid_stride = grid_stride; a.vol_stride = vol;
            a.max_n = 0; a.maxd = maxd; a.maxt = maxt; a.n_items = B;
            a.map_w = G; a.map_h = G; a.map_sets = 1;
            a.counters = m->yag_counters.p;
            // as ym_match_map_many: a pass whose every possible np.arange length fits yag_map_kernel's limit needs no yag_score_kernel,
            // one whose none does no yag_map_kernel; option 46 = 0 leaves every item to the rule as written
            const int est = (int)std::ceil(2 * a.search_xy / a.step_xy);
            const bool run_map = est - 1 <= YM_YAG_MAP_DIM && m->yag_fast != 0, run_score = est + 1 > YM_YAG_MAP_DIM || !run_map;
            a.map_dim = run_map ? YM_YAG_MAP_DIM : 0;
            const int split = std::max(1, std::min(32, 1024 / (B * maxt)));
            a.map_split = split;
            hipLaunchKernelGGL(ym::yag_setup_kernel, dim3(1, B), dim3(256), 0, st, a);
            if ((rc = prof_begin(m, 0, &ev_k))) return rc;
            if (run_map) {
                if (split > 1) HIP_TRY(hipMemsetAsync(a.sums, 0, (size_t)B * vol * sizeof(uint32_t), st));
                hipLaunchKernelGGL(ym::yag_map_kernel, dim3(8 * maxt * ((B + 7) / 8) * split), dim3(256), 0, st, a);
                if (split > 1) hipLaunchKernelGGL(ym::yag_map_score_kernel, dim3((maxd * maxd + 255) / 256, maxt, B), dim3(256), 0, st, a);
            } else if (pass == 0) m->sets_fallback_host += B;
            if (run_score) hipLaunchKernelGGL(ym::yag_score_kernel, dim3((maxd * maxd + 255) / 256, maxt, B), dim3(256), 0, st, a);
            if ((rc = prof_end(m, ev_k))) return rc;
            hipLaunchKernelGGL(ym::yag_reduce_kernel<1024>, dim3(B), dim3(1024), 0, st, a);
        }
    }
    if ((rc = prof_end(m, ev_call))) return rc;
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
    m->last_valid = false; // the debug getters describe this call: the sums through map_last, grids and query points through sets_last
    m->map_last.valid = true; m->map_last.n_items = n_items; m->map_last.first_kept = first_kept; m->map_last.passes = passes;
    m->map_last.vol = vol; m->map_last.pass_offset[0] = 0; m->map_last.pass_offset[1] = sums_items * vol;
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
