// ym_host_mapscore.hpp -- host runtime: the scoring tail that ym_match_map (ym_abi_maps.hpp), ym_match_map_many (ym_abi_maptrack.hpp)
// and ym_match_sets_many (ym_abi_sets.hpp) share: the coarse search, the padded lattice, one find_best_pose pass over a chunk of
// a batch, the results.  DESIGN.md sections 13 and 18.
// Part of yagmatch.hip (included inside its anonymous namespace); not a header of its own.

// the reference's hard-coded coarse pass against a map (scan_matching.py:152-153) unless the caller overrides it
int map_search_params(const ym_map_search *coarse, ym_map_search *cs) {
    if (coarse) *cs = *coarse;
    else { cs->xy_search = 0.25; cs->xy_step = 0.01; cs->angle_search = 0.1; cs->angle_step = 0.01; cs->grid_resolution = 0.05; cs->penalize = 0; cs->reserved = 0; }
    if (!(cs->xy_step > 0) || !(cs->angle_step > 0) || !(cs->grid_resolution > 0) || !(cs->xy_search > 0) || !(cs->angle_search > 0))
        return set_err(YM_ERR_INVALID, "bad coarse search parameters");
    return YM_OK;
}

// The centre of a set of query scans (scan_matching.py:68-74, :136-139): the mean of their positions, Python's left-to-right sum;
// the heading is 0.  item: the set's index for the refusal's text, -1 in a call of one set.  *total: the set's beams.
int yag_set_centre(const ym_matcher *m, const ym_scan *const *q, int nq, int item, double *cx, double *cy, int *total, int *max_n) {
    double sx = 0, sy = 0;
    *total = 0;
    for (int i = 0; i < nq; i++) {
        if (!q[i] || q[i]->device != m->device)
            return item < 0 ? set_err(YM_ERR_INVALID, "query %d is null or lives on another device", i)
                            : set_err(YM_ERR_INVALID, "item %d: query %d is null or lives on another device", item, i);
        sx = i == 0 ? q[i]->pose[0] : sx + q[i]->pose[0];
        sy = i == 0 ? q[i]->pose[1] : sy + q[i]->pose[1];
        *total += q[i]->n;
        *max_n = std::max(*max_n, q[i]->n);
    }
    *cx = sx / (double)nq; *cy = sy / (double)nq;
    return YM_OK;
}

// item b of a batch: the scans queries[lo .. lo + nq) of a table that begins at queries[first]; its points go behind *total_pts
int yag_item_desc(const ym_matcher *m, const ym_scan *const *queries, int first, int lo, int nq, int b, ym::MapItemDesc *it, size_t *total_pts,
                  int *max_n) {
    int total, rc;
    if ((rc = yag_set_centre(m, queries + lo, nq, b, &it->ox_real, &it->oy_real, &total, max_n))) return rc;
    it->scan_begin = lo - first; it->n_scans = nq; it->out_off = (int64_t)*total_pts;
    *total_pts += (size_t)std::max(total, 1);
    return YM_OK;
}

// the items' initial states: pose and centre at the set's centre, the grid's origin (origin[b * stride] and the next), where the
// item's points go
void yag_init_states(const ym_matcher *m, const std::vector<ym::MapItemDesc> &items, const double *origin, size_t stride, YmItemState *st0) {
    std::memset(st0, 0, sizeof(YmItemState) * items.size());
    for (size_t b = 0; b < items.size(); b++) {
        st0[b].pose[0] = st0[b].center[0] = items[b].ox_real; st0[b].pose[1] = st0[b].center[1] = items[b].oy_real;
        st0[b].off_x = origin[b * stride]; st0[b].off_y = origin[b * stride + 1];
        st0[b].ql = m->map_pts.p + items[b].out_off;
    }
}

// yag_map_kernel's counters: zeroed when the first batch of a matcher allocates them
int yag_counters_ensure(ym_matcher *m) {
    if (m->yag_counters.p) return YM_OK;
    int rc;
    if ((rc = m->yag_counters.ensure(8))) return rc;
    HIP_TRY(hipMemsetAsync(m->yag_counters.p, 0, m->yag_counters.cap * sizeof(unsigned long long), m->stream));
    return YM_OK;
}

// the batch's query points into m->map_pts, a block per item
void enqueue_map_points_many(ym_matcher *m, const YmScanRef *scans, const ym::MapItemDesc *items, int n_items, int max_n) {
    ym::MapPointsManyArgs pa;
    std::memset(&pa, 0, sizeof pa);
    pa.scans = scans; pa.items = items; pa.max_n = max_n; pa.out = m->map_pts.p; pa.states = m->states.p;
    (void)hipFuncSetAttribute(reinterpret_cast<const void *>(ym::map_points_many_kernel), hipFuncAttributeMaxDynamicSharedMemorySize,
                              (int)YM_PREP_LDS_BYTES(YM_MAX_BEAMS));
    hipLaunchKernelGGL(ym::map_points_many_kernel, dim3(n_items), dim3(1024), YM_PREP_LDS_BYTES(max_n), m->stream, pa);
}

// The padded lattice: it holds np.arange's lengths of both passes.  yag_setup_kernel clamps the lengths to it, so every caller
// takes it from here.  what: "map " or "", the refusal's first word.
struct YagLattice { int maxd = 0, maxt = 0; size_t vol = 0; };
int yag_lattice_bound(const ym_map_search &cs, double res, const char *what, YagLattice *L) {
    L->maxd = std::max({8, (int)std::ceil(2 * cs.xy_search / cs.xy_step) + 2, (int)std::ceil(4 * res / res) + 2});
    L->maxt = std::max({13, (int)std::ceil(2 * cs.angle_search / cs.angle_step) + 2});
    if (L->maxd > YM_YAG_MAX_DIM || L->maxt > YM_YAG_MAX_NT)
        return set_err(YM_ERR_UNSUPPORTED, "%ssearch lattice %d x %d x %d exceeds the built-in limit", what, L->maxd, L->maxd, L->maxt);
    L->vol = (size_t)L->maxt * L->maxd * L->maxd;
    return YM_OK;
}

// what every pass of these calls sets alike; pass 0 searches as `cs` says, pass 1 as the reference's fine search on the matcher's cells
ym::YagArgs yag_pass_args(const ym_matcher *m, const ym_map_search &cs, const YagLattice &L, int pass, int penalize, int refine) {
    ym::YagArgs a;
    std::memset(&a, 0, sizeof a);
    a.g = m->geom; a.pass = pass; a.refine = refine ? 1 : 0;
    a.last = (pass == 1 || !refine) ? 1 : 0;
    if (pass == 0) {
        a.search_xy = cs.xy_search; a.step_xy = cs.xy_step; a.search_t = cs.angle_search; a.step_t = cs.angle_step;
        a.map_res = cs.grid_resolution; a.penalize = cs.penalize ? 1 : 0;
    } else {
        yag_fine_search(a, m->cfg.resolution);
        a.map_res = m->cfg.resolution; a.penalize = penalize ? 1 : 0;
    }
    a.coarse_angle_res = m->cfg.coarse_angle_resolution;
    a.axes = m->yaxes.p; a.out = m->resp.p;
    a.vol_stride = L.vol; a.maxd = L.maxd; a.maxt = L.maxt;
    return a;
}

// ---- one pass over one chunk of a batch (items c0 .. c0 + B): ym_match_map_many and ym_match_sets_many
struct YagBatch {
    const uint8_t *grid; size_t grid_stride; // one grid for all items (stride 0) or one per item of the chunk
    int map_w, map_h;
    double map_ox, map_oy;                   // the grid's origin where the items' states do not carry it
    int map_sets;
    ym_map_search coarse;
    int penalize, refine;
    YagLattice L;
    size_t sums_items; bool keep_all;        // the sums of a pass: [sums_items][vol], of all items or of the chunk
    bool need_fast;                          // yag_map_kernel only while option 46 leaves it on
    int64_t *fallback;                       // counts the items of coarse passes that yag_map_kernel did not take
    bool profile;                            // the integer sums are timed (ym_profile_read slot 0)
};

int enqueue_yag_batch_pass(ym_matcher *m, Slot &slot, const YagBatch &S, int c0, int B, int pass) {
    hipStream_t st = m->stream;
    const int maxd = S.L.maxd, maxt = S.L.maxt;
    const size_t vol = S.L.vol;
    ym::YagArgs a = yag_pass_args(m, S.coarse, S.L, pass, S.penalize, S.refine);
    a.states = m->states.p + c0; a.host_out = reinterpret_cast<YmItemState *>(slot.result.dp) + c0;
    a.rot = nullptr; // (the kernels rotate the points themselves: the same products and sums)
    a.sums = m->sums.p + (size_t)pass * S.sums_items * vol + (S.keep_all ? (size_t)c0 * vol : 0);
    a.grid = S.grid; a.grid_stride = S.grid_stride;
    a.max_n = 0; a.n_items = B;
    a.map_w = S.map_w; a.map_h = S.map_h; a.map_ox = S.map_ox; a.map_oy = S.map_oy; a.map_sets = S.map_sets;
    a.counters = m->yag_counters.p;
    // np.arange's length is within one of ceil(2 search / step): a pass whose every possible length fits yag_map_kernel's
    // limit needs no yag_score_kernel, one whose none does no yag_map_kernel; in between both run and the lengths decide
    const int est = (int)std::ceil(2 * a.search_xy / a.step_xy);
    const bool run_map = est - 1 <= YM_YAG_MAP_DIM && (!S.need_fast || m->yag_fast != 0);
    const bool run_score = est + 1 > YM_YAG_MAP_DIM || !run_map;
    a.map_dim = run_map ? YM_YAG_MAP_DIM : 0;
    // a few items alone leave the device empty: their (item, angle) blocks are split until about four blocks per CU exist
    const int split = std::max(1, std::min(32, 1024 / (B * maxt)));
    a.map_split = split;
    yag_frame_record(m, a, S.map_sets ? 2 : 1);
    hipLaunchKernelGGL(ym::yag_setup_kernel, dim3(1, B), dim3(256), 0, st, a);
    hipEvent_t ev_k = nullptr;
    int rc;
    if (S.profile && (rc = prof_begin(m, 0, &ev_k))) return rc;
    if (run_map) {
        if (split > 1) HIP_TRY(hipMemsetAsync(a.sums, 0, (size_t)B * vol * sizeof(uint32_t), st));
        hipLaunchKernelGGL(ym::yag_map_kernel, dim3(8 * maxt * ((B + 7) / 8) * split), dim3(256), 0, st, a);
        if (split > 1) hipLaunchKernelGGL(ym::yag_map_score_kernel, dim3((maxd * maxd + 255) / 256, maxt, B), dim3(256), 0, st, a);
    } else if (pass == 0) *S.fallback += B;
    if (run_score) hipLaunchKernelGGL(ym::yag_score_kernel, dim3((maxd * maxd + 255) / 256, maxt, B), dim3(256), 0, st, a);
    if ((rc = prof_end(m, ev_k))) return rc;
    hipLaunchKernelGGL(ym::yag_reduce_kernel<1024>, dim3(B), dim3(1024), 0, st, a);
    return YM_OK;
}

// ---- YmItemState -> ym_result
void yag_unpack_result(const YmItemState &r, int refine, ym_result *out) {
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

// what the debug getters describe after such a call: its integer sums (ym_debug_map_sums), not a match_scan call and -- until
// ym_match_sets_many says otherwise -- no set grids
void map_last_set(ym_matcher *m, int n_items, int first_kept, int passes, size_t vol, size_t pass1_offset) {
    m->last_valid = false;
    m->sets_last.valid = false;
    m->map_last.valid = true; m->map_last.n_items = n_items; m->map_last.first_kept = first_kept; m->map_last.passes = passes;
    m->map_last.vol = vol; m->map_last.pass_offset[0] = 0; m->map_last.pass_offset[1] = pass1_offset;
}
