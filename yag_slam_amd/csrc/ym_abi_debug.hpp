// ym_abi_debug.hpp -- C ABI: introspection for the parity tests, development options, profiling, counters
// Part of yagmatch.hip (included inside its extern "C" block); not a header of its own.
// ---- debug getters
int ym_debug_map_sums(ym_matcher *m, int item, int pass, uint32_t *out, int64_t out_count);
// the last completed call was ym_match_sets / ym_match_sets_many: the getters below describe its items
static bool sets_debug(const ym_matcher *m) { return !m->last_valid && m->map_last.valid && m->sets_last.valid; }
int ym_debug_grid_info(ym_matcher *m, int item, ym_grid_info *info) {
    if (!m || !info) return set_err(YM_ERR_INVALID, "null argument");
    if (sets_debug(m)) { // the last call matched scan sets: an item's grid is the reference's whole G x G grid
        const ym_matcher::SetsLast &sl = m->sets_last;
        if (item < 0 || item >= m->map_last.n_items) return set_err(YM_ERR_INVALID, "no such item in the last call");
        std::memset(info, 0, sizeof *info);
        info->width = info->height = info->pitch = sl.G;
        info->storage_w = info->storage_h = info->roi_w = info->roi_h = sl.G;
        YmItemState s;
        DEV_GUARD(m->device);
        HIP_TRY(hipStreamSynchronize(m->stream));
        HIP_TRY(hipMemcpy(&s, m->states.p + item, sizeof s, hipMemcpyDeviceToHost));
        info->offset_x = s.off_x; info->offset_y = s.off_y;
        return YM_OK;
    }
    if (!m->last_valid || item < 0 || item >= m->last_B) return set_err(YM_ERR_INVALID, "no such item in the last call");
    const YmGeom &g = m->last_geom;
    info->width = g.win_w; info->height = g.win_w; info->pitch = g.pitch;
    info->origin_x = g.win_origin; info->origin_y = g.win_origin;
    info->storage_w = g.storage_w; info->storage_h = g.storage_w;
    info->roi_x = g.border; info->roi_y = g.border; info->roi_w = g.roi_w; info->roi_h = g.roi_w;
    YmItemState s;
    DEV_GUARD(m->device);
    HIP_TRY(hipStreamSynchronize(m->stream));
    HIP_TRY(hipMemcpy(&s, m->states.p + item, sizeof s, hipMemcpyDeviceToHost));
    info->offset_x = s.off_x; info->offset_y = s.off_y;
    return YM_OK;
}

int ym_debug_grid(ym_matcher *m, int item, uint8_t *out, int64_t out_bytes) {
    if (!m || !out) return set_err(YM_ERR_INVALID, "null argument");
    if (sets_debug(m)) {
        const ym_matcher::SetsLast &sl = m->sets_last;
        if (item < 0 || item >= m->map_last.n_items) return set_err(YM_ERR_INVALID, "no such item in the last call");
        if (item < sl.first_grid) return set_err(YM_ERR_INVALID, "the grid of item %d was overwritten: the call keeps those of its last chunk, from item %d on", item, sl.first_grid);
        const int64_t need_s = (int64_t)sl.G * sl.G;
        if (out_bytes < need_s) return set_err(YM_ERR_INVALID, "grid buffer too small: need %lld bytes", (long long)need_s);
        DEV_GUARD(m->device);
        HIP_TRY(hipStreamSynchronize(m->stream));
        HIP_TRY(hipMemcpy(out, m->sets_grid.p + (size_t)(item - sl.first_grid) * sl.grid_stride, (size_t)need_s, hipMemcpyDeviceToHost));
        return YM_OK;
    }
    if (!m->last_valid || item < 0 || item >= m->last_B) return set_err(YM_ERR_INVALID, "no such item in the last call");
    const int64_t need = (int64_t)m->last_geom.pitch * m->last_geom.win_w;
    if (out_bytes < need) return set_err(YM_ERR_INVALID, "grid buffer too small: need %lld bytes", (long long)need);
    DEV_GUARD(m->device);
    HIP_TRY(hipStreamSynchronize(m->stream));
    HIP_TRY(hipMemcpy(out, m->grid.p + (size_t)item * m->last_grid_stride, (size_t)need, hipMemcpyDeviceToHost));
    return YM_OK;
}

int ym_debug_sums(ym_matcher *m, int item, int pass, uint32_t *out, int64_t out_count) {
    if (!m || !out || pass < 0 || pass > 1) return set_err(YM_ERR_INVALID, "bad argument");
    if (sets_debug(m)) return ym_debug_map_sums(m, item, pass, out, out_count); // (dense [k][iy][ix] with the item's own nx, ny, nt)
    if (!m->last_valid || item < 0 || item >= m->last_B) return set_err(YM_ERR_INVALID, "no such item in the last call");
    const size_t n = m->last_sums_stride[pass];
    if (n == 0) return set_err(YM_ERR_INVALID, "pass %d did not run", pass);
    const size_t ncopy = std::min(n, (size_t)out_count); // a pass's volume is stored dense from the start of its slot
    if (m->cfg.semantics == YM_SEM_KARTO && (size_t)out_count < n)
        return set_err(YM_ERR_INVALID, "sums buffer too small: need %zu entries", n);
    DEV_GUARD(m->device);
    HIP_TRY(hipStreamSynchronize(m->stream));
    HIP_TRY(hipMemcpy(out, m->sums.p + m->sums_pass_offset[pass] + (size_t)item * n, ncopy * sizeof(uint32_t),
                      hipMemcpyDeviceToHost));
    return YM_OK;
}

int ym_debug_query_local(ym_matcher *m, int item, double *out_xy, int32_t cap, int32_t *n) {
    if (!m || !out_xy || !n) return set_err(YM_ERR_INVALID, "null argument");
    const bool sets = sets_debug(m); // (the points of the set, relative to its centre)
    if (sets ? (item < 0 || item >= m->map_last.n_items) : (!m->last_valid || item < 0 || item >= m->last_B))
        return set_err(YM_ERR_INVALID, "no such item in the last call");
    YmItemState s;
    DEV_GUARD(m->device);
    HIP_TRY(hipStreamSynchronize(m->stream));
    HIP_TRY(hipMemcpy(&s, m->states.p + item, sizeof s, hipMemcpyDeviceToHost));
    *n = s.nq;
    if (cap < s.nq) return set_err(YM_ERR_INVALID, "buffer too small: need %d points", s.nq);
    if (s.nq > 0)
        HIP_TRY(hipMemcpy(out_xy, s.ql, sizeof(double2) * s.nq, hipMemcpyDeviceToHost));
    return YM_OK;
}

int ym_debug_cells(ym_matcher *m, int item, int32_t *out, int64_t out_count, int32_t *max_n) {
    if (!m || !max_n) return set_err(YM_ERR_INVALID, "null argument");
    if (!m->last_valid || item < 0 || item >= m->last_B) return set_err(YM_ERR_INVALID, "no such item in the last call");
    *max_n = m->last_max_n;
    const size_t per = (size_t)m->last_max_base * m->last_max_n;
    if (!out) return YM_OK;
    if ((size_t)out_count < per * 2) return set_err(YM_ERR_INVALID, "buffer too small: need %zu ints", per * 2);
    DEV_GUARD(m->device);
    HIP_TRY(hipStreamSynchronize(m->stream));
    // (the caller's format is (x, y) int32 pairs, YM_CELL_NONE twice where there is no cell, whatever the device keeps)
    std::vector<YmCell> dev(per);
    HIP_TRY(hipMemcpy(dev.data(), m->cells.p + (size_t)item * per, sizeof(YmCell) * per, hipMemcpyDeviceToHost));
    for (size_t i = 0; i < per; i++) {
        const int2 c = ym_cell_unpack(dev[i]);
        out[2 * i] = c.x;
        out[2 * i + 1] = c.y;
    }
    return YM_OK;
}

// the pair lists bin_kernel built (or a call with the same key left in the buffers: option 45) for one query slot of the last call
int ym_debug_pair_lists(ym_matcher *m, int slot, ym_pair_list_info *info, double *ctrig, int32_t *starts, int32_t *flags, uint16_t *entries,
                        uint32_t *rbox) {
    if (!m || !info) return set_err(YM_ERR_INVALID, "null argument");
    const ym_matcher::ListsLast &ll = m->lists_last;
    if (!m->last_valid || !ll.valid) return set_err(YM_ERR_INVALID, "the last call built no region pair lists");
    if (slot < 0 || slot >= (int)ll.qrep.size()) return set_err(YM_ERR_INVALID, "no such query slot in the last call");
    const int n_out = (ctrig != nullptr) + (starts != nullptr) + (flags != nullptr) + (entries != nullptr) + (rbox != nullptr);
    if (n_out != 0 && n_out != 5) return set_err(YM_ERR_INVALID, "all five arrays or none");
    const int b = ll.qrep[slot];
    if (b < 0 || b >= m->last_B) return set_err(YM_ERR_HIP, "query slot %d names item %d (a fault of the library)", slot, b);
    ym_pair_list_info o;
    std::memset(&o, 0, sizeof o);
    o.nt = ll.nt; o.lnw = ll.lnw; o.lparts = ll.lparts; o.nbins = ll.nbins; o.nrx = ll.nrx; o.nry = ll.nry; o.nregions = ll.nregions;
    o.rg_h = ll.rg_h; o.rg_cls = ll.rg_cls; o.rg_zero = ll.rg_zero; o.ng = ll.ng; o.qrep = b; o.n_slots = (int32_t)ll.qrep.size();
    o.entries_pstride = (int64_t)ll.entries_pstride;
    YmItemState s;
    int32_t c0[2];
    DEV_GUARD(m->device);
    HIP_TRY(hipStreamSynchronize(m->stream));
    HIP_TRY(hipMemcpy(&s, m->states.p + b, sizeof s, hipMemcpyDeviceToHost));
    const int32_t *hc = m->hypcell.p + (size_t)b * 2 * m->last_dim_stride;
    HIP_TRY(hipMemcpy(&c0[0], hc, sizeof(int32_t), hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(&c0[1], hc + m->last_dim_stride, sizeof(int32_t), hipMemcpyDeviceToHost));
    o.cx0 = c0[0]; o.cy0 = c0[1]; o.nq = s.nq; o.off_x = s.off_x; o.off_y = s.off_y; o.ylat[0] = s.ylat[0]; o.ylat[1] = s.ylat[1];
    if (n_out == 0) { *info = o; return YM_OK; }
    // (into buffers of the library's own first: a copy that fails leaves the caller's arrays as they were)
    const size_t n_starts = (size_t)ll.lparts * (ll.nbins + 1), n_entries = (size_t)ll.lparts * ll.entries_pstride, n_rbox = (size_t)ll.nregions * ll.lparts;
    std::vector<double> h_trig((size_t)2 * ll.nt);
    std::vector<int32_t> h_starts(n_starts + ll.lparts);
    std::vector<uint16_t> h_entries(n_entries);
    std::vector<uint32_t> h_rbox(n_rbox);
    HIP_TRY(hipMemcpy(h_trig.data(), m->ctrig.p + (size_t)b * m->last_nt_stride, sizeof(double) * 2 * ll.nt, hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(h_starts.data(), m->rg_starts.p + (size_t)slot * ll.starts_stride, sizeof(int32_t) * h_starts.size(), hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(h_entries.data(), m->rg_entries.p + (size_t)slot * ll.entries_stride, sizeof(uint16_t) * n_entries, hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(h_rbox.data(), m->rg_rbox.p + (size_t)slot * ll.rbox_stride, sizeof(uint32_t) * n_rbox, hipMemcpyDeviceToHost));
    *info = o;
    std::memcpy(ctrig, h_trig.data(), sizeof(double) * h_trig.size());
    std::memcpy(starts, h_starts.data(), sizeof(int32_t) * n_starts);
    std::memcpy(flags, h_starts.data() + n_starts, sizeof(int32_t) * ll.lparts);
    std::memcpy(entries, h_entries.data(), sizeof(uint16_t) * n_entries);
    std::memcpy(rbox, h_rbox.data(), sizeof(uint32_t) * n_rbox);
    return YM_OK;
}

// what find_best_pose pass `pass` of item `item` of the last YM_SEM_YAGPY call computed with (include/yagmatch.h).  Reads only.
int ym_debug_yag_frame(ym_matcher *m, int item, int pass, ym_yag_frame *info, double *axes, double *trig, double *points) {
    if (!m || !info || pass < 0 || pass > 1) return set_err(YM_ERR_INVALID, "bad argument");
    if (m->cfg.semantics != YM_SEM_YAGPY) return set_err(YM_ERR_UNSUPPORTED, "ym_debug_yag_frame needs a YM_SEM_YAGPY matcher");
    const ym_matcher::YagFrameLast &fl = m->yag_frame_last;
    const bool chain = m->last_valid, sets = sets_debug(m);
    const int kind = chain ? 0 : sets ? 2 : 1;
    if ((!chain && !m->map_last.valid) || fl.kind != kind) return set_err(YM_ERR_INVALID, "the last call left no frame");
    if (item < 0 || item >= (chain ? m->last_B : m->map_last.n_items)) return set_err(YM_ERR_INVALID, "no such item in the last call");
    if (pass >= fl.passes) return set_err(YM_ERR_INVALID, "pass %d did not run", pass);
    const int n_out = (axes != nullptr) + (trig != nullptr) + (points != nullptr);
    if (n_out != 0 && n_out != 3) return set_err(YM_ERR_INVALID, "all three arrays or none");
    const ym_matcher::YagFrameLast::Pass &fp = fl.pass[pass];
    YmItemState s;
    DEV_GUARD(m->device);
    HIP_TRY(hipStreamSynchronize(m->stream));
    HIP_TRY(hipMemcpy(&s, m->states.p + item, sizeof s, hipMemcpyDeviceToHost));
    ym_yag_frame o;
    std::memset(&o, 0, sizeof o);
    o.kind = kind; o.pass = pass; o.nx = s.ydims[pass][0]; o.ny = s.ydims[pass][1]; o.nt = s.ydims[pass][2]; o.nq = s.nq;
    o.grid_w = fp.grid_w; o.grid_h = fp.grid_h; o.roi_w = fl.roi_w; o.win_origin = fl.win_origin; o.win_w = fl.win_w; o.pitch = fl.pitch;
    o.lat_nx = fl.lat_nx; o.lat_ny = fl.lat_ny; o.lat_nt = fl.lat_nt; o.step_cells = fl.step_cells;
    o.regular = s.regular[0]; o.map_split = fl.map_split;
    o.ox = fp.own_origin ? s.off_x : fp.ox; o.oy = fp.own_origin ? s.off_y : fp.oy; o.res = fp.res;
    o.search_xy = fp.search_xy; o.step_xy = fp.step_xy; o.search_t = fp.search_t; o.step_t = fp.step_t;
    for (int i = 0; i < 3; i++) o.centre[i] = pass ? s.ybest[0][1 + i] : s.pose[i];
    if (o.nx < 0 || o.ny < 0 || o.nt < 0 || o.nx > YM_YAG_MAX_DIM || o.ny > YM_YAG_MAX_DIM || o.nt > YM_YAG_MAX_DIM || o.nq < 0)
        return set_err(YM_ERR_HIP, "item %d has an impossible lattice (a fault of the library)", item);
    if (n_out == 0) { *info = o; return YM_OK; }
    const size_t n_axes = (size_t)o.nx + o.ny + o.nt;
    DevBuf<double> d_axes;
    DevBuf<double2> d_trig;
    int rc;
    if ((rc = d_axes.alloc(std::max<size_t>(n_axes, 1))) || (rc = d_trig.alloc((size_t)std::max(o.nt, 1)))) return rc;
    ym::YagFrameArgs a;
    a.state = m->states.p + item; a.pass = pass;
    a.search_xy = fp.search_xy; a.step_xy = fp.step_xy; a.search_t = fp.search_t; a.step_t = fp.step_t;
    a.axes = d_axes.p; a.trig = d_trig.p;
    hipLaunchKernelGGL(ym::yag_frame_kernel, dim3(1), dim3(256), 0, m->stream, a);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipStreamSynchronize(m->stream));
    // (into buffers of the library's own first: a copy that fails leaves the caller's arrays as they were)
    std::vector<double> h_axes(n_axes), h_trig((size_t)2 * o.nt), h_pts((size_t)2 * o.nq);
    if (n_axes) HIP_TRY(hipMemcpy(h_axes.data(), d_axes.p, sizeof(double) * n_axes, hipMemcpyDeviceToHost));
    if (o.nt) HIP_TRY(hipMemcpy(h_trig.data(), d_trig.p, sizeof(double2) * o.nt, hipMemcpyDeviceToHost));
    if (o.nq) HIP_TRY(hipMemcpy(h_pts.data(), s.ql, sizeof(double2) * o.nq, hipMemcpyDeviceToHost));
    if (chain && pass == fl.passes - 1) {
        // the axes buffer still holds this pass's axes of every item of a chain call: the recomputed ones must be those, bit for bit
        std::vector<double> live((size_t)3 * YM_YAG_MAX_DIM);
        HIP_TRY(hipMemcpy(live.data(), m->yaxes.p + (size_t)item * 3 * YM_YAG_MAX_DIM, sizeof(double) * live.size(), hipMemcpyDeviceToHost));
        const int n[3] = {o.nx, o.ny, o.nt};
        for (int ax = 0, at = 0; ax < 3; at += n[ax], ax++)
            if (std::memcmp(live.data() + (size_t)ax * YM_YAG_MAX_DIM, h_axes.data() + at, sizeof(double) * n[ax]))
                return set_err(YM_ERR_HIP, "item %d: the recomputed axes of pass %d are not the ones the pass used (a fault of the library)", item, pass);
    }
    *info = o;
    std::memcpy(axes, h_axes.data(), sizeof(double) * n_axes);
    std::memcpy(trig, h_trig.data(), sizeof(double) * h_trig.size());
    std::memcpy(points, h_pts.data(), sizeof(double) * h_pts.size());
    return YM_OK;
}

// The options the parity tests use are tabulated in include/yagmatch.h.  The others -- development and timing switches:
//    2  rasterise every tile of the window                      3  beams in flight per lane in the direct correlate (16 / 32 / 48)
//    4  extra dynamic LDS bytes per direct-correlate block        5  beam chunks per angle of the direct correlate
//    9  chunk-waves per direct-correlate block (1, 2, 4)        23  0 = single matches wait for a stream event instead of polling
//   26  512 = the single-item prepare kernel with 512 threads   29  0 = the region path's pair lists on the call's own stream
//   34  blocks that share an (item, angle block)'s regions (0 = by batch size)
//   36  the raster does not write the row-major window (timing only)
//   38  unused dynamic LDS bytes per region-correlate block     40  batch size from which batches get raster work lists (48)
//   42  the region correlate's threshold alone (0 = 48)
//   49  1 = the angular covariance always gathers the scan again (tests: tabulated in include/yagmatch.h)
// (0, 32, 33, 35, 43 and 44 chose between correlate forms that are gone: YM_ERR_INVALID)
int ym_debug_option(ym_matcher *m, int option, int value) {
    if (m) { m->cache_gen++; m->list_key_valid = false; } // (whatever the option changes, no earlier plan or pair list is reused)
    if (!m) return set_err(YM_ERR_INVALID, "null matcher");
    if (option == 0 || option == 32 || option == 33 || option == 35 || option == 43 || option == 44)
        return set_err(YM_ERR_INVALID, "debug option %d (an experimental correlate form) no longer exists", option);
    else if (option == 2) m->full_raster = value;
    else if (option == 3) m->corr_u = value;
    else if (option == 4) m->corr_pad_lds = value;
    else if (option == 5) m->corr_chunks = value;
    else if (option == 6) m->finish_form = value;
    else if (option == 9) m->corr_cw = value;
    else if (option == 10) m->select_global = value;
    else if (option == 41) m->select_split_max = value;
    else if (option == 11) m->finish_threads = value;
    else if (option == 12) m->keep_sums = value;
    else if (option == 13) m->corr_dedup = value;
    else if (option == 14) m->corr_region = value;
    else if (option == 15) m->corr_region_na = m->corr_region_nw = value;
    else if (option == 23) m->poll_completion = value != 0;
    else if (option == 24) m->use_scan_structure = value != 0;
    else if (option == 25) m->chain_margin = value;
    else if (option == 26) m->prepare_threads = value;
    else if (option == 28) { // both LDS correlates from `value` items on (at least 8); 0 = the defaults again (gather 64, region 48)
        if (value == 0) { m->lds_min_batch = 64; m->rg_min_batch = 48; }
        else m->lds_min_batch = m->rg_min_batch = std::max(8, value);
    }
    else if (option == 42) m->rg_min_batch = value == 0 ? 48 : std::max(8, value); // the region correlate's threshold alone
    else if (option == 29) m->overlap_lists = value != 0;
    else if (option == 31) m->staged_queries = value != 0;
    else if (option == 30) m->tile_h_forced = value == YM_TILE_H || value == YM_TILE_H_TALL ? value : 0;
    else if (option == 16) m->raster_gx = value;
    else if (option == 17) m->corr_region_parts = value;
    else if (option == 21) m->corr_fuse_score = value;
    else if (option == 45) { m->list_cache_on = value != 0; m->list_key_valid = false; }
    else if (option == 46) m->yag_fast = value < 0 ? 0 : value > 2 ? 1 : value;
    else if (option == 47) m->map_chunk_forced = value > 0 ? value : 0;
    else if (option == 48) m->sets_chunk_forced = value > 0 ? value : 0;
    else if (option == 49) m->force_regather = value != 0;
    else if (option == 34) m->corr_region_rsplit = value;
    else if (option == 36) m->raster_planes_only = value;
    else if (option == 37) m->raster_no_rowtab = value;
    else if (option == 38) m->corr_region_pad_lds = value;
    else if (option == 39) m->keep_planes = value;
    else if (option == 40) m->tile_list_min_batch = value;
    else if (option == 19) m->corr_region_cap = value;
    else if (option == 20) m->corr_region_lds = value;
    else if (option == 18) m->raster_hits_per_tile = value;
    else if (option == 7) { // point cache: 0 = on (default), 1 = off, 2 = drop every entry now
        m->cache_off = value == 1;
        m->cache_entries.clear();
        m->cache_index.clear();
        m->cache_used = 0;
    }
    else if (option == 8) { // point cache limit in KiB (development / tests: force the start-over path)
        m->cache_limit = (size_t)std::max(1, value) << 10;
        HIP_TRY(hipStreamSynchronize(m->stream));
        m->cache_entries.clear();
        m->cache_index.clear();
        m->cache_used = 0;
        m->cache_arena.release();
    }
    else return set_err(YM_ERR_INVALID, "unknown option %d", option);
    return YM_OK;
}

int ym_debug_live_bytes(int64_t *device_bytes, int64_t *pinned_bytes) {
    if (!device_bytes || !pinned_bytes) return set_err(YM_ERR_INVALID, "null argument");
    *device_bytes = g_live_dev_bytes.load();
    *pinned_bytes = g_live_pinned_bytes.load();
    return YM_OK;
}

int ym_debug_stamps(ym_matcher *m, int enable, uint64_t *out, int32_t count) {
    if (!m) return set_err(YM_ERR_INVALID, "null matcher");
    DEV_GUARD(m->device);
    HIP_TRY(hipStreamSynchronize(m->stream));
    if (out && count > 0)
        HIP_TRY(hipMemcpy(out, m->stamps.p, sizeof(uint64_t) * std::min(count, 32), hipMemcpyDeviceToHost));
    if (enable && !m->stamps_on) HIP_TRY(hipMemset(m->stamps.p, 0, 32 * sizeof(unsigned long long))); // (some slots are counters)
    m->stamps_on = enable != 0;
    return YM_OK;
}

// ---- profiling
int ym_profile_enable(ym_matcher *m, int on) {
    if (!m) return set_err(YM_ERR_INVALID, "null matcher");
    m->profiling = on != 0;
    return YM_OK;
}

int ym_profile_read(ym_matcher *m, int which, double *ms_total, int64_t *launches, int reset) {
    if (!m || which < 0 || which > 2) return set_err(YM_ERR_INVALID, "bad argument");
    DEV_GUARD(m->device);
    HIP_TRY(hipStreamSynchronize(m->stream));
    int rc = prof_collect(m);
    if (rc) return rc;
    if (ms_total) *ms_total = m->prof[which].ms;
    if (launches) *launches = m->prof[which].launches;
    if (reset) { m->prof[which].ms = 0; m->prof[which].launches = 0; }
    return YM_OK;
}

int ym_sequence_stats(const ym_matcher *m, int64_t *segments, int64_t *faults, int64_t *sync_steps) {
    if (!m || !segments || !faults || !sync_steps) return set_err(YM_ERR_INVALID, "null argument");
    *segments = m->seq_segments; *faults = m->seq_faults; *sync_steps = m->seq_sync_steps;
    return YM_OK;
}

int ym_debug_counters(ym_matcher *m, int64_t *out, int32_t count) {
    if (!m || !out || count < 0) return set_err(YM_ERR_INVALID, "bad argument");
    int64_t v[YM_DEBUG_COUNTERS];
    std::memset(v, 0, sizeof v);
    if (m->yag_counters.p) {
        DEV_GUARD(m->device);
        unsigned long long c[8];
        HIP_TRY(hipStreamSynchronize(m->stream));
        HIP_TRY(hipMemcpy(c, m->yag_counters.p, sizeof c, hipMemcpyDeviceToHost));
        for (int i = 0; i < 4; i++) v[i] = (int64_t)c[i];
        v[6] = (int64_t)c[4]; v[7] = (int64_t)c[5];
        v[8] = (int64_t)c[6]; v[9] = (int64_t)c[7];
    }
    v[4] = m->list_cache_hits;
    v[5] = m->last_corr_form;
    v[7] += m->map_fallback_host;
    v[9] += m->sets_fallback_host;
    for (int i = 0; i < std::min<int>(count, YM_DEBUG_COUNTERS); i++) out[i] = v[i];
    return YM_OK;
}

// the dense [k][iy][ix] integer sums of item `item`, pass `pass`, of the last map call (ym_match_map: item 0)
int ym_debug_map_sums(ym_matcher *m, int item, int pass, uint32_t *out, int64_t out_count) {
    if (!m || !out || pass < 0 || pass > 1) return set_err(YM_ERR_INVALID, "bad argument");
    const ym_matcher::MapLast &ml = m->map_last;
    if (m->last_valid || !ml.valid) return set_err(YM_ERR_INVALID, "the last call was not a map call");
    if (item < 0 || item >= ml.n_items) return set_err(YM_ERR_INVALID, "no such item in the last map call");
    if (pass >= ml.passes) return set_err(YM_ERR_INVALID, "pass %d did not run", pass);
    if (item < ml.first_kept) return set_err(YM_ERR_INVALID, "the sums of item %d were overwritten: a call of this size keeps those from item %d on", item, ml.first_kept);
    DEV_GUARD(m->device);
    HIP_TRY(hipStreamSynchronize(m->stream));
    YmItemState s;
    HIP_TRY(hipMemcpy(&s, m->states.p + item, sizeof s, hipMemcpyDeviceToHost));
    const size_t n = (size_t)s.ydims[pass][0] * s.ydims[pass][1] * s.ydims[pass][2];
    if (n > ml.vol) return set_err(YM_ERR_HIP, "item %d has a lattice larger than its volume (a fault of the library)", item);
    if (out_count < 0 || (size_t)out_count < n) return set_err(YM_ERR_INVALID, "sums buffer too small: need %zu entries", n);
    if (n) HIP_TRY(hipMemcpy(out, m->sums.p + ml.pass_offset[pass] + (size_t)(item - ml.first_kept) * ml.vol, n * sizeof(uint32_t), hipMemcpyDeviceToHost));
    return YM_OK;
}

int ym_cache_stats(const ym_matcher *m, int64_t *hits, int64_t *misses) {
    if (!m) return set_err(YM_ERR_INVALID, "null matcher");
    if (hits) *hits = m->cache_hits;
    if (misses) *misses = m->cache_misses;
    return YM_OK;
}
