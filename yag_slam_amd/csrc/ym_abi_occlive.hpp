// ym_abi_occlive.hpp -- C ABI: the live occupancy grid (ym_occmap_*; kernels in ym_k_occupancy.hpp and their launch helpers in
// ym_abi_occupancy.hpp, both shared with the full renderer; window and growth arithmetic in ym_occlive_window.hpp)
// Part of yagmatch.hip (included inside its extern "C" block); not a header of its own.
// Everything runs on the null stream and every entry returns with its work complete, like occupancy_render: a scan may be destroyed
// as soon as the call that read it has returned.
static int occmap_check(const ym_occmap *om) { return om ? YM_OK : set_err(YM_ERR_INVALID, "null occupancy map"); }

ym_occmap *ym_occmap_create(int device, double resolution, double range_threshold, const double *anchor_xy, int slack_cells) {
    if (!(resolution > 0) || !(range_threshold > 0)) { set_err(YM_ERR_INVALID, "resolution and range_threshold must be > 0"); return nullptr; }
    const double scale = 1.0 / resolution;
    // (the wave-per-ray trace multiplies two ray lengths in cells: ym_k_occupancy.hpp proves its bound from this one)
    if (!(range_threshold * scale < 16777216.0)) { set_err(YM_ERR_UNSUPPORTED, "range_threshold / resolution must be below 2^24 cells"); return nullptr; }
    if (slack_cells < 0) { set_err(YM_ERR_INVALID, "slack_cells %d: 0 or more", slack_cells); return nullptr; }
    if (anchor_xy && !(std::isfinite(anchor_xy[0]) && std::isfinite(anchor_xy[1]))) { set_err(YM_ERR_INVALID, "anchor: not finite"); return nullptr; }
    if (check_device(device) != YM_OK) return nullptr;
    ym_occmap *om = new ym_occmap();
    om->device = device;
    om->resolution = resolution; om->range_threshold = range_threshold; om->scale = scale;
    om->slack = slack_cells;
    if (anchor_xy) { om->has_anchor = true; om->anchor[0] = anchor_xy[0]; om->anchor[1] = anchor_xy[1]; }
    return om;
}

void ym_occmap_destroy(ym_occmap *om) {
    if (!om) return;
    DevGuard guard(om->device);
    delete om;
}

// development: option 1 = the trace kernel's form (0: a wave per ray, the default; 1: a thread per ray)
int ym_occmap_debug_option(ym_occmap *om, int option, int value) {
    if (int rc = occmap_check(om)) return rc;
    if (option == 1 && (value == 0 || value == 1)) { om->trace_form = value; return YM_OK; }
    return set_err(YM_ERR_INVALID, "unknown option %d = %d", option, value);
}

int ym_occmap_accumulate(ym_occmap *om, const ym_scan *const *scans, const double *poses, int n, int sign) {
    if (int rc = occmap_check(om)) return rc;
    if (!scans || n <= 0) return set_err(YM_ERR_INVALID, "no scans");
    if (sign != 1 && sign != -1) return set_err(YM_ERR_INVALID, "sign %d: +1 or -1", sign);
    if (sign < 0 && !om->added) return set_err(YM_ERR_INVALID, "nothing has been added yet: nothing to subtract");
    int max_n = 1;
    for (int i = 0; i < n; i++) {
        if (!scans[i] || scans[i]->device != om->device) return set_err(YM_ERR_INVALID, "scan %d is null or lives on another device", i);
        max_n = std::max(max_n, scans[i]->n);
        const double *p = poses ? poses + 3 * (size_t)i : scans[i]->pose;
        if (!(std::isfinite(p[0]) && std::isfinite(p[1]) && std::isfinite(p[2]))) return set_err(YM_ERR_INVALID, "pose %d: not finite", i);
    }
    DEV_GUARD(om->device);
    std::vector<YmScanRef> hs(n);
    for (int i = 0; i < n; i++) hs[i] = scan_ref(scans[i], poses ? poses + 3 * (size_t)i : nullptr, true);
    int rc;
    DevBuf<YmScanRef> d_scans;
    if ((rc = d_scans.alloc(n))) return rc;
    HIP_TRY(hipMemcpy(d_scans.p, hs.data(), sizeof(YmScanRef) * n, hipMemcpyHostToDevice));
    ym::OccArgs a;
    std::memset(&a, 0, sizeof a);
    a.scans = d_scans.p; a.n_scans = n; a.max_n = max_n; a.range_threshold = om->range_threshold; a.scale = om->scale;
    a.sign = sign > 0 ? 1u : 0xFFFFFFFFu;
    if (sign > 0) {
        // the bounding boxes, as the full renderer takes them, joined with the running box
        DevBuf<double> d_boxes;
        DevBuf<int32_t> d_reach;
        if ((rc = d_boxes.alloc((size_t)4 * n)) || (rc = d_reach.alloc((size_t)4 * n))) return rc;
        double box[4] = {1e300, 1e300, -1e300, -1e300};
        if (om->added) std::memcpy(box, om->box, sizeof box);
        if ((rc = occ_join_boxes(d_scans.p, n, max_n, om->range_threshold, d_boxes.p, box))) return rc;
        double anchor[2] = {om->anchor[0], om->anchor[1]};
        if (!om->has_anchor) { anchor[0] = box[0]; anchor[1] = box[1]; } // the first add decides
        ymw::Rect window;
        if (!ymw::window_of_box(box, anchor, om->scale, &window))
            return set_err(YM_ERR_UNSUPPORTED, "the scans' bounding box leaves the lattice (2^30 cells either side of the anchor)");
        if ((double)window.w * (double)window.h > 2.0e9)
            return set_err(YM_ERR_UNSUPPORTED, "occupancy grid of %lld x %lld cells", (long long)window.w, (long long)window.h);
        // the cells the new rays can touch
        a.anchor_x = anchor[0]; a.anchor_y = anchor[1]; a.reach = d_reach.p;
        hipLaunchKernelGGL(ym::occ_reach_kernel, dim3(n), dim3(256), 0, nullptr, a);
        HIP_TRY(hipGetLastError());
        std::vector<int32_t> rr((size_t)4 * n);
        HIP_TRY(hipMemcpy(rr.data(), d_reach.p, sizeof(int32_t) * rr.size(), hipMemcpyDeviceToHost));
        ymw::Rect reach = om->added ? om->reach : ymw::Rect();
        for (int i = 0; i < n; i++) {
            ymw::Rect r;
            r.x0 = rr[4 * i]; r.y0 = rr[4 * i + 1];
            r.w = (int64_t)rr[4 * i + 2] - r.x0 + 1; r.h = (int64_t)rr[4 * i + 3] - r.y0 + 1;
            if (r.empty() || !ymw::in_lattice(r)) return set_err(YM_ERR_UNSUPPORTED, "scan %d reaches beyond the lattice (2^30 cells either side of the anchor)", i);
            reach = ymw::join(reach, r);
        }
        ymw::Growth g;
        const int grc = ymw::plan_growth(om->alloc, ymw::join(window, reach), om->slack, &g);
        if (grc == ymw::kGrowTooLarge) return set_err(YM_ERR_UNSUPPORTED, "the occupancy map would need more than 2 * 10^9 cells of memory");
        if (grc != ymw::kGrowOk) return set_err(YM_ERR_UNSUPPORTED, "the occupancy map would leave the lattice");
        if (g.grow) {
            const size_t cells = (size_t)g.alloc.cells(), old_cells = (size_t)om->alloc.cells();
            DevBuf<unsigned> bigger;
            if ((rc = bigger.alloc(2 * cells))) return rc;
            HIP_TRY(hipMemset(bigger.p, 0, 2 * cells * sizeof(unsigned)));
            if (g.copy_w > 0) {
                const size_t dst0 = (size_t)g.dst_offset();
                for (int plane = 0; plane < 2; plane++)
                    HIP_TRY(hipMemcpy2D(bigger.p + plane * cells + dst0, (size_t)g.alloc.w * sizeof(unsigned), om->cnt.p + plane * old_cells,
                                        (size_t)om->alloc.w * sizeof(unsigned), (size_t)g.copy_w * sizeof(unsigned), (size_t)g.copy_h,
                                        hipMemcpyDeviceToDevice));
                om->reallocations++;
            }
            std::swap(om->cnt.p, bigger.p);
            std::swap(om->cnt.cap, bigger.cap); // (the old memory goes with `bigger`)
            om->alloc = g.alloc;
        }
        std::memcpy(om->box, box, sizeof box);
        om->anchor[0] = anchor[0]; om->anchor[1] = anchor[1]; om->has_anchor = true;
        om->window = window; om->reach = reach; om->added = true;
    }
    a.anchor_x = om->anchor[0]; a.anchor_y = om->anchor[1];
    a.org_x = (int32_t)om->alloc.x0; a.org_y = (int32_t)om->alloc.y0; a.width = (int32_t)om->alloc.w; a.height = (int32_t)om->alloc.h;
    a.pitch = om->alloc.w;
    a.pass = om->cnt.p; a.hits = om->cnt.p + (size_t)om->alloc.cells();
    if ((rc = occ_trace(a, d_scans.p, n, om->trace_form))) return rc;
    HIP_TRY(hipStreamSynchronize(nullptr));
    return YM_OK;
}

int ym_occmap_clear(ym_occmap *om) {
    if (int rc = occmap_check(om)) return rc;
    DEV_GUARD(om->device);
    if (om->cnt.p) HIP_TRY(hipMemset(om->cnt.p, 0, 2 * (size_t)om->alloc.cells() * sizeof(unsigned)));
    om->added = false;
    om->window = ymw::Rect(); om->reach = ymw::Rect();
    return YM_OK;
}

int ym_occmap_get_info(const ym_occmap *om, ym_occmap_info *info) {
    if (!om || !info) return set_err(YM_ERR_INVALID, "null argument");
    std::memset(info, 0, sizeof *info);
    info->resolution = om->resolution;
    info->has_anchor = om->has_anchor ? 1 : 0; info->added = om->added ? 1 : 0;
    info->anchor_x = om->anchor[0]; info->anchor_y = om->anchor[1];
    info->width = (int32_t)om->window.w; info->height = (int32_t)om->window.h;
    info->origin_x = (int32_t)om->window.x0; info->origin_y = (int32_t)om->window.y0;
    info->offset_x = om->anchor[0] + (double)om->window.x0 * om->resolution;
    info->offset_y = om->anchor[1] + (double)om->window.y0 * om->resolution;
    info->alloc_width = (int32_t)om->alloc.w; info->alloc_height = (int32_t)om->alloc.h;
    info->alloc_origin_x = (int32_t)om->alloc.x0; info->alloc_origin_y = (int32_t)om->alloc.y0;
    info->reallocations = om->reallocations;
    return YM_OK;
}

// the window can be read: something was added and it has both a width and a height
static int occmap_readable(const ym_occmap *om) {
    if (!om->added) return set_err(YM_ERR_INVALID, "nothing has been added yet: nothing to read");
    if (om->window.empty()) return set_err(YM_ERR_UNSUPPORTED, "occupancy grid of %lld x %lld cells", (long long)om->window.w, (long long)om->window.h);
    return YM_OK;
}

int ym_occmap_read(ym_occmap *om, uint8_t *image, int64_t bytes, const ym_despeckle_opts *clean, ym_despeckle_stats *stats) {
    if (!om || !image) return set_err(YM_ERR_INVALID, "null argument");
    int rc;
    if (clean && (rc = despeckle_check_opts(*clean))) return rc;
    if ((rc = occmap_readable(om))) return rc;
    const size_t n = (size_t)om->window.cells();
    if (bytes < 0 || (size_t)bytes != n) return set_err(YM_ERR_INVALID, "buffer of %lld bytes: the window has %zu", (long long)bytes, n);
    if (clean && n > (size_t)INT32_MAX)
        return set_err(YM_ERR_UNSUPPORTED, "occupancy grid of %lld x %lld cells: the filter takes at most 2^31 - 1", (long long)om->window.w, (long long)om->window.h);
    DEV_GUARD(om->device);
    if ((rc = om->img.ensure(n))) return rc;
    ym::OccArgs a;
    std::memset(&a, 0, sizeof a);
    a.pitch = om->alloc.w; a.pass = om->cnt.p; a.hits = om->cnt.p + (size_t)om->alloc.cells();
    a.win_x = (int32_t)(om->window.x0 - om->alloc.x0); a.win_y = (int32_t)(om->window.y0 - om->alloc.y0);
    a.win_w = (int32_t)om->window.w; a.win_h = (int32_t)om->window.h;
    a.image = om->img.p;
    hipLaunchKernelGGL(ym::occ_update_kernel, dim3((unsigned)((a.win_w + 255) / 256), (unsigned)std::min(a.win_h, 65535)), dim3(256), 0, nullptr, a);
    HIP_TRY(hipGetLastError());
    ym_despeckle_stats s{};
    if (clean && (rc = despeckle_run(om->img.p, om->img.p, a.win_w, a.win_h, *clean, nullptr, &s))) return rc;
    HIP_TRY(hipMemcpy(image, om->img.p, n, hipMemcpyDeviceToHost));
    if (clean && stats) *stats = s;
    return YM_OK;
}

int ym_occmap_read_counts(ym_occmap *om, uint32_t *pass, uint32_t *hits, int64_t cells) {
    if (!om || !pass || !hits) return set_err(YM_ERR_INVALID, "null argument");
    int rc;
    if ((rc = occmap_readable(om))) return rc;
    const size_t n = (size_t)om->window.cells();
    if (cells < 0 || (size_t)cells != n) return set_err(YM_ERR_INVALID, "buffers of %lld cells: the window has %zu", (long long)cells, n);
    DEV_GUARD(om->device);
    const size_t row = (size_t)om->window.w * sizeof(unsigned), pitch = (size_t)om->alloc.w * sizeof(unsigned);
    const unsigned *src = om->cnt.p + (size_t)ymw::cell_offset(om->alloc, om->window.x0, om->window.y0); // (the memory holds the window)
    HIP_TRY(hipMemcpy2D(pass, row, src, pitch, row, (size_t)om->window.h, hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy2D(hits, row, src + (size_t)om->alloc.cells(), pitch, row, (size_t)om->window.h, hipMemcpyDeviceToHost));
    return YM_OK;
}
