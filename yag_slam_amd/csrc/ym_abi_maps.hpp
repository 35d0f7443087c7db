// ym_abi_maps.hpp -- C ABI: resident correlation maps: made, grown, forgotten from, reframed, matched against.
// The host side that the map-changing calls share is ym_host_mapgrow.hpp, the matchers' scoring tail ym_host_mapscore.hpp.
// Part of yagmatch.hip (included inside its extern "C" block); not a header of its own.
// ---- prebuilt maps: the "match against a map" entry of the reference's Python matcher
static ym_map *map_alloc(ym_matcher *m, int width, int height) {
    if (!m) { set_err(YM_ERR_INVALID, "null matcher"); return nullptr; }
    if (m->cfg.semantics != YM_SEM_YAGPY) {
        set_err(YM_ERR_UNSUPPORTED, "maps exist only in the reference's Python matcher: create the matcher with YM_SEM_YAGPY");
        return nullptr;
    }
    if (width <= 0 || height <= 0 || (double)width * height > 1.0e9) { set_err(YM_ERR_INVALID, "bad map size %d x %d", width, height); return nullptr; }
    ym_map *mp = new ym_map();
    mp->device = m->device;
    mp->width = width; mp->height = height;
    const size_t n = (size_t)width * height;
    if (mp->d_cgrid.alloc(n) != YM_OK || mp->d_g8.alloc(n + 64) != YM_OK) { // (the error text is set)
        delete mp;
        return nullptr;
    }
    return mp;
}

ym_map *ym_map_from_occupancy(ym_matcher *m, const uint8_t *image, int width, int height, int pitch, int occupied_value) {
    if (!image || pitch < width) { set_err(YM_ERR_INVALID, "bad occupancy image"); return nullptr; }
    DevGuard guard(m ? m->device : 0);
    ym_map *mp = map_alloc(m, width, height);
    if (!mp) return nullptr;
    const int ks = 2 * m->geom.half_kernel + 1;
    DevBuf<uint8_t> d_img;
    auto setup = [&]() -> int {
        int rc;
        if ((rc = d_img.alloc((size_t)pitch * height))) return rc;
        HIP_TRY(hipMemcpyAsync(d_img.p, image, (size_t)pitch * height, hipMemcpyHostToDevice, m->stream));
        if ((rc = map_taps_upload(m))) return rc;
        hipLaunchKernelGGL(ym::map_from_occupancy_kernel, dim3((width + 63) / 64, (height + 3) / 4), dim3(256), 0, m->stream, d_img.p, width,
                           height, pitch, occupied_value, m->kernel_f_dev.p, ks, mp->d_cgrid.p, mp->d_g8.p);
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipStreamSynchronize(m->stream));
        return YM_OK;
    };
    if (setup() != YM_OK) { delete mp; return nullptr; } // (the error text is set)
    return mp;
}

ym_map *ym_map_from_grid(ym_matcher *m, const double *cgrid, int width, int height) {
    if (!cgrid) { set_err(YM_ERR_INVALID, "null grid"); return nullptr; }
    DevGuard guard(m ? m->device : 0);
    ym_map *mp = map_alloc(m, width, height);
    if (!mp) return nullptr;
    const size_t n = (size_t)width * height;
    auto setup = [&]() -> int {
        HIP_TRY(hipMemcpyAsync(mp->d_cgrid.p, cgrid, n * sizeof(double), hipMemcpyHostToDevice, m->stream));
        hipLaunchKernelGGL(ym::map_from_grid_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, m->stream, mp->d_cgrid.p, n, mp->d_g8.p);
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipStreamSynchronize(m->stream));
        return YM_OK;
    };
    if (setup() != YM_OK) { delete mp; return nullptr; } // (the error text is set)
    return mp;
}

int ym_map_size(const ym_map *mp, int *width, int *height) {
    if (!mp) return set_err(YM_ERR_INVALID, "null map");
    if (width) *width = mp->width;
    if (height) *height = mp->height;
    return YM_OK;
}

int ym_map_read(const ym_map *mp, double *out, int64_t out_count) {
    if (!mp || !out) return set_err(YM_ERR_INVALID, "null argument");
    const size_t n = (size_t)mp->width * mp->height;
    if ((size_t)out_count < n) return set_err(YM_ERR_INVALID, "buffer too small: need %zu entries", n);
    DEV_GUARD(mp->device);
    HIP_TRY(hipMemcpy(out, mp->d_cgrid.p, n * sizeof(double), hipMemcpyDeviceToHost));
    return YM_OK;
}

void ym_map_destroy(ym_map *mp) {
    if (!mp) return;
    DevGuard guard(mp->device);
    delete mp;
}

// ---- maps that take scans (ym_k_mapgrow.hpp)
static int map_clear(ym_matcher *m, ym_map *mp) {
    const size_t n = (size_t)mp->width * mp->height;
    hipLaunchKernelGGL(ym::map_clear_kernel, dim3((unsigned)((n + 2047) / 2048)), dim3(256), 0, m->stream, mp->d_cgrid.p, mp->d_g8.p, n);
    HIP_TRY(hipGetLastError());
    if (mp->counted) { // (the flags are zero between calls; a call that failed half way may have left some)
        HIP_TRY(hipMemsetAsync(mp->d_stamps.p, 0, n * sizeof(uint32_t), m->stream));
        HIP_TRY(hipMemsetAsync(mp->d_dirty.p, 0, n, m->stream));
    }
    HIP_TRY(hipStreamSynchronize(m->stream));
    return YM_OK;
}

ym_map *ym_map_create_empty(ym_matcher *m, int width, int height) {
    DevGuard guard(m ? m->device : 0);
    ym_map *mp = map_alloc(m, width, height);
    if (!mp) return nullptr;
    if (map_clear(m, mp) != YM_OK) { delete mp; return nullptr; } // (the error text is set)
    return mp;
}

ym_map *ym_map_create_counted(ym_matcher *m, int width, int height, double ox, double oy) {
    return ym_map_create_counted_window(m, width, height, ox, oy, 0, 0);
}

ym_map *ym_map_create_counted_window(ym_matcher *m, int width, int height, double ax, double ay, int x0, int y0) {
    if (!ymm::offset_ok(x0, y0)) {
        set_err(YM_ERR_INVALID, "window offset (%d, %d): at most 2^30 cells either way", x0, y0);
        return nullptr;
    }
    DevGuard guard(m ? m->device : 0);
    ym_map *mp = map_alloc(m, width, height);
    if (!mp) return nullptr;
    const size_t n = (size_t)width * height;
    mp->counted = true; mp->ox = ax; mp->oy = ay; mp->x0 = x0; mp->y0 = y0;
    if (mp->d_stamps.alloc(n) != YM_OK || mp->d_dirty.alloc(n) != YM_OK || map_clear(m, mp) != YM_OK) { // (the error text is set)
        delete mp;
        return nullptr;
    }
    return mp;
}

int ym_map_counted(const ym_map *mp) { return mp && mp->counted ? 1 : 0; }

int ym_map_read_stamps(const ym_map *mp, uint32_t *out, int64_t out_count) {
    if (!mp || !out) return set_err(YM_ERR_INVALID, "null argument");
    if (!mp->counted) return set_err(YM_ERR_UNSUPPORTED, "this map keeps no counts: use ym_map_create_counted");
    const size_t n = (size_t)mp->width * mp->height;
    if (out_count < 0 || (size_t)out_count < n) return set_err(YM_ERR_INVALID, "buffer too small: need %zu entries", n);
    DEV_GUARD(mp->device);
    HIP_TRY(hipMemcpy(out, mp->d_stamps.p, n * sizeof(uint32_t), hipMemcpyDeviceToHost));
    return YM_OK;
}

int ym_map_clear(ym_matcher *m, ym_map *mp) {
    int rc;
    if ((rc = map_call_check(m, mp, "ym_map_clear"))) return rc;
    DEV_GUARD(m->device);
    return map_clear(m, mp);
}

// A counted map's one way to change (ym_map_update_scans, and ym_map_add_scans with nothing to remove): `remove` out at remove_poses,
// `add` in at the scans' own poses.  The caller has checked m, mp, the semantics and the map's device.
static int map_update(ym_matcher *m, ym_map *mp, const ym_scan *const *remove, const double *remove_poses, int n_remove,
                      const ym_scan *const *add, int n_add, ym_map_update_stats *stats) {
    int max_n = 1, rc;
    size_t remove_beams = 0;
    if ((rc = map_scan_list(m, remove, n_remove, "removed scan", &max_n, &remove_beams))) return rc;
    if ((rc = map_scan_list(m, add, n_add, "scan", &max_n))) return rc;
    ym_map_update_stats s;
    std::memset(&s, 0, sizeof s);
    if (n_remove == 0 && n_add == 0) {
        if (stats) *stats = s;
        return YM_OK;
    }
    const int ks = map_ksize(m), half = m->geom.half_kernel;
    if ((rc = map_launch_limits(max_n, ks, n_remove > 0))) return rc;
    DEV_GUARD(m->device);
    hipStream_t st = m->stream;
    const size_t n_cells = (size_t)mp->width * mp->height;
    enum { kRem = 0, kAdd = 1 }; // the job's two blocks of stamp statistics
    MapJob job;                  // (lives until the stream waits below)
    if ((rc = map_workspace(m, std::max(n_remove, n_add), max_n)) || (rc = map_taps_upload(m)) ||
        (rc = m->grow_released.ensure(std::min(remove_beams, n_cells))) || (rc = job.begin(m, n_remove + n_add, 2, true)))
        return rc;
    const MapTarget target = {mp->d_cgrid.p, mp->d_g8.p, mp->d_stamps.p, mp->d_dirty.p, mp->width, mp->height, mp->ox, mp->oy, mp->x0, mp->y0, ymm::Box()};
    const MapPassArgs pa = map_pass_args(m, target, max_n);
    // the removes first, all of them: a count falls to zero at most once in a call
    if ((rc = map_stamp_pass(m, job, pa, remove, remove_poses, n_remove, kMapCountRemove, false, kRem))) return rc;
    if ((rc = map_stamp_pass(m, job, pa, add, nullptr, n_add, kMapCountAdd, true, kAdd))) return rc;
    if ((rc = job.fetch(m))) return rc;
    HIP_TRY(hipStreamSynchronize(st));
    const unsigned long long *gr = job.got + kRem * ym::kMgStatSlots, *ga = job.got + kAdd * ym::kMgStatSlots, *gu = job.got + job.upd;
    s.unmatched = (int64_t)gu[ym::kMuUnmatched]; s.released = (int64_t)gu[ym::kMuReleased]; s.gained = (int64_t)gu[ym::kMuGained];
    s.removed = (int64_t)gr[ym::kMgStamped] - s.unmatched; s.added = (int64_t)ga[ym::kMgStamped];
    s.dropped = (int64_t)gr[ym::kMgDropped] + (int64_t)ga[ym::kMgDropped];
    ymm::Box changed; // both boxes widened by the taps' reach and cut to the map
    if (s.added > 0) changed = ymm::widen_stats(ga + ym::kMgX0, half, mp->width, mp->height);
    if (s.released > 0) {
        // the recompute: launches of their own after the smear's atomics, so the counts and the cells they read are complete
        const ymm::Box rbox = ymm::widen_stats(gu + ym::kMuX0, half, mp->width, mp->height);
        ym::MapForgetArgs f = pa.f;
        const int piece = (int)(2147483647u / (unsigned)(ks * ks)); // released cells of one mark launch
        for (int64_t r0 = 0; r0 < s.released; r0 += piece) {
            f.first = (int)r0; f.count = (int)std::min<int64_t>(piece, s.released - r0);
            hipLaunchKernelGGL(ym::map_forget_mark_kernel, dim3((unsigned)(((size_t)f.count * ks * ks + 255) / 256)), dim3(256), 0, st, f);
        }
        if ((rc = map_recompute(m, f, rbox))) return rc;
        HIP_TRY(hipStreamSynchronize(st));
        changed = ymm::join(changed, rbox);
    }
    if (!changed.empty()) { s.x0 = changed.x0; s.y0 = changed.y0; s.x1 = changed.x1; s.y1 = changed.y1; }
    if (stats) *stats = s;
    return YM_OK;
}

int ym_map_update_scans(ym_matcher *m, ym_map *mp, const ym_scan *const *remove, const double *remove_poses, int n_remove,
                        const ym_scan *const *add, int n_add, ym_map_update_stats *stats) {
    if ((n_remove != 0 && (!remove || !remove_poses)) || (n_add != 0 && !add)) return set_err(YM_ERR_INVALID, "null argument");
    if (n_remove < 0 || n_add < 0) return set_err(YM_ERR_INVALID, "n_remove and n_add must not be negative");
    int rc;
    if ((rc = map_call_check(m, mp, "ym_map_update_scans"))) return rc;
    if (!mp->counted) return set_err(YM_ERR_UNSUPPORTED, "this map keeps no counts and cannot forget: use ym_map_create_counted");
    return map_update(m, mp, remove, remove_poses, n_remove, add, n_add, stats);
}

// ---- maps that notice change (ym_k_seenthrough.hpp): which held readings do the viewers look through
int ym_map_seen_through(ym_matcher *m, const ym_map *mp, const ym_scan *const *held, const double *held_poses, int n_held,
                        const ym_scan *const *viewers, int n_viewers, int clearance, int protect, int32_t *counts, uint8_t *flags,
                        uint8_t *mask, ym_map_seen_stats *stats) {
    if ((n_held != 0 && (!held || !held_poses || !counts)) || (n_viewers != 0 && !viewers)) return set_err(YM_ERR_INVALID, "null argument");
    if (n_held < 0 || n_viewers < 0) return set_err(YM_ERR_INVALID, "n_held and n_viewers must not be negative");
    if (clearance < 0 || protect < 0) return set_err(YM_ERR_INVALID, "clearance and protect must not be negative");
    int rc;
    if ((rc = map_call_check(m, mp, "ym_map_seen_through"))) return rc;
    if (!mp->counted) return set_err(YM_ERR_UNSUPPORTED, "this map keeps no counts and holds no scans: use ym_map_create_counted");
    // the sweep's 32-bit walk: 2 k dm + dM stays below 2^31 while a ray has fewer than 2^15 major steps
    if (!(m->cfg.range_threshold / m->cfg.resolution + 2.0 < 32768.0))
        return set_err(YM_ERR_UNSUPPORTED, "a range threshold of %g m at %g m per cell: rays of 32768 cells or more", m->cfg.range_threshold,
                       m->cfg.resolution);
    int held_n = 1, view_n = 1;
    if ((rc = map_scan_list(m, held, n_held, "held scan", &held_n)) || (rc = map_scan_list(m, viewers, n_viewers, "viewer", &view_n))) return rc;
    const double side = 2.0 * protect + 1.0;
    if ((double)view_n * side * side > 2.0e9)
        return set_err(YM_ERR_UNSUPPORTED, "%d beams x %.0f x %.0f protected cells: more than one launch holds", view_n, side, side);
    DEV_GUARD(m->device);
    hipStream_t st = m->stream;
    const size_t n_cells = (size_t)mp->width * mp->height;
    ym::SeenArgs s;
    std::memset(&s, 0, sizeof s);
    s.width = mp->width; s.height = mp->height; s.ox = mp->ox; s.oy = mp->oy; s.res = m->cfg.resolution; s.wx0 = mp->x0; s.wy0 = mp->y0;
    s.clearance = clearance; s.protect = protect;
    if ((rc = m->seen_mask.ensure(n_cells))) return rc;
    s.mask = m->seen_mask.p;
    HIP_TRY(hipMemsetAsync(s.mask, 0, n_cells, st));
    // the viewers at their current poses: every sweep, then every protect launch (a protected cell stays clear of all rays)
    std::vector<YmScanRef> vrefs((size_t)n_viewers); // (the copies below read these until the stream wait)
    std::vector<int32_t> walked;
    const unsigned sweep_x = (unsigned)((view_n + ym::kSeenRaysPerBlock - 1) / ym::kSeenRaysPerBlock);
    if (n_viewers > 0) {
        walked.assign((size_t)n_viewers * sweep_x, 0);
        if ((rc = m->seen_viewers.ensure((size_t)n_viewers)) || (rc = m->seen_walked.ensure(walked.size()))) return rc;
        for (int i = 0; i < n_viewers; i++) vrefs[(size_t)i] = scan_ref(viewers[i]);
        HIP_TRY(hipMemcpyAsync(m->seen_viewers.p, vrefs.data(), sizeof(YmScanRef) * (size_t)n_viewers, hipMemcpyHostToDevice, st));
        s.max_n = view_n;
        const unsigned protect_x = (unsigned)(((size_t)view_n * (size_t)(side * side) + 255) / 256);
        for (int stage = 0; stage < 2; stage++) {
            for (int c0 = 0; c0 < n_viewers; c0 += kMapGrowChunk) {
                const int B = std::min(kMapGrowChunk, n_viewers - c0);
                s.scans = m->seen_viewers.p + c0;
                s.walked = m->seen_walked.p + (size_t)c0 * sweep_x;
                if (stage == 0) hipLaunchKernelGGL(ym::seen_sweep_kernel, dim3(sweep_x, B), dim3(256), 0, st, s);
                else hipLaunchKernelGGL(ym::seen_protect_kernel, dim3(protect_x, B), dim3(256), 0, st, s);
            }
        }
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipMemcpyAsync(walked.data(), m->seen_walked.p, sizeof(int32_t) * walked.size(), hipMemcpyDeviceToHost, st));
    }
    // the held scans at the poses they were added at: map_grow_cells_kernel's cells (no exclusion rectangle), then the counts
    MapJob job; // (lives until the stream wait below)
    if (n_held > 0) {
        if ((rc = map_workspace(m, n_held, held_n)) || (rc = job.begin(m, n_held, 1, false)) || (rc = m->seen_counts.ensure(2 * (size_t)n_held)) ||
            (flags && (rc = m->seen_flags.ensure((size_t)n_held * held_n))))
            return rc;
        const MapTarget target = {nullptr, nullptr, nullptr, nullptr, mp->width, mp->height, mp->ox, mp->oy, mp->x0, mp->y0, ymm::Box()};
        MapPassArgs pa = map_pass_args(m, target, held_n);
        s.scans = nullptr; s.walked = nullptr;
        s.max_n = held_n; s.cells = m->grow_cells.p; s.counts = m->seen_counts.p; s.flags = flags ? m->seen_flags.p : nullptr;
        pa.s = s;
        if ((rc = map_stamp_pass(m, job, pa, held, held_poses, n_held, kMapCountSeen, false, 0))) return rc;
        HIP_TRY(hipMemcpyAsync(counts, m->seen_counts.p, sizeof(int32_t) * 2 * (size_t)n_held, hipMemcpyDeviceToHost, st));
        if (flags) HIP_TRY(hipMemcpyAsync(flags, m->seen_flags.p, (size_t)n_held * held_n, hipMemcpyDeviceToHost, st));
    }
    if (mask) HIP_TRY(hipMemcpyAsync(mask, s.mask, n_cells, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    if (stats) {
        stats->rays = stats->inside = stats->seen = 0;
        for (int32_t w : walked) stats->rays += w;
        for (int i = 0; i < n_held; i++) { stats->inside += counts[2 * (size_t)i]; stats->seen += counts[2 * (size_t)i + 1]; }
    }
    return YM_OK;
}

int ym_map_add_scans(ym_matcher *m, ym_map *mp, double ox, double oy, const ym_scan *const *scans, int n_scans, ym_map_add_stats *stats) {
    if (!scans && n_scans != 0) return set_err(YM_ERR_INVALID, "null argument");
    if (n_scans < 0) return set_err(YM_ERR_INVALID, "n_scans must not be negative");
    int rc;
    if ((rc = map_call_check(m, mp, "ym_map_add_scans"))) return rc;
    ym_map_add_stats s;
    std::memset(&s, 0, sizeof s);
    if (mp->counted) { // the counts go up with the stamps
        // the window's origin, from the anchor and the whole offset (never step by step: section 17); the anchor itself at offset 0
        const double wox = mp->ox + mp->x0 * m->cfg.resolution, woy = mp->oy + mp->y0 * m->cfg.resolution;
        if (!(ox == wox && oy == woy))
            return set_err(YM_ERR_INVALID, "a counted map keeps its origin: that of its window is (%.17g, %.17g)", wox, woy);
        ym_map_update_stats u;
        if ((rc = map_update(m, mp, nullptr, nullptr, 0, scans, n_scans, &u))) return rc;
        s.points = u.added + u.dropped; s.stamped = u.added; s.dropped = u.dropped;
        s.x0 = u.x0; s.y0 = u.y0; s.x1 = u.x1; s.y1 = u.y1;
        if (stats) *stats = s;
        return YM_OK;
    }
    int max_n = 1;
    if ((rc = map_scan_list(m, scans, n_scans, "scan", &max_n))) return rc;
    if (n_scans == 0) {
        if (stats) *stats = s;
        return YM_OK;
    }
    if ((rc = map_launch_limits(max_n, map_ksize(m), false))) return rc;
    DEV_GUARD(m->device);
    MapJob job; // (lives until the stream wait below)
    if ((rc = map_workspace(m, n_scans, max_n)) || (rc = map_taps_upload(m)) || (rc = job.begin(m, n_scans, 1, false))) return rc;
    // an uncounted map takes the caller's origin as it is, at offset 0
    const MapTarget target = {mp->d_cgrid.p, mp->d_g8.p, nullptr, nullptr, mp->width, mp->height, ox, oy, 0, 0, ymm::Box()};
    if ((rc = map_stamp_pass(m, job, map_pass_args(m, target, max_n), scans, nullptr, n_scans, kMapCountNone, true, 0))) return rc;
    if ((rc = job.fetch(m))) return rc;
    HIP_TRY(hipStreamSynchronize(m->stream));
    const unsigned long long *got = job.got;
    s.points = (int64_t)got[ym::kMgPoints]; s.stamped = (int64_t)got[ym::kMgStamped]; s.dropped = (int64_t)got[ym::kMgDropped];
    if (s.stamped > 0) { // the stamped cells' box, widened by the taps' reach and cut to the map
        const ymm::Box b = ymm::widen_stats(got + ym::kMgX0, m->geom.half_kernel, mp->width, mp->height);
        s.x0 = b.x0; s.y0 = b.y0; s.x1 = b.x1; s.y1 = b.y1;
    }
    if (stats) *stats = s;
    return YM_OK;
}

// ---- maps whose window moves (ym_k_mapgrow.hpp)
int ym_map_window(const ym_map *mp, int *x0, int *y0, int *width, int *height) {
    if (!mp) return set_err(YM_ERR_INVALID, "null map");
    if (x0) *x0 = mp->x0;
    if (y0) *y0 = mp->y0;
    if (width) *width = mp->width;
    if (height) *height = mp->height;
    return YM_OK;
}

int ym_map_reframe(ym_matcher *m, ym_map *mp, int dx, int dy, int width, int height, const ym_scan *const *held,
                   const double *held_poses, int n_held, ym_map_reframe_stats *stats) {
    if (n_held != 0 && (!held || !held_poses)) return set_err(YM_ERR_INVALID, "null argument");
    if (n_held < 0) return set_err(YM_ERR_INVALID, "n_held must not be negative");
    if (width <= 0 || height <= 0 || (double)width * height > 1.0e9) return set_err(YM_ERR_INVALID, "bad map size %d x %d", width, height);
    int rc;
    if ((rc = map_call_check(m, mp, "ym_map_reframe"))) return rc;
    const int64_t nx0 = (int64_t)mp->x0 + dx, ny0 = (int64_t)mp->y0 + dy;
    if (!ymm::offset_ok(nx0, ny0))
        return set_err(YM_ERR_INVALID, "window offset (%lld, %lld): at most 2^30 cells either way", (long long)nx0, (long long)ny0);
    if (!mp->counted && n_held != 0) return set_err(YM_ERR_INVALID, "this map keeps no counts and holds no scans: n_held must be 0");
    int max_n = 1;
    if ((rc = map_scan_list(m, held, n_held, "held scan", &max_n))) return rc;
    const int half = m->geom.half_kernel;
    if (mp->counted && (rc = map_launch_limits(max_n, map_ksize(m), true))) return rc;
    ym_map_reframe_stats s;
    std::memset(&s, 0, sizeof s);
    s.x0 = mp->x0; s.y0 = mp->y0; s.width = mp->width; s.height = mp->height;
    if (dx == 0 && dy == 0 && width == mp->width && height == mp->height) { // the identity: nothing to do
        s.kept = (int64_t)width * height;
        if (stats) *stats = s;
        return YM_OK;
    }
    const ymm::Box ov = ymm::overlap(mp->width, mp->height, dx, dy, width, height); // in cells of the new window
    const bool overlap = !ov.empty();
    const ymm::Shift shift = ymm::copy_shift(overlap, dx, dy);
    DEV_GUARD(m->device);
    hipStream_t st = m->stream;
    const size_t n = (size_t)width * height;
    // everything is built in arrays of its own and traded in when all of it is complete: whatever fails, the map is as it was
    DevBuf<double> n_cgrid;
    DevBuf<uint8_t> n_g8, n_dirty;
    DevBuf<uint32_t> n_stamps;
    DevBuf<unsigned long long> d_stats;
    if ((rc = n_cgrid.alloc(n)) || (rc = n_g8.alloc(n + 64)) || (rc = d_stats.alloc(2))) return rc;
    if (mp->counted && ((rc = n_stamps.alloc(n)) || (rc = n_dirty.alloc(n)))) return rc;
    HIP_TRY(hipMemsetAsync(d_stats.p, 0, 2 * sizeof(unsigned long long), st));
    HIP_TRY(hipMemsetAsync(n_g8.p + n, 0, 64, st));
    ym::MapReframeArgs r;
    std::memset(&r, 0, sizeof r);
    r.src_cgrid = mp->d_cgrid.p; r.src_g8 = mp->d_g8.p; r.src_stamps = mp->d_stamps.p; r.src_w = mp->width; r.src_h = mp->height;
    r.dx = shift.dx; r.dy = shift.dy; r.width = width; r.height = height;
    r.cgrid = n_cgrid.p; r.g8 = n_g8.p; r.stamps = n_stamps.p; r.dirty = n_dirty.p; r.stats = d_stats.p; r.half = half;
    const dim3 groups((unsigned)((n + 1023) / 1024));
    if (mp->counted) hipLaunchKernelGGL(ym::map_reframe_copy_kernel<true>, groups, dim3(256), 0, st, r);
    else hipLaunchKernelGGL(ym::map_reframe_copy_kernel<false>, groups, dim3(256), 0, st, r);
    HIP_TRY(hipGetLastError());
    if (overlap) s.kept = (int64_t)(ov.x1 - ov.x0) * (ov.y1 - ov.y0);
    if (mp->counted) {
        MapJob job; // (lives until the stream wait below)
        unsigned long long got_r[2] = {0, 0};
        if ((rc = map_taps_upload(m))) return rc;
        if (n_held > 0 && ((rc = map_workspace(m, n_held, max_n)) || (rc = job.begin(m, n_held, 1, true)))) return rc;
        const MapTarget target = {n_cgrid.p, n_g8.p, n_stamps.p, n_dirty.p, width, height, mp->ox, mp->oy, (int)nx0, (int)ny0, ov};
        const MapPassArgs pa = map_pass_args(m, target, max_n);
        if (n_held > 0) { // the restamp: what the old window dropped and the new one holds
            if ((rc = map_stamp_pass(m, job, pa, held, held_poses, n_held, kMapCountAdd, true, 0))) return rc;
            if ((rc = job.fetch(m))) return rc;
        }
        if (overlap) {
            // the recompute, after the restamp's atomics: the cells within the taps' reach of the overlap whose neighbourhood meets
            // the two windows differently are flagged and take their value from the new window's counts
            const ymm::Box rect = ymm::mark_rect(ov, half, width, height);
            if ((rc = map_reframe_mark(m, r, rect)) || (rc = map_recompute(m, pa.f, rect))) return rc;
        }
        HIP_TRY(hipMemcpyAsync(got_r, d_stats.p, sizeof got_r, hipMemcpyDeviceToHost, st));
        HIP_TRY(hipStreamSynchronize(st));
        int64_t in_overlap = 0;
        if (n_held > 0) {
            s.restamped = (int64_t)job.got[ym::kMgStamped]; s.dropped = (int64_t)job.got[ym::kMgDropped];
            in_overlap = (int64_t)job.got[ym::kMgOverlap];
        }
        s.recomputed = (int64_t)got_r[1];
        const int64_t copied = (int64_t)got_r[0];
        s.mismatch = copied > in_overlap ? copied - in_overlap : in_overlap - copied;
        if (s.mismatch != 0) { // the counts and the scans said to be held disagree: the new arrays go, the map stays
            s.kept = s.restamped = s.dropped = s.recomputed = 0;
            if (stats) *stats = s;
            return set_err(YM_ERR_INVALID, "the kept cells count %lld readings and the held scans put %lld there: nothing was changed",
                           (long long)copied, (long long)in_overlap);
        }
    } else {
        HIP_TRY(hipStreamSynchronize(st));
    }
    // the stream is idle: trade the arrays in (the old ones are freed with the locals)
    mp->d_cgrid.swap(n_cgrid); mp->d_g8.swap(n_g8);
    if (mp->counted) { mp->d_stamps.swap(n_stamps); mp->d_dirty.swap(n_dirty); }
    mp->width = width; mp->height = height; mp->x0 = (int)nx0; mp->y0 = (int)ny0;
    s.x0 = mp->x0; s.y0 = mp->y0; s.width = width; s.height = height;
    if (stats) *stats = s;
    return YM_OK;
}

int ym_match_map(ym_matcher *m, const ym_map *mp, double ox, double oy, const ym_scan *const *queries, int n_queries,
                 int penalize, int refine, const ym_map_search *coarse, ym_result *out) {
    if (!m || !mp || !queries || !out) return set_err(YM_ERR_INVALID, "null argument");
    if (m->cfg.semantics != YM_SEM_YAGPY) return set_err(YM_ERR_UNSUPPORTED, "ym_match_map needs a YM_SEM_YAGPY matcher");
    if (n_queries <= 0 || n_queries > 64) return set_err(YM_ERR_INVALID, "n_queries must be in [1, 64]");
    if (mp->device != m->device) return set_err(YM_ERR_INVALID, "map lives on another device");
    DEV_GUARD(m->device);
    double ox_real, oy_real; // the search centre
    int total = 0, max_n = 1, rc;
    if ((rc = yag_set_centre(m, queries, n_queries, -1, &ox_real, &oy_real, &total, &max_n))) return rc;
    total = std::max(total, 1);
    ym_map_search cs;
    YagLattice L;
    if ((rc = map_search_params(coarse, &cs)) || (rc = yag_lattice_bound(cs, m->cfg.resolution, "map ", &L))) return rc;
    const int maxd = L.maxd, maxt = L.maxt;
    const size_t vol = L.vol;
    Slot &slot = m->slots[kAsyncSlots];
    if (slot.in_flight) return set_err(YM_ERR_BUSY, "the synchronous slot is in flight");
    const size_t scans_bytes = align_up(sizeof(YmScanRef) * n_queries, 16);
    if ((rc = m->states.ensure(1)) || (rc = m->map_pts.ensure((size_t)total)) || (rc = m->yaxes.ensure((size_t)3 * YM_YAG_MAX_DIM)) ||
        (rc = m->yrot.ensure((size_t)maxt * total)) || (rc = m->sums.ensure(2 * vol)) || (rc = m->resp.ensure(vol)) ||
        (rc = slot.desc.ensure(scans_bytes + sizeof(YmItemState))) || (rc = slot.result.ensure(sizeof(YmItemState))) ||
        (rc = m->desc_dev.ensure(scans_bytes)))
        return rc;
    slot.desc_live_bytes = 0; // (the slot's pinned descriptor buffer is rewritten here)
    YmScanRef *hs = reinterpret_cast<YmScanRef *>(slot.desc.p);
    std::memset(hs, 0, scans_bytes);
    for (int i = 0; i < n_queries; i++) hs[i] = scan_ref(queries[i]);
    YmItemState *st0 = reinterpret_cast<YmItemState *>(slot.desc.p + scans_bytes);
    std::memset(st0, 0, sizeof *st0);
    st0->pose[0] = st0->center[0] = ox_real; st0->pose[1] = st0->center[1] = oy_real;
    st0->off_x = ox; st0->off_y = oy;
    st0->ql = m->map_pts.p;
    hipStream_t st = m->stream;
    HIP_TRY(hipMemcpyAsync(m->desc_dev.p, hs, scans_bytes, hipMemcpyHostToDevice, st));
    HIP_TRY(hipMemcpyAsync(m->states.p, st0, sizeof *st0, hipMemcpyHostToDevice, st));
    ym::MapPointsArgs pa;
    pa.scans = reinterpret_cast<const YmScanRef *>(m->desc_dev.p); pa.n_scans = n_queries; pa.max_n = max_n;
    pa.ox_real = ox_real; pa.oy_real = oy_real; pa.out = m->map_pts.p; pa.state = m->states.p;
    (void)hipFuncSetAttribute(reinterpret_cast<const void *>(ym::map_points_kernel), hipFuncAttributeMaxDynamicSharedMemorySize,
                              (int)YM_PREP_LDS_BYTES(YM_MAX_BEAMS));
    hipLaunchKernelGGL(ym::map_points_kernel, dim3(1), dim3(1024), YM_PREP_LDS_BYTES(max_n), st, pa);
    m->sums_pass_offset[0] = 0;
    m->sums_pass_offset[1] = vol;
    for (int pass = 0; pass < (refine ? 2 : 1); pass++) {
        ym::YagArgs a = yag_pass_args(m, cs, L, pass, penalize, refine);
        a.states = m->states.p; a.host_out = reinterpret_cast<YmItemState *>(slot.result.dp);
        a.rot = m->yrot.p;
        a.sums = m->sums.p + m->sums_pass_offset[pass];
        a.grid = mp->d_g8.p; a.grid_stride = 0;
        a.max_n = total;
        a.map_w = mp->width; a.map_h = mp->height; a.map_ox = ox; a.map_oy = oy;
        yag_frame_record(m, a, 1);
        hipLaunchKernelGGL(ym::yag_setup_kernel, dim3(maxt, 1), dim3(256), 0, st, a);
        hipLaunchKernelGGL(ym::yag_score_kernel, dim3((maxd * maxd + 255) / 256, maxt, 1), dim3(256), 0, st, a);
        hipLaunchKernelGGL(ym::yag_reduce_kernel<1024>, dim3(1), dim3(1024), 0, st, a);
    }
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipStreamSynchronize(st));
    yag_unpack_result(*reinterpret_cast<const YmItemState *>(slot.result.p), refine, out);
    map_last_set(m, 1, 0, refine ? 2 : 1, vol, vol);
    return YM_OK;
}
