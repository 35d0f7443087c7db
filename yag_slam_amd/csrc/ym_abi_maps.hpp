// ym_abi_maps.hpp -- C ABI: prebuilt maps (match against a map), occupancy-grid rendering
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
        if ((rc = m->kernel_f_dev.ensure(m->kernel_f.size()))) return rc;
        HIP_TRY(hipMemcpyAsync(m->kernel_f_dev.p, m->kernel_f.data(), m->kernel_f.size() * sizeof(double), hipMemcpyHostToDevice, m->stream));
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

static const int kMapMaxOffset = 1 << 30; // a window's offset in lattice cells: exact in fp64 and in the int32 of the kernels

ym_map *ym_map_create_counted(ym_matcher *m, int width, int height, double ox, double oy) {
    return ym_map_create_counted_window(m, width, height, ox, oy, 0, 0);
}

ym_map *ym_map_create_counted_window(ym_matcher *m, int width, int height, double ax, double ay, int x0, int y0) {
    if (x0 < -kMapMaxOffset || x0 > kMapMaxOffset || y0 < -kMapMaxOffset || y0 > kMapMaxOffset) {
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
    if (!m || !mp) return set_err(YM_ERR_INVALID, "null argument");
    if (m->cfg.semantics != YM_SEM_YAGPY) return set_err(YM_ERR_UNSUPPORTED, "ym_map_clear needs a YM_SEM_YAGPY matcher");
    if (mp->device != m->device) return set_err(YM_ERR_INVALID, "map lives on another device");
    DEV_GUARD(m->device);
    return map_clear(m, mp);
}

// scans of one launch: the cells of every beam take 4 bytes, grid.y stays far below its limit
static const int kMapGrowChunk = 4096;

// A counted map's one way to change (ym_map_update_scans, and ym_map_add_scans with nothing to remove): `remove` out at remove_poses,
// `add` in at the scans' own poses.  The caller has checked m, mp, the semantics and the map's device.
static int map_update(ym_matcher *m, ym_map *mp, const ym_scan *const *remove, const double *remove_poses, int n_remove,
                      const ym_scan *const *add, int n_add, ym_map_update_stats *stats) {
    int max_n = 1;
    size_t remove_beams = 0;
    for (int i = 0; i < n_remove; i++) {
        if (!remove[i] || remove[i]->device != m->device) return set_err(YM_ERR_INVALID, "removed scan %d is null or lives on another device", i);
        max_n = std::max(max_n, remove[i]->n);
        remove_beams += (size_t)remove[i]->n;
    }
    for (int i = 0; i < n_add; i++) {
        if (!add[i] || add[i]->device != m->device) return set_err(YM_ERR_INVALID, "scan %d is null or lives on another device", i);
        max_n = std::max(max_n, add[i]->n);
    }
    ym_map_update_stats s;
    std::memset(&s, 0, sizeof s);
    if (n_remove == 0 && n_add == 0) {
        if (stats) *stats = s;
        return YM_OK;
    }
    const int ks = 2 * m->geom.half_kernel + 1, half = m->geom.half_kernel;
    if ((double)max_n * ks * ks > 2.0e9) return set_err(YM_ERR_UNSUPPORTED, "%d beams x %d x %d taps: more than one launch holds", max_n, ks, ks);
    const size_t halo_bytes = (size_t)(ym::kMfTileW + ks - 1) * (size_t)(ym::kMfTileH + ks - 1);
    if (n_remove > 0 && halo_bytes > 65536)
        return set_err(YM_ERR_UNSUPPORTED, "%d x %d taps: the recompute's tile and halo (%zu bytes) do not fit 64 KiB of LDS", ks, ks, halo_bytes);
    DEV_GUARD(m->device);
    hipStream_t st = m->stream;
    const size_t n_cells = (size_t)mp->width * mp->height;
    const int chunk = std::min(std::max(n_remove, n_add), kMapGrowChunk);
    enum { kRem = 0, kAdd = ym::kMgStatSlots, kUpd = 2 * ym::kMgStatSlots, kSlots = 2 * ym::kMgStatSlots + ym::kMuStatSlots };
    int rc;
    if ((rc = m->grow_scans.ensure((size_t)chunk)) || (rc = m->grow_cells.ensure((size_t)chunk * max_n)) ||
        (rc = m->grow_stats.ensure(kSlots)) || (rc = m->kernel_f_dev.ensure(m->kernel_f.size())) ||
        (rc = m->grow_released.ensure(std::min(remove_beams, n_cells))))
        return rc;
    HIP_TRY(hipMemcpyAsync(m->kernel_f_dev.p, m->kernel_f.data(), m->kernel_f.size() * sizeof(double), hipMemcpyHostToDevice, st));
    // (what the copies of this call read on the host -- `init`, `all` -- stays as it is until the wait at the end)
    unsigned long long init[kSlots], got[kSlots];
    for (int i = 0; i < kSlots; i++) init[i] = 0;
    init[kRem + ym::kMgX0] = init[kRem + ym::kMgY0] = init[kAdd + ym::kMgX0] = init[kAdd + ym::kMgY0] = ~0ull;
    init[kUpd + ym::kMuX0] = init[kUpd + ym::kMuY0] = ~0ull;
    HIP_TRY(hipMemcpyAsync(m->grow_stats.p, init, sizeof init, hipMemcpyHostToDevice, st));
    std::vector<YmScanRef> all((size_t)n_remove + (size_t)n_add);
    ym::MapGrowArgs a;
    std::memset(&a, 0, sizeof a);
    a.scans = m->grow_scans.p; a.max_n = max_n; a.width = mp->width; a.height = mp->height;
    a.ox = mp->ox; a.oy = mp->oy; a.res = m->cfg.resolution; a.wx0 = mp->x0; a.wy0 = mp->y0;
    a.cells = m->grow_cells.p; a.kernel = m->kernel_f_dev.p; a.ksize = ks;
    a.cgrid = mp->d_cgrid.p; a.g8 = mp->d_g8.p;
    ym::MapForgetArgs f;
    std::memset(&f, 0, sizeof f);
    f.cells = m->grow_cells.p; f.max_n = max_n; f.width = mp->width; f.height = mp->height;
    f.stamps = mp->d_stamps.p; f.released = m->grow_released.p; f.stats = m->grow_stats.p + kUpd; f.dirty = mp->d_dirty.p;
    f.kernel = m->kernel_f_dev.p; f.ksize = ks; f.cgrid = mp->d_cgrid.p; f.g8 = mp->d_g8.p;
    const dim3 beams((unsigned)((max_n + 255) / 256)), taps((unsigned)(((size_t)max_n * ks * ks + 255) / 256));
    // the removes first, all of them: a count falls to zero at most once in a call
    a.stats = m->grow_stats.p + kRem;
    for (int c0 = 0; c0 < n_remove; c0 += chunk) {
        const int B = std::min(chunk, n_remove - c0);
        YmScanRef *hs = all.data() + c0;
        for (int i = 0; i < B; i++) hs[i] = scan_ref(remove[c0 + i], remove_poses + 3 * (size_t)(c0 + i));
        HIP_TRY(hipMemcpyAsync(m->grow_scans.p, hs, sizeof(YmScanRef) * (size_t)B, hipMemcpyHostToDevice, st));
        a.n_scans = B;
        hipLaunchKernelGGL(ym::map_grow_cells_kernel, dim3(B), dim3(1024), 0, st, a);
        hipLaunchKernelGGL(ym::map_count_kernel<true>, dim3(beams.x, B), dim3(256), 0, st, f);
        HIP_TRY(hipGetLastError());
    }
    a.stats = m->grow_stats.p + kAdd;
    for (int c0 = 0; c0 < n_add; c0 += chunk) {
        const int B = std::min(chunk, n_add - c0);
        YmScanRef *hs = all.data() + n_remove + c0;
        for (int i = 0; i < B; i++) hs[i] = scan_ref(add[c0 + i]);
        HIP_TRY(hipMemcpyAsync(m->grow_scans.p, hs, sizeof(YmScanRef) * (size_t)B, hipMemcpyHostToDevice, st));
        a.n_scans = B;
        hipLaunchKernelGGL(ym::map_grow_cells_kernel, dim3(B), dim3(1024), 0, st, a);
        hipLaunchKernelGGL(ym::map_count_kernel<false>, dim3(beams.x, B), dim3(256), 0, st, f);
        hipLaunchKernelGGL(ym::map_grow_smear_kernel<false>, dim3(taps.x, B), dim3(256), 0, st, a);
        hipLaunchKernelGGL(ym::map_grow_smear_kernel<true>, dim3(taps.x, B), dim3(256), 0, st, a);
        HIP_TRY(hipGetLastError());
    }
    HIP_TRY(hipMemcpyAsync(got, m->grow_stats.p, sizeof got, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    const unsigned long long *gr = got + kRem, *ga = got + kAdd, *gu = got + kUpd;
    s.unmatched = (int64_t)gu[ym::kMuUnmatched]; s.released = (int64_t)gu[ym::kMuReleased]; s.gained = (int64_t)gu[ym::kMuGained];
    s.removed = (int64_t)gr[ym::kMgStamped] - s.unmatched; s.added = (int64_t)ga[ym::kMgStamped];
    s.dropped = (int64_t)gr[ym::kMgDropped] + (int64_t)ga[ym::kMgDropped];
    int x0 = INT32_MAX, y0 = INT32_MAX, x1 = 0, y1 = 0; // the changed cells' box: both boxes widened by the taps' reach and cut to the map
    if (s.added > 0) {
        x0 = std::max(0, (int)ga[ym::kMgX0] - half); y0 = std::max(0, (int)ga[ym::kMgY0] - half);
        x1 = std::min(mp->width, (int)ga[ym::kMgX1] + half + 1); y1 = std::min(mp->height, (int)ga[ym::kMgY1] + half + 1);
    }
    if (s.released > 0) {
        // the recompute: a launch of its own after the smear's atomics, so the counts and the cells it reads are complete
        const int rx0 = std::max(0, (int)gu[ym::kMuX0] - half), ry0 = std::max(0, (int)gu[ym::kMuY0] - half);
        const int rx1 = std::min(mp->width, (int)gu[ym::kMuX1] + half + 1), ry1 = std::min(mp->height, (int)gu[ym::kMuY1] + half + 1);
        const int piece = (int)(2147483647u / (unsigned)(ks * ks)); // released cells of one mark launch
        for (int64_t r0 = 0; r0 < s.released; r0 += piece) {
            f.first = (int)r0; f.count = (int)std::min<int64_t>(piece, s.released - r0);
            hipLaunchKernelGGL(ym::map_forget_mark_kernel, dim3((unsigned)(((size_t)f.count * ks * ks + 255) / 256)), dim3(256), 0, st, f);
        }
        f.bx0 = rx0 / ym::kMfTileW * ym::kMfTileW; f.by0 = ry0 / ym::kMfTileH * ym::kMfTileH; f.bx1 = rx1; f.by1 = ry1;
        const dim3 tiles((unsigned)((f.bx1 - f.bx0 + ym::kMfTileW - 1) / ym::kMfTileW), (unsigned)((f.by1 - f.by0 + ym::kMfTileH - 1) / ym::kMfTileH));
        for (unsigned ty = 0; ty < tiles.y; ty += 65535u) { // (a launch has at most 65535 rows of blocks)
            ym::MapForgetArgs g = f;
            g.by0 = f.by0 + (int)ty * ym::kMfTileH;
            hipLaunchKernelGGL(ym::map_forget_gather_kernel, dim3(tiles.x, std::min(65535u, tiles.y - ty)), dim3(256), halo_bytes, st, g);
        }
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipStreamSynchronize(st));
        x0 = std::min(x0, rx0); y0 = std::min(y0, ry0); x1 = std::max(x1, rx1); y1 = std::max(y1, ry1);
    }
    if (x1 > x0 && y1 > y0) { s.x0 = x0; s.y0 = y0; s.x1 = x1; s.y1 = y1; }
    if (stats) *stats = s;
    return YM_OK;
}

int ym_map_update_scans(ym_matcher *m, ym_map *mp, const ym_scan *const *remove, const double *remove_poses, int n_remove,
                        const ym_scan *const *add, int n_add, ym_map_update_stats *stats) {
    if (!m || !mp || (n_remove != 0 && (!remove || !remove_poses)) || (n_add != 0 && !add)) return set_err(YM_ERR_INVALID, "null argument");
    if (n_remove < 0 || n_add < 0) return set_err(YM_ERR_INVALID, "n_remove and n_add must not be negative");
    if (m->cfg.semantics != YM_SEM_YAGPY) return set_err(YM_ERR_UNSUPPORTED, "ym_map_update_scans needs a YM_SEM_YAGPY matcher");
    if (mp->device != m->device) return set_err(YM_ERR_INVALID, "map lives on another device");
    if (!mp->counted) return set_err(YM_ERR_UNSUPPORTED, "this map keeps no counts and cannot forget: use ym_map_create_counted");
    return map_update(m, mp, remove, remove_poses, n_remove, add, n_add, stats);
}

int ym_map_add_scans(ym_matcher *m, ym_map *mp, double ox, double oy, const ym_scan *const *scans, int n_scans, ym_map_add_stats *stats) {
    if (!m || !mp || (!scans && n_scans != 0)) return set_err(YM_ERR_INVALID, "null argument");
    if (m->cfg.semantics != YM_SEM_YAGPY) return set_err(YM_ERR_UNSUPPORTED, "ym_map_add_scans needs a YM_SEM_YAGPY matcher");
    if (n_scans < 0) return set_err(YM_ERR_INVALID, "n_scans must not be negative");
    if (mp->device != m->device) return set_err(YM_ERR_INVALID, "map lives on another device");
    if (mp->counted) { // the counts go up with the stamps
        // the window's origin, from the anchor and the whole offset (never step by step: section 17); the anchor itself at offset 0
        const double wox = mp->ox + mp->x0 * m->cfg.resolution, woy = mp->oy + mp->y0 * m->cfg.resolution;
        if (!(ox == wox && oy == woy))
            return set_err(YM_ERR_INVALID, "a counted map keeps its origin: that of its window is (%.17g, %.17g)", wox, woy);
        ym_map_update_stats u;
        int rc;
        if ((rc = map_update(m, mp, nullptr, nullptr, 0, scans, n_scans, &u))) return rc;
        if (stats) {
            std::memset(stats, 0, sizeof *stats);
            stats->points = u.added + u.dropped; stats->stamped = u.added; stats->dropped = u.dropped;
            stats->x0 = u.x0; stats->y0 = u.y0; stats->x1 = u.x1; stats->y1 = u.y1;
        }
        return YM_OK;
    }
    int max_n = 1;
    for (int i = 0; i < n_scans; i++) {
        if (!scans[i] || scans[i]->device != m->device) return set_err(YM_ERR_INVALID, "scan %d is null or lives on another device", i);
        max_n = std::max(max_n, scans[i]->n);
    }
    ym_map_add_stats s;
    std::memset(&s, 0, sizeof s);
    if (n_scans == 0) {
        if (stats) *stats = s;
        return YM_OK;
    }
    const int ks = 2 * m->geom.half_kernel + 1, half = m->geom.half_kernel;
    if ((double)max_n * ks * ks > 2.0e9) return set_err(YM_ERR_UNSUPPORTED, "%d beams x %d x %d taps: more than one launch holds", max_n, ks, ks);
    DEV_GUARD(m->device);
    hipStream_t st = m->stream;
    const int chunk = std::min(n_scans, kMapGrowChunk);
    int rc;
    if ((rc = m->grow_scans.ensure((size_t)chunk)) || (rc = m->grow_cells.ensure((size_t)chunk * max_n)) ||
        (rc = m->grow_stats.ensure(ym::kMgStatSlots)) || (rc = m->kernel_f_dev.ensure(m->kernel_f.size())))
        return rc;
    HIP_TRY(hipMemcpyAsync(m->kernel_f_dev.p, m->kernel_f.data(), m->kernel_f.size() * sizeof(double), hipMemcpyHostToDevice, st));
    // (what the copies of this call read on the host -- `init`, `hs` -- stays as it is until the wait at the end)
    const unsigned long long init[ym::kMgStatSlots] = {0, 0, 0, ~0ull, ~0ull, 0, 0};
    unsigned long long got[ym::kMgStatSlots];
    HIP_TRY(hipMemcpyAsync(m->grow_stats.p, init, sizeof init, hipMemcpyHostToDevice, st));
    std::vector<YmScanRef> all((size_t)n_scans);
    ym::MapGrowArgs a;
    std::memset(&a, 0, sizeof a);
    a.scans = m->grow_scans.p; a.max_n = max_n; a.width = mp->width; a.height = mp->height;
    a.ox = ox; a.oy = oy; a.res = m->cfg.resolution;
    a.cells = m->grow_cells.p; a.stats = m->grow_stats.p; a.kernel = m->kernel_f_dev.p; a.ksize = ks;
    a.cgrid = mp->d_cgrid.p; a.g8 = mp->d_g8.p;
    const dim3 taps((unsigned)(((size_t)max_n * ks * ks + 255) / 256));
    for (int c0 = 0; c0 < n_scans; c0 += chunk) {
        const int B = std::min(chunk, n_scans - c0);
        YmScanRef *hs = all.data() + c0;
        for (int i = 0; i < B; i++) hs[i] = scan_ref(scans[c0 + i]);
        HIP_TRY(hipMemcpyAsync(m->grow_scans.p, hs, sizeof(YmScanRef) * (size_t)B, hipMemcpyHostToDevice, st));
        a.n_scans = B;
        hipLaunchKernelGGL(ym::map_grow_cells_kernel, dim3(B), dim3(1024), 0, st, a);
        hipLaunchKernelGGL(ym::map_grow_smear_kernel<false>, dim3(taps.x, B), dim3(256), 0, st, a);
        hipLaunchKernelGGL(ym::map_grow_smear_kernel<true>, dim3(taps.x, B), dim3(256), 0, st, a);
        HIP_TRY(hipGetLastError());
    }
    HIP_TRY(hipMemcpyAsync(got, m->grow_stats.p, sizeof got, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    s.points = (int64_t)got[ym::kMgPoints]; s.stamped = (int64_t)got[ym::kMgStamped]; s.dropped = (int64_t)got[ym::kMgDropped];
    if (s.stamped > 0) { // the stamped cells' box, widened by the taps' reach and cut to the map
        s.x0 = std::max(0, (int)got[ym::kMgX0] - half); s.y0 = std::max(0, (int)got[ym::kMgY0] - half);
        s.x1 = std::min(mp->width, (int)got[ym::kMgX1] + half + 1); s.y1 = std::min(mp->height, (int)got[ym::kMgY1] + half + 1);
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
    if (!m || !mp || (n_held != 0 && (!held || !held_poses))) return set_err(YM_ERR_INVALID, "null argument");
    if (n_held < 0) return set_err(YM_ERR_INVALID, "n_held must not be negative");
    if (width <= 0 || height <= 0 || (double)width * height > 1.0e9) return set_err(YM_ERR_INVALID, "bad map size %d x %d", width, height);
    if (m->cfg.semantics != YM_SEM_YAGPY) return set_err(YM_ERR_UNSUPPORTED, "ym_map_reframe needs a YM_SEM_YAGPY matcher");
    if (mp->device != m->device) return set_err(YM_ERR_INVALID, "map lives on another device");
    const int64_t nx0 = (int64_t)mp->x0 + dx, ny0 = (int64_t)mp->y0 + dy;
    if (nx0 < -kMapMaxOffset || nx0 > kMapMaxOffset || ny0 < -kMapMaxOffset || ny0 > kMapMaxOffset)
        return set_err(YM_ERR_INVALID, "window offset (%lld, %lld): at most 2^30 cells either way", (long long)nx0, (long long)ny0);
    if (!mp->counted && n_held != 0) return set_err(YM_ERR_INVALID, "this map keeps no counts and holds no scans: n_held must be 0");
    int max_n = 1;
    for (int i = 0; i < n_held; i++) {
        if (!held[i] || held[i]->device != m->device) return set_err(YM_ERR_INVALID, "held scan %d is null or lives on another device", i);
        max_n = std::max(max_n, held[i]->n);
    }
    const int ks = 2 * m->geom.half_kernel + 1, half = m->geom.half_kernel;
    const size_t halo_bytes = (size_t)(ym::kMfTileW + ks - 1) * (size_t)(ym::kMfTileH + ks - 1);
    if (mp->counted) {
        if ((double)max_n * ks * ks > 2.0e9) return set_err(YM_ERR_UNSUPPORTED, "%d beams x %d x %d taps: more than one launch holds", max_n, ks, ks);
        if (halo_bytes > 65536)
            return set_err(YM_ERR_UNSUPPORTED, "%d x %d taps: the recompute's tile and halo (%zu bytes) do not fit 64 KiB of LDS", ks, ks, halo_bytes);
    }
    ym_map_reframe_stats s;
    std::memset(&s, 0, sizeof s);
    s.x0 = mp->x0; s.y0 = mp->y0; s.width = mp->width; s.height = mp->height;
    if (dx == 0 && dy == 0 && width == mp->width && height == mp->height) { // the identity: nothing to do
        s.kept = (int64_t)width * height;
        if (stats) *stats = s;
        return YM_OK;
    }
    // the overlap of the two windows, in cells of the new one (int64: dx, dy are any int)
    const int64_t o0x = std::max<int64_t>(0, -(int64_t)dx), o1x = std::min<int64_t>(width, (int64_t)mp->width - dx);
    const int64_t o0y = std::max<int64_t>(0, -(int64_t)dy), o1y = std::min<int64_t>(height, (int64_t)mp->height - dy);
    const bool overlap = o1x > o0x && o1y > o0y;
    const int ex0 = overlap ? (int)o0x : 0, ex1 = overlap ? (int)o1x : 0, ey0 = overlap ? (int)o0y : 0, ey1 = overlap ? (int)o1y : 0;
    // (without an overlap every source test of the copy must fail: a shift no window reaches, which cannot overflow the kernel's sums)
    const int kdx = overlap ? dx : -kMapMaxOffset * 2 + 1, kdy = overlap ? dy : 0;
    DEV_GUARD(m->device);
    hipStream_t st = m->stream;
    const size_t n = (size_t)width * height;
    // everything is built in arrays of its own and traded in when all of it is complete: whatever fails, the map is as it was
    DevBuf<double> n_cgrid;
    DevBuf<uint8_t> n_g8, n_dirty;
    DevBuf<uint32_t> n_stamps;
    DevBuf<unsigned long long> d_stats;
    int rc;
    if ((rc = n_cgrid.alloc(n)) || (rc = n_g8.alloc(n + 64)) || (rc = d_stats.alloc(2))) return rc;
    if (mp->counted && ((rc = n_stamps.alloc(n)) || (rc = n_dirty.alloc(n)))) return rc;
    HIP_TRY(hipMemsetAsync(d_stats.p, 0, 2 * sizeof(unsigned long long), st));
    HIP_TRY(hipMemsetAsync(n_g8.p + n, 0, 64, st));
    ym::MapReframeArgs r;
    std::memset(&r, 0, sizeof r);
    r.src_cgrid = mp->d_cgrid.p; r.src_g8 = mp->d_g8.p; r.src_stamps = mp->d_stamps.p; r.src_w = mp->width; r.src_h = mp->height;
    r.dx = kdx; r.dy = kdy; r.width = width; r.height = height;
    r.cgrid = n_cgrid.p; r.g8 = n_g8.p; r.stamps = n_stamps.p; r.dirty = n_dirty.p; r.stats = d_stats.p; r.half = half;
    const dim3 groups((unsigned)((n + 1023) / 1024));
    if (mp->counted) hipLaunchKernelGGL(ym::map_reframe_copy_kernel<true>, groups, dim3(256), 0, st, r);
    else hipLaunchKernelGGL(ym::map_reframe_copy_kernel<false>, groups, dim3(256), 0, st, r);
    HIP_TRY(hipGetLastError());
    if (overlap) s.kept = (int64_t)(ex1 - ex0) * (ey1 - ey0);
    unsigned long long got_r[2] = {0, 0};
    if (mp->counted) {
        enum { kAdd = 0, kUpd = ym::kMgStatSlots, kSlots = ym::kMgStatSlots + ym::kMuStatSlots };
        // (what the copies of this call read on the host -- `init`, `all` -- stays as it is until the wait below)
        unsigned long long init[kSlots], got[kSlots];
        std::vector<YmScanRef> all((size_t)n_held);
        if ((rc = m->kernel_f_dev.ensure(m->kernel_f.size()))) return rc;
        HIP_TRY(hipMemcpyAsync(m->kernel_f_dev.p, m->kernel_f.data(), m->kernel_f.size() * sizeof(double), hipMemcpyHostToDevice, st));
        if (n_held > 0) { // the restamp: what the old window dropped and the new one holds
            const int chunk = std::min(n_held, kMapGrowChunk);
            if ((rc = m->grow_scans.ensure((size_t)chunk)) || (rc = m->grow_cells.ensure((size_t)chunk * max_n)) ||
                (rc = m->grow_stats.ensure(kSlots)))
                return rc;
            for (int i = 0; i < kSlots; i++) init[i] = 0;
            init[kAdd + ym::kMgX0] = init[kAdd + ym::kMgY0] = init[kUpd + ym::kMuX0] = init[kUpd + ym::kMuY0] = ~0ull;
            HIP_TRY(hipMemcpyAsync(m->grow_stats.p, init, sizeof init, hipMemcpyHostToDevice, st));
            ym::MapGrowArgs a;
            std::memset(&a, 0, sizeof a);
            a.scans = m->grow_scans.p; a.max_n = max_n; a.width = width; a.height = height;
            a.ox = mp->ox; a.oy = mp->oy; a.res = m->cfg.resolution; a.wx0 = (int)nx0; a.wy0 = (int)ny0;
            a.ex0 = ex0; a.ey0 = ey0; a.ex1 = ex1; a.ey1 = ey1;
            a.cells = m->grow_cells.p; a.stats = m->grow_stats.p + kAdd; a.kernel = m->kernel_f_dev.p; a.ksize = ks;
            a.cgrid = n_cgrid.p; a.g8 = n_g8.p;
            ym::MapForgetArgs f;
            std::memset(&f, 0, sizeof f);
            f.cells = m->grow_cells.p; f.max_n = max_n; f.width = width; f.height = height;
            f.stamps = n_stamps.p; f.stats = m->grow_stats.p + kUpd; f.dirty = n_dirty.p;
            f.kernel = m->kernel_f_dev.p; f.ksize = ks; f.cgrid = n_cgrid.p; f.g8 = n_g8.p;
            const dim3 beams((unsigned)((max_n + 255) / 256)), taps((unsigned)(((size_t)max_n * ks * ks + 255) / 256));
            for (int c0 = 0; c0 < n_held; c0 += chunk) {
                const int B = std::min(chunk, n_held - c0);
                YmScanRef *hs = all.data() + c0;
                for (int i = 0; i < B; i++) hs[i] = scan_ref(held[c0 + i], held_poses + 3 * (size_t)(c0 + i));
                HIP_TRY(hipMemcpyAsync(m->grow_scans.p, hs, sizeof(YmScanRef) * (size_t)B, hipMemcpyHostToDevice, st));
                a.n_scans = B;
                hipLaunchKernelGGL(ym::map_grow_cells_kernel, dim3(B), dim3(1024), 0, st, a);
                hipLaunchKernelGGL(ym::map_count_kernel<false>, dim3(beams.x, B), dim3(256), 0, st, f);
                hipLaunchKernelGGL(ym::map_grow_smear_kernel<false>, dim3(taps.x, B), dim3(256), 0, st, a);
                hipLaunchKernelGGL(ym::map_grow_smear_kernel<true>, dim3(taps.x, B), dim3(256), 0, st, a);
                HIP_TRY(hipGetLastError());
            }
            HIP_TRY(hipMemcpyAsync(got, m->grow_stats.p, sizeof got, hipMemcpyDeviceToHost, st));
        }
        if (overlap) {
            // the recompute, after the restamp's atomics: the cells within the taps' reach of the overlap whose neighbourhood meets
            // the two windows differently are flagged and take their value from the new window's counts
            r.mx0 = std::max(0, ex0 - half); r.mx1 = std::min(width, ex1 + half);
            const int my0 = std::max(0, ey0 - half), my1 = std::min(height, ey1 + half);
            r.my1 = my1;
            for (int y = my0; y < my1; y += 65535) { // (a launch has at most 65535 rows of blocks)
                r.my0 = y;
                hipLaunchKernelGGL(ym::map_reframe_mark_kernel, dim3((unsigned)((r.mx1 - r.mx0 + 255) / 256), (unsigned)std::min(65535, my1 - y)),
                                   dim3(256), 0, st, r);
            }
            ym::MapForgetArgs g;
            std::memset(&g, 0, sizeof g);
            g.width = width; g.height = height; g.stamps = n_stamps.p; g.dirty = n_dirty.p;
            g.kernel = m->kernel_f_dev.p; g.ksize = ks; g.cgrid = n_cgrid.p; g.g8 = n_g8.p;
            g.bx0 = r.mx0 / ym::kMfTileW * ym::kMfTileW; g.by0 = my0 / ym::kMfTileH * ym::kMfTileH; g.bx1 = r.mx1; g.by1 = my1;
            const dim3 tiles((unsigned)((g.bx1 - g.bx0 + ym::kMfTileW - 1) / ym::kMfTileW), (unsigned)((g.by1 - g.by0 + ym::kMfTileH - 1) / ym::kMfTileH));
            for (unsigned ty = 0; ty < tiles.y; ty += 65535u) {
                ym::MapForgetArgs p = g;
                p.by0 = g.by0 + (int)ty * ym::kMfTileH;
                hipLaunchKernelGGL(ym::map_forget_gather_kernel, dim3(tiles.x, std::min(65535u, tiles.y - ty)), dim3(256), halo_bytes, st, p);
            }
            HIP_TRY(hipGetLastError());
        }
        HIP_TRY(hipMemcpyAsync(got_r, d_stats.p, sizeof got_r, hipMemcpyDeviceToHost, st));
        HIP_TRY(hipStreamSynchronize(st));
        int64_t in_overlap = 0;
        if (n_held > 0) {
            s.restamped = (int64_t)got[ym::kMgStamped]; s.dropped = (int64_t)got[ym::kMgDropped];
            in_overlap = (int64_t)got[ym::kMgOverlap];
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
    // scan_matching.py:136-139: the search centre is the mean of the query poses (Python's left-to-right sum), heading 0
    double sx = 0, sy = 0;
    int total = 0, max_n = 1;
    for (int i = 0; i < n_queries; i++) {
        if (!queries[i] || queries[i]->device != m->device) return set_err(YM_ERR_INVALID, "query %d is null or lives on another device", i);
        sx = i == 0 ? queries[i]->pose[0] : sx + queries[i]->pose[0];
        sy = i == 0 ? queries[i]->pose[1] : sy + queries[i]->pose[1];
        total += queries[i]->n;
        max_n = std::max(max_n, queries[i]->n);
    }
    const double ox_real = sx / (double)n_queries, oy_real = sy / (double)n_queries;
    total = std::max(total, 1);
    // the reference's hard-coded coarse pass (scan_matching.py:152-153) unless the caller overrides it
    ym_map_search cs;
    if (coarse) cs = *coarse;
    else { cs.xy_search = 0.25; cs.xy_step = 0.01; cs.angle_search = 0.1; cs.angle_step = 0.01; cs.grid_resolution = 0.05; cs.penalize = 0; cs.reserved = 0; }
    if (!(cs.xy_step > 0) || !(cs.angle_step > 0) || !(cs.grid_resolution > 0) || !(cs.xy_search > 0) || !(cs.angle_search > 0))
        return set_err(YM_ERR_INVALID, "bad coarse search parameters");
    const double res = m->cfg.resolution;
    const int maxd = std::max({8, (int)std::ceil(2 * cs.xy_search / cs.xy_step) + 2, (int)std::ceil(4 * res / res) + 2});
    const int maxt = std::max({13, (int)std::ceil(2 * cs.angle_search / cs.angle_step) + 2});
    if (maxd > YM_YAG_MAX_DIM || maxt > YM_YAG_MAX_NT)
        return set_err(YM_ERR_UNSUPPORTED, "map search lattice %d x %d x %d exceeds the built-in limit", maxd, maxd, maxt);
    const size_t vol = (size_t)maxt * maxd * maxd;
    int rc;
    Slot &slot = m->slots[kAsyncSlots];
    if (slot.in_flight) return set_err(YM_ERR_BUSY, "the synchronous slot is in flight");
    if ((rc = m->states.ensure(1))) return rc;
    if ((rc = m->map_pts.ensure((size_t)total))) return rc;
    if ((rc = m->yaxes.ensure((size_t)3 * YM_YAG_MAX_DIM))) return rc;
    if ((rc = m->yrot.ensure((size_t)maxt * total))) return rc;
    if ((rc = m->sums.ensure(2 * vol))) return rc;
    if ((rc = m->resp.ensure(vol))) return rc;
    const size_t scans_bytes = align_up(sizeof(YmScanRef) * n_queries, 16);
    if ((rc = slot.desc.ensure(scans_bytes + sizeof(YmItemState)))) return rc;
    if ((rc = slot.result.ensure(sizeof(YmItemState)))) return rc;
    if ((rc = m->desc_dev.ensure(scans_bytes))) return rc;
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
        a.states = m->states.p; a.host_out = reinterpret_cast<YmItemState *>(slot.result.dp);
        a.axes = m->yaxes.p; a.rot = m->yrot.p;
        a.sums = m->sums.p + m->sums_pass_offset[pass]; a.out = m->resp.p;
        a.grid = mp->d_g8.p; a.grid_stride = 0; a.vol_stride = vol;
        a.max_n = total; a.maxd = maxd; a.maxt = maxt;
        a.map_w = mp->width; a.map_h = mp->height; a.map_ox = ox; a.map_oy = oy;
        hipLaunchKernelGGL(ym::yag_setup_kernel, dim3(maxt, 1), dim3(256), 0, st, a);
        hipLaunchKernelGGL(ym::yag_score_kernel, dim3((maxd * maxd + 255) / 256, maxt, 1), dim3(256), 0, st, a);
        hipLaunchKernelGGL(ym::yag_reduce_kernel<1024>, dim3(1), dim3(1024), 0, st, a);
    }
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipStreamSynchronize(st));
    const YmItemState &r = *reinterpret_cast<const YmItemState *>(slot.result.p);
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
    m->last_valid = false; // the debug getters describe match_scan calls
    m->sets_last.valid = false;
    m->map_last.valid = true; m->map_last.n_items = 1; m->map_last.first_kept = 0; m->map_last.passes = refine ? 2 : 1; // (ym_debug_map_sums)
    m->map_last.vol = vol; m->map_last.pass_offset[0] = 0; m->map_last.pass_offset[1] = vol;
    return YM_OK;
}

// ---- the component area filter (ym_k_despeckle.hpp)
static const ym_despeckle_opts kNodeDespeckle = {0, 255, 5, 8}; // ros1/slam_node_ros1:191-197

static int despeckle_check_opts(const ym_despeckle_opts &o) {
    if (o.foreground < 0 || o.foreground > 255) return set_err(YM_ERR_INVALID, "foreground %d: 0 .. 255", o.foreground);
    if (o.fill < 0 || o.fill > 255) return set_err(YM_ERR_INVALID, "fill %d: 0 .. 255", o.fill);
    if (o.min_area < 0) return set_err(YM_ERR_INVALID, "min_area %d: 0 or more", o.min_area);
    if (o.connectivity != 4 && o.connectivity != 8) return set_err(YM_ERR_INVALID, "connectivity %d: 4 or 8", o.connectivity);
    return YM_OK;
}

// d_image -> d_out (both dense [height][width] on the current device; they may be the same), the statistics to *stats.
// Four launches on `stream` and one wait; the working memory is freed when the call ends, whatever its outcome.
static int despeckle_run(const uint8_t *d_image, uint8_t *d_out, int width, int height, const ym_despeckle_opts &o, hipStream_t stream,
                         ym_despeckle_stats *stats) {
    const size_t n = (size_t)width * height;
    DevBuf<unsigned> parent, size;
    DevBuf<unsigned long long> d_stats;
    int rc;
    if ((rc = parent.alloc(n)) || (rc = size.alloc(n)) || (rc = d_stats.alloc(ym::kDspStatSlots))) return rc;
    HIP_TRY(hipMemsetAsync(d_stats.p, 0, ym::kDspStatSlots * sizeof(unsigned long long), stream));
    ym::DespeckleArgs a{};
    a.image = d_image; a.out = d_out; a.width = width; a.height = height; a.nbx = (width + 63) / 64;
    a.foreground = o.foreground; a.fill = o.fill; a.min_area = (unsigned)o.min_area;
    a.parent = parent.p; a.size = size.p; a.stats = d_stats.p;
    const dim3 grid((unsigned)((size_t)a.nbx * (size_t)((height + 15) / 16))); // (below 2^31: width * height is)
    hipLaunchKernelGGL(ym::dsp_init_kernel, grid, dim3(256), 0, stream, a);
    if (o.connectivity == 8) hipLaunchKernelGGL(ym::dsp_merge_kernel<8>, grid, dim3(256), 0, stream, a);
    else hipLaunchKernelGGL(ym::dsp_merge_kernel<4>, grid, dim3(256), 0, stream, a);
    hipLaunchKernelGGL(ym::dsp_sizes_kernel, grid, dim3(256), 0, stream, a);
    hipLaunchKernelGGL(ym::dsp_apply_kernel, grid, dim3(256), 0, stream, a);
    HIP_TRY(hipGetLastError());
    unsigned long long got[ym::kDspStatSlots];
    HIP_TRY(hipMemcpyAsync(got, d_stats.p, sizeof got, hipMemcpyDeviceToHost, stream));
    HIP_TRY(hipStreamSynchronize(stream));
    if (got[ym::kDspErr]) return set_err(YM_ERR_HIP, "the component pass reached its retry cap (a fault of the library)");
    if (stats) {
        ym_despeckle_stats s{};
        s.foreground_cells = (int64_t)got[ym::kDspFg]; s.background_cells = (int64_t)got[ym::kDspBg];
        s.components = (int64_t)got[ym::kDspComponents]; s.removed_components = (int64_t)got[ym::kDspRemoved];
        s.cleared_cells = (int64_t)got[ym::kDspCleared];
        s.background_filled = s.background_cells > 0 && s.background_cells < (int64_t)o.min_area ? 1 : 0;
        *stats = s;
    }
    return YM_OK;
}

int ym_image_despeckle(int device, const uint8_t *image, int width, int height, int pitch, const ym_despeckle_opts *opts, uint8_t *out,
                       ym_despeckle_stats *stats) {
    const ym_despeckle_opts o = opts ? *opts : kNodeDespeckle;
    int rc;
    if ((rc = despeckle_check_opts(o))) return rc;
    if (!image || !out) return set_err(YM_ERR_INVALID, "image or out: null");
    if (width < 1 || height < 1) return set_err(YM_ERR_INVALID, "image of %d x %d cells", width, height);
    if (pitch < width) return set_err(YM_ERR_INVALID, "pitch %d: at least width (%d bytes)", pitch, width);
    if ((int64_t)width * height > (int64_t)INT32_MAX)
        return set_err(YM_ERR_UNSUPPORTED, "image of %d x %d cells: at most 2^31 - 1", width, height);
    if ((rc = check_device(device))) return rc;
    DEV_GUARD(device);
    const size_t n = (size_t)width * height;
    DevBuf<uint8_t> d_img;
    if ((rc = d_img.alloc(n))) return rc;
    HIP_TRY(hipMemcpy2D(d_img.p, (size_t)width, image, (size_t)pitch, (size_t)width, (size_t)height, hipMemcpyHostToDevice));
    ym_despeckle_stats s{};
    if ((rc = despeckle_run(d_img.p, d_img.p, width, height, o, nullptr, &s))) return rc;
    // (the outputs are written only once the whole call has succeeded: `out` by the one copy that can still fail)
    HIP_TRY(hipMemcpy(out, d_img.p, n, hipMemcpyDeviceToHost));
    if (stats) *stats = s;
    return YM_OK;
}

// ---- occupancy-grid rendering (karto_scanmatcher.create_occupancy_grid)
// Shared with the live occupancy grid (ym_abi_occlive.hpp); both run on the null stream.
// The bounding boxes (LocalizedRangeScan::Update) of a device scan table, joined into box[4] = xmin, ymin, xmax, ymax, which the
// caller initialises: the box OccupancyGrid::ComputeDimensions sizes the grid by.  d_boxes: the caller's device memory for
// [n_scans][4] doubles, allocated with the caller's other buffers and freed with them.  (Measured: allocated and freed in here, so
// before the counts are allocated, a trace of 500 to 2000 scans ran 13 % faster to 7 % slower through unchanged kernels and an add
// of five scans 12 us slower -- profiles/map_side_fold_time.json; where the counts lie decides the rate of their atomics.)
static int occ_join_boxes(const YmScanRef *d_scans, int n_scans, int max_n, double range_threshold, double *d_boxes, double box[4]) {
    ym::OccArgs a;
    std::memset(&a, 0, sizeof a);
    a.scans = d_scans; a.n_scans = n_scans; a.max_n = max_n; a.range_threshold = range_threshold; a.boxes = d_boxes;
    hipLaunchKernelGGL(ym::occ_bbox_kernel, dim3(n_scans), dim3(256), 0, nullptr, a);
    HIP_TRY(hipGetLastError());
    std::vector<double> boxes((size_t)4 * n_scans);
    HIP_TRY(hipMemcpy(boxes.data(), d_boxes, sizeof(double) * boxes.size(), hipMemcpyDeviceToHost));
    for (int i = 0; i < n_scans; i++) {
        box[0] = std::min(box[0], boxes[4 * i]); box[1] = std::min(box[1], boxes[4 * i + 1]);
        box[2] = std::max(box[2], boxes[4 * i + 2]); box[3] = std::max(box[3], boxes[4 * i + 3]);
    }
    return YM_OK;
}

// The rays of a device scan table into the counts `a` describes (everything but a.scans and a.n_scans is the caller's).
// form 1: a thread per ray; 0: a wave per ray, which needs range_threshold * scale < 2^24 (ym_occmap_create checks it)
static int occ_trace(ym::OccArgs a, const YmScanRef *d_scans, int n_scans, int form) {
    for (int first = 0; first < n_scans; first += 32768) { // (a launch has at most 65535 rows of blocks)
        const int count = std::min(n_scans - first, 32768);
        a.scans = d_scans + first; a.n_scans = count;
        if (form == 1) hipLaunchKernelGGL(ym::occ_trace_thread_kernel, dim3((a.max_n + 255) / 256, count), dim3(256), 0, nullptr, a);
        else hipLaunchKernelGGL(ym::occ_trace_wave_kernel, dim3((a.max_n + 3) / 4, count), dim3(256), 0, nullptr, a);
        HIP_TRY(hipGetLastError());
    }
    return YM_OK;
}

// keep_counts (ym_occupancy_create_counted, a test hook): the pass and hit counts are copied to the host before they are freed
// clean (ym_occupancy_create_clean): the image goes through the component area filter on the device before its copy to the host
static ym_occupancy *occupancy_render(const ym_scan *const *scans, int n_scans, double resolution, double range_threshold, bool keep_counts,
                                      const ym_despeckle_opts *clean = nullptr) {
    if (!scans || n_scans <= 0) { set_err(YM_ERR_INVALID, "no scans"); return nullptr; }
    if (!(resolution > 0) || !(range_threshold > 0)) { set_err(YM_ERR_INVALID, "resolution and range_threshold must be > 0"); return nullptr; }
    const int device = scans[0] ? scans[0]->device : -1;
    int max_n = 1;
    for (int i = 0; i < n_scans; i++) {
        if (!scans[i] || scans[i]->device != device) { set_err(YM_ERR_INVALID, "scan %d is null or lives on another device", i); return nullptr; }
        max_n = std::max(max_n, scans[i]->n);
    }
    DevGuard guard(device);
    if (guard.status() != YM_OK) return nullptr;
    std::vector<YmScanRef> hs(n_scans);
    for (int i = 0; i < n_scans; i++) hs[i] = scan_ref(scans[i], nullptr, true);
    DevBuf<YmScanRef> d_scans;
    DevBuf<double> d_boxes;
    DevBuf<unsigned> d_cnt;
    DevBuf<uint8_t> d_img;
    ym_occupancy *og = new ym_occupancy();
    og->device = device;
    auto render = [&]() -> int {
        int rc;
        if ((rc = d_scans.alloc(n_scans)) || (rc = d_boxes.alloc((size_t)4 * n_scans))) return rc;
        HIP_TRY(hipMemcpy(d_scans.p, hs.data(), sizeof(YmScanRef) * n_scans, hipMemcpyHostToDevice));
        // OccupancyGrid::ComputeDimensions: the scans' bounding boxes joined, width = Round(size * scale)
        double box[4] = {1e300, 1e300, -1e300, -1e300};
        if ((rc = occ_join_boxes(d_scans.p, n_scans, max_n, range_threshold, d_boxes.p, box))) return rc;
        const double scale = 1.0 / resolution;
        const int width = (int)kt_round_h((box[2] - box[0]) * scale), height = (int)kt_round_h((box[3] - box[1]) * scale);
        if (width <= 0 || height <= 0 || (double)width * height > 2.0e9)
            return set_err(YM_ERR_UNSUPPORTED, "occupancy grid of %d x %d cells", width, height);
        const size_t n = (size_t)width * height;
        if ((rc = d_cnt.alloc(2 * n)) || (rc = d_img.alloc(n))) return rc;
        HIP_TRY(hipMemset(d_cnt.p, 0, 2 * n * sizeof(unsigned)));
        // the live grid's kernels with the lattice anchored at the box's minimum, the memory at the lattice's origin and as wide as
        // the grid, every ray added, and all of it read
        ym::OccArgs a;
        std::memset(&a, 0, sizeof a);
        a.max_n = max_n; a.range_threshold = range_threshold; a.scale = scale; a.anchor_x = box[0]; a.anchor_y = box[1];
        a.width = a.win_w = width; a.height = a.win_h = height; a.pitch = width; a.sign = 1u;
        a.pass = d_cnt.p; a.hits = d_cnt.p + n; a.image = d_img.p;
        if ((rc = occ_trace(a, d_scans.p, n_scans, 1))) return rc; // (a launch over many scans: a thread per ray)
        hipLaunchKernelGGL(ym::occ_update_kernel, dim3((unsigned)((width + 255) / 256), (unsigned)std::min(height, 65535)), dim3(256), 0, nullptr, a);
        HIP_TRY(hipGetLastError());
        og->info.width = width; og->info.height = height;
        og->info.offset_x = box[0]; og->info.offset_y = box[1]; og->info.resolution = resolution;
        if (clean) {
            if (n > (size_t)INT32_MAX) return set_err(YM_ERR_UNSUPPORTED, "occupancy grid of %d x %d cells: the filter takes at most 2^31 - 1", width, height);
            if ((rc = despeckle_run(d_img.p, d_img.p, width, height, *clean, nullptr, &og->clean_stats))) return rc;
            og->cleaned = true;
        }
        og->image.resize(n);
        HIP_TRY(hipMemcpy(og->image.data(), d_img.p, n, hipMemcpyDeviceToHost));
        if (keep_counts) {
            og->counts.resize(2 * n);
            HIP_TRY(hipMemcpy(og->counts.data(), d_cnt.p, 2 * n * sizeof(unsigned), hipMemcpyDeviceToHost));
        }
        return YM_OK;
    };
    if (render() != YM_OK) { delete og; return nullptr; } // (the error text is set)
    return og;
}

ym_occupancy *ym_occupancy_create(const ym_scan *const *scans, int n_scans, double resolution, double range_threshold) {
    return occupancy_render(scans, n_scans, resolution, range_threshold, false);
}

ym_occupancy *ym_occupancy_create_counted(const ym_scan *const *scans, int n_scans, double resolution, double range_threshold) {
    return occupancy_render(scans, n_scans, resolution, range_threshold, true);
}

ym_occupancy *ym_occupancy_create_clean(const ym_scan *const *scans, int n_scans, double resolution, double range_threshold,
                                        const ym_despeckle_opts *opts) {
    const ym_despeckle_opts o = opts ? *opts : kNodeDespeckle;
    if (despeckle_check_opts(o) != YM_OK) return nullptr; // (the error text is set)
    return occupancy_render(scans, n_scans, resolution, range_threshold, false, &o);
}

int ym_occupancy_get_despeckle_stats(const ym_occupancy *og, ym_despeckle_stats *stats) {
    if (!og || !stats) return set_err(YM_ERR_INVALID, "null argument");
    if (!og->cleaned) return set_err(YM_ERR_INVALID, "this grid was made without the filter: use ym_occupancy_create_clean");
    *stats = og->clean_stats;
    return YM_OK;
}

int ym_occupancy_get_info(const ym_occupancy *og, ym_occupancy_info *info) {
    if (!og || !info) return set_err(YM_ERR_INVALID, "null argument");
    *info = og->info;
    return YM_OK;
}

int ym_occupancy_read(const ym_occupancy *og, uint8_t *image, int64_t image_bytes) {
    if (!og || !image) return set_err(YM_ERR_INVALID, "null argument");
    if ((size_t)image_bytes < og->image.size()) return set_err(YM_ERR_INVALID, "buffer too small: need %zu bytes", og->image.size());
    std::memcpy(image, og->image.data(), og->image.size());
    return YM_OK;
}

int ym_occupancy_read_counts(const ym_occupancy *og, uint32_t *pass, uint32_t *hits, int64_t cells) {
    if (!og || !pass || !hits) return set_err(YM_ERR_INVALID, "null argument");
    const size_t n = og->image.size();
    if (og->counts.size() != 2 * n) return set_err(YM_ERR_INVALID, "this grid was made without counts: use ym_occupancy_create_counted");
    if (cells < 0 || (size_t)cells < n) return set_err(YM_ERR_INVALID, "buffers too small: need %zu cells each", n);
    std::memcpy(pass, og->counts.data(), n * sizeof(uint32_t));
    std::memcpy(hits, og->counts.data() + n, n * sizeof(uint32_t));
    return YM_OK;
}

void ym_occupancy_destroy(ym_occupancy *og) { delete og; }
