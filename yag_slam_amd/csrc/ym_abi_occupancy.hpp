// ym_abi_occupancy.hpp -- C ABI: the component area filter (ym_image_despeckle) and occupancy-grid rendering (ym_occupancy_*)
// Part of yagmatch.hip (included inside its extern "C" block); not a header of its own.
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
