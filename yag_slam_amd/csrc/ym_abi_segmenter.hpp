// ym_abi_segmenter.hpp -- C ABI: a prior map's image to its label image, resident as a ym_segments (ym_map_free_space,
// ym_segments_from_map, ym_segments_labels; ym_k_segmenter.hpp).  The host's part: the scalars of DESIGN.md "Map segmenter"
// (n_segments, step, min_size), the launch sequence and the Lloyd loop with its cap.
// Part of yagmatch.hip (included inside its extern "C" block, after ym_abi_segments.hpp); not a header of its own.
constexpr int64_t kSegSumPerSegment = 600000; // the reference's rule: n_segments = sum(closed) // 600000 * density

// the buffers of one segmentation: freed when the call ends, whatever its outcome
struct SegmenterWork {
    DevBuf<uint8_t> src, closed;
    DevBuf<unsigned long long> sums, cell_acc, acc;
    DevBuf<unsigned> err, block_counts, parent, size;
    DevBuf<int32_t> cell_centre, assign;
    DevBuf<double2> centres[2];
};

static int segmenter_check_image(const uint8_t *image, int w, int h, int pitch, int close_size) {
    if (!image) return set_err(YM_ERR_INVALID, "image: null");
    if (w < 1 || w > 65536) return set_err(YM_ERR_INVALID, "w %d: 1 .. 65536", w);
    if (h < 1 || h > 65536) return set_err(YM_ERR_INVALID, "h %d: 1 .. 65536", h);
    if (pitch < w) return set_err(YM_ERR_INVALID, "pitch %d: at least w (%d bytes)", pitch, w);
    if (close_size < 1 || close_size > 2 * ym::kCloseMaxR + 1 || close_size % 2 == 0)
        return set_err(YM_ERR_INVALID, "close_size %d: odd, 1 .. %d", close_size, 2 * ym::kCloseMaxR + 1);
    return YM_OK;
}

// A: upload, threshold and closing; sums[0 .. 1] = the sum of `closed` and its non-zero pixels (the call waits for them)
static int segmenter_close(SegmenterWork &wk, ym::SegmenterArgs &a, hipStream_t stream, const uint8_t *image, int pitch, int close_size,
                           unsigned long long *sums) {
    const size_t n = (size_t)a.width * a.height;
    int rc;
    if ((rc = wk.src.ensure(n)) || (rc = wk.closed.ensure(n)) || (rc = wk.sums.ensure(4)) || (rc = wk.err.ensure(ym::kSegErrSlots))) return rc;
    HIP_TRY(hipMemcpy2D(wk.src.p, (size_t)a.width, image, (size_t)pitch, (size_t)a.width, (size_t)a.height, hipMemcpyHostToDevice));
    HIP_TRY(hipMemsetAsync(wk.sums.p, 0, 4 * sizeof(unsigned long long), stream));
    HIP_TRY(hipMemsetAsync(wk.err.p, 0, ym::kSegErrSlots * sizeof(unsigned), stream));
    a.src = wk.src.p; a.closed = wk.closed.p; a.sums = wk.sums.p; a.err = wk.err.p;
    a.radius = close_size / 2;
    const dim3 grid((unsigned)((a.width + ym::kCloseTile - 1) / ym::kCloseTile), (unsigned)((a.height + ym::kCloseTile - 1) / ym::kCloseTile));
    hipLaunchKernelGGL(ym::seg_close_kernel, grid, dim3(256), 0, stream, a);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpyAsync(sums, wk.sums.p, 2 * sizeof(unsigned long long), hipMemcpyDeviceToHost, stream));
    HIP_TRY(hipStreamSynchronize(stream));
    return YM_OK;
}

int ym_map_free_space(int device, const uint8_t *image, int w, int h, int pitch, int close_size, uint8_t *closed, int64_t *sum,
                      int64_t *n_free) {
    int rc;
    if ((rc = segmenter_check_image(image, w, h, pitch, close_size))) return rc;
    if (!closed || !sum || !n_free) return set_err(YM_ERR_INVALID, "closed, sum or n_free: null");
    if ((rc = check_device(device))) return rc;
    DEV_GUARD(device);
    SegmenterWork wk;
    ym::SegmenterArgs a{};
    a.width = w; a.height = h;
    unsigned long long sums[2];
    if ((rc = segmenter_close(wk, a, nullptr, image, pitch, close_size, sums))) return rc;
    // (the outputs are written only once the whole call has succeeded: `closed` last, by the one copy that can still fail)
    HIP_TRY(hipMemcpy(closed, wk.closed.p, (size_t)w * h, hipMemcpyDeviceToHost));
    *sum = (int64_t)sums[0];
    *n_free = (int64_t)sums[1];
    return YM_OK;
}

// the three launches of the raster-order prefix sum; *total = the flagged items
extern "C++" {
template <int kWhat>
static int segmenter_number(SegmenterWork &wk, ym::SegmenterArgs &a, hipStream_t stream, long long n_items, unsigned *total) {
    const unsigned n_blocks = (unsigned)((n_items + ym::kSegScanChunk - 1) / ym::kSegScanChunk);
    int rc;
    if ((rc = wk.block_counts.ensure(n_blocks))) return rc;
    a.n_items = n_items; a.n_blocks = n_blocks; a.block_counts = wk.block_counts.p;
    hipLaunchKernelGGL(ym::seg_flag_count_kernel<kWhat>, dim3(n_blocks), dim3(256), 0, stream, a);
    hipLaunchKernelGGL(ym::seg_scan_kernel, dim3(1), dim3(1024), 0, stream, a);
    hipLaunchKernelGGL(ym::seg_rank_kernel<kWhat>, dim3(n_blocks), dim3(256), 0, stream, a);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpyAsync(total, wk.err.p + ym::kSegTotal, sizeof(unsigned), hipMemcpyDeviceToHost, stream));
    HIP_TRY(hipStreamSynchronize(stream));
    return YM_OK;
}
}  // extern "C++"

static int segmenter_run(ym_segments *sg, const uint8_t *image, int pitch, const ym_segment_opts &o, ym_segment_info *info) {
    const int w = sg->width, h = sg->height;
    const size_t n_pix = (size_t)w * h, n_img = (size_t)sg->pitch * h;
    hipStream_t stream = sg->stream;
    SegmenterWork wk;
    ym::SegmenterArgs a{};
    a.width = w; a.height = h; a.pitch = sg->pitch;
    int rc;
    unsigned long long sums[3] = {0, 0, 0};
    if ((rc = segmenter_close(wk, a, stream, image, pitch, o.close_size, sums))) return rc;
    const int64_t sum = (int64_t)sums[0], n_free = (int64_t)sums[1];
    // A.7 - A.9
    int64_t n_segments = o.n_segments;
    if (n_segments == 0) {
        const double v = (double)(sum / kSegSumPerSegment) * o.density; // (int(S // 600000 * density): the reference's precedence)
        if (v >= 2147483648.0) return set_err(YM_ERR_INVALID, "n_segments: sum %lld // 600000 * density %g is beyond int32", (long long)sum, o.density);
        n_segments = (int64_t)v;
    }
    if (n_segments < 1)
        return set_err(YM_ERR_INVALID, "n_segments %lld (sum of the closed image %lld // 600000 * density %g): at least 1", (long long)n_segments,
                       (long long)sum, o.density);
    if (n_free == 0) return set_err(YM_ERR_INVALID, "image: no free pixel (>= 254) is left after the closing");
    // B.1 - B.2
    const int step = std::max(1, (int)(std::sqrt((double)n_free / (double)n_segments) + 0.5));
    const int gw = (w + step - 1) / step, gh = (h + step - 1) / step, parts = (step + ym::kSegPart - 1) / ym::kSegPart;
    const int64_t cells = (int64_t)gw * gh, cell_blocks = cells * parts * parts;
    if (cell_blocks > INT32_MAX)
        return set_err(YM_ERR_UNSUPPORTED, "n_segments %lld: cells of %d pixels make %lld blocks on this image (at most 2^31 - 1)",
                       (long long)n_segments, step, (long long)cell_blocks);
    a.step = step; a.gw = gw; a.gh = gh; a.parts = parts; a.nbx = gw * parts;
    if ((rc = wk.cell_acc.ensure(3 * (size_t)cells)) || (rc = wk.cell_centre.ensure((size_t)cells)) || (rc = wk.assign.ensure(n_img))) return rc;
    // (the seeds' first centres are written before their count is known: room for every cell, bounded by the free pixels)
    const size_t max_centres = (size_t)std::min<int64_t>(cells, n_free);
    if ((rc = wk.centres[0].ensure(max_centres)) || (rc = wk.centres[1].ensure(max_centres))) return rc;
    HIP_TRY(hipMemsetAsync(wk.cell_acc.p, 0, 3 * (size_t)cells * sizeof(unsigned long long), stream));
    a.cell_acc = wk.cell_acc.p; a.cell_centre = wk.cell_centre.p;
    hipLaunchKernelGGL(ym::seg_cell_sums_kernel, dim3((unsigned)cell_blocks), dim3(256), 0, stream, a);
    a.centres_next = wk.centres[0].p;
    unsigned seeds = 0;
    if ((rc = segmenter_number<ym::kSeeds>(wk, a, stream, cells, &seeds))) return rc;
    if (seeds == 0) return set_err(YM_ERR_INVALID, "n_segments %lld: no cell of %d x %d pixels is a quarter free", (long long)n_segments, step, step);
    // C: Lloyd passes; the centres alternate between the two buffers
    a.n_centres = (int)seeds;
    if ((rc = wk.acc.ensure(3 * (size_t)seeds))) return rc;
    a.acc = wk.acc.p; a.assign = wk.assign.p;
    HIP_TRY(hipMemsetAsync(wk.assign.p, 0, n_img * sizeof(int32_t), stream));
    int cur = 0, runs = 0;
    for (int it = 0; it < o.iterations; it++) { // (the cap of the loop: the caller's iterations)
        HIP_TRY(hipMemsetAsync(wk.acc.p, 0, 3 * (size_t)seeds * sizeof(unsigned long long), stream));
        HIP_TRY(hipMemsetAsync(wk.err.p + ym::kSegChanged, 0, sizeof(unsigned), stream));
        a.centres = wk.centres[cur].p; a.centres_next = wk.centres[cur ^ 1].p;
        hipLaunchKernelGGL(ym::seg_assign_kernel, dim3((unsigned)cell_blocks), dim3(256), 0, stream, a);
        hipLaunchKernelGGL(ym::seg_centres_kernel, dim3((seeds + 255) / 256), dim3(256), 0, stream, a);
        HIP_TRY(hipGetLastError());
        unsigned changed = 0;
        HIP_TRY(hipMemcpyAsync(&changed, wk.err.p + ym::kSegChanged, sizeof(unsigned), hipMemcpyDeviceToHost, stream));
        HIP_TRY(hipStreamSynchronize(stream));
        cur ^= 1;
        runs++;
        if (!changed) break; // (no pixel changed its centre: every further pass would repeat this one)
    }
    const int64_t min_size = (n_free / n_segments) / o.min_size_div;
    unsigned segments = 0;
    int64_t labelled = 0;
    if (o.stage == YM_SEGMENT_STAGE_ASSIGNED) {
        HIP_TRY(hipMemcpyAsync(sg->d_img.p, wk.assign.p, n_img * sizeof(int32_t), hipMemcpyDeviceToDevice, stream));
    } else {
        // D: components, sizes, numbers
        if ((rc = wk.parent.ensure(n_pix)) || (rc = wk.size.ensure(n_pix))) return rc;
        HIP_TRY(hipMemsetAsync(wk.size.p, 0, n_pix * sizeof(unsigned), stream));
        a.parent = wk.parent.p; a.size = wk.size.p; a.min_size = (unsigned long long)min_size; a.labels = sg->d_img.p;
        const dim3 grid((unsigned)((w + 63) / 64), (unsigned)((h + 15) / 16));
        hipLaunchKernelGGL(ym::seg_cc_init_kernel, grid, dim3(256), 0, stream, a);
        hipLaunchKernelGGL(ym::seg_cc_merge_kernel, grid, dim3(256), 0, stream, a);
        hipLaunchKernelGGL(ym::seg_cc_sizes_kernel, grid, dim3(256), 0, stream, a);
        if ((rc = segmenter_number<ym::kRoots>(wk, a, stream, (long long)n_pix, &segments))) return rc;
        hipLaunchKernelGGL(ym::seg_relabel_kernel, grid, dim3(256), 0, stream, a);
        HIP_TRY(hipGetLastError());
        unsigned err = 0;
        HIP_TRY(hipMemcpyAsync(&err, wk.err.p + ym::kSegErrLoop, sizeof(unsigned), hipMemcpyDeviceToHost, stream));
        HIP_TRY(hipMemcpyAsync(&sums[2], wk.sums.p + 2, sizeof(unsigned long long), hipMemcpyDeviceToHost, stream));
        HIP_TRY(hipStreamSynchronize(stream));
        if (err) return set_err(YM_ERR_HIP, "the component pass reached its retry cap (a fault of the library)");
        if (segments > (unsigned)INT32_MAX) return set_err(YM_ERR_UNSUPPORTED, "%u segments: beyond int32 labels", segments);
        labelled = (int64_t)sums[2];
    }
    if (o.stage == YM_SEGMENT_STAGE_ASSIGNED) {
        // the label range, as ym_segments_create finds it
        const int32_t init[2] = {INT32_MAX, INT32_MIN};
        HIP_TRY(hipMemcpy(sg->range.p, init, sizeof init, hipMemcpyHostToDevice));
        ym::SegArgs ra = segments_args(sg);
        ra.range = sg->range.p;
        const size_t n_vec = (size_t)((w + 3) / 4) * h;
        hipLaunchKernelGGL(ym::segment_range_kernel, dim3((unsigned)std::min<size_t>((n_vec + 255) / 256, ym::kSegRangeBlocks)), dim3(256), 0, stream, ra);
        HIP_TRY(hipGetLastError());
        int32_t got[2];
        HIP_TRY(hipMemcpyAsync(got, sg->range.p, sizeof got, hipMemcpyDeviceToHost, stream));
        HIP_TRY(hipStreamSynchronize(stream));
        sg->min_label = got[0]; sg->max_label = got[1];
    } else {
        // the label range needs no pass: the labels are 1 .. K, and 0 wherever a pixel is not labelled
        sg->min_label = segments > 0 && labelled == (int64_t)n_pix ? 1 : 0;
        sg->max_label = (int32_t)segments;
    }
    if (info) {
        ym_segment_info out{};
        out.sum = sum; out.n_free = n_free;
        out.n_segments = (int32_t)n_segments; out.step = step; out.seeds = (int32_t)seeds; out.segments = (int32_t)segments;
        out.iterations_run = runs; out.min_size = (int32_t)std::min<int64_t>(min_size, INT32_MAX);
        out.unlabelled = o.stage == YM_SEGMENT_STAGE_ASSIGNED ? -1 : n_free - labelled;
        *info = out;
    }
    return YM_OK;
}

ym_segments *ym_segments_from_map(int device, const uint8_t *image, int w, int h, int pitch, const ym_segment_opts *opts, ym_segment_info *info) {
    ym_segment_opts o;
    if (opts) o = *opts;
    else { o.n_segments = 0; o.density = 1.0; o.close_size = 11; o.iterations = 10; o.min_size_div = 4; o.stage = YM_SEGMENT_STAGE_FINAL; }
    if (segmenter_check_image(image, w, h, pitch, o.close_size) != YM_OK) return nullptr;
    if (o.n_segments < 0) { set_err(YM_ERR_INVALID, "n_segments %d: 0 (the 600000 rule) or more", o.n_segments); return nullptr; }
    if (!(o.density > 0.0) || !std::isfinite(o.density)) { set_err(YM_ERR_INVALID, "density %g: positive and finite", o.density); return nullptr; }
    if (o.iterations < 1) { set_err(YM_ERR_INVALID, "iterations %d: at least 1", o.iterations); return nullptr; }
    if (o.min_size_div < 1) { set_err(YM_ERR_INVALID, "min_size_div %d: at least 1", o.min_size_div); return nullptr; }
    if (o.stage != YM_SEGMENT_STAGE_FINAL && o.stage != YM_SEGMENT_STAGE_ASSIGNED) { set_err(YM_ERR_INVALID, "stage %d: 0 or 1", o.stage); return nullptr; }
    if (check_device(device) != YM_OK) return nullptr;
    DevGuard guard(device);
    if (guard.status() != YM_OK) return nullptr;
    ym_segments *sg = new ym_segments();
    sg->device = device; sg->width = w; sg->height = h; sg->pitch = (w + 3) / 4 * 4;
    auto setup = [&]() -> int {
        int rc;
        if ((rc = sg->stream.create()) || (rc = sg->d_img.alloc((size_t)sg->pitch * h)) || (rc = sg->range.ensure(2)) || (rc = sg->flags.ensure(4))) return rc;
        return segmenter_run(sg, image, pitch, o, info);
    };
    if (setup() != YM_OK) { // (the error text is set)
        if (sg->stream) (void)hipStreamSynchronize(sg->stream);
        delete sg;
        return nullptr;
    }
    return sg;
}

int ym_segments_labels(ym_segments *sg, int32_t *labels, int64_t n) {
    if (!sg) return set_err(YM_ERR_INVALID, "null segments");
    const size_t need = (size_t)sg->width * sg->height;
    if (!labels || n < 0 || (uint64_t)n < need) return set_err(YM_ERR_INVALID, "labels: room for %zu labels needed", need);
    DEV_GUARD(sg->device);
    HIP_TRY(hipStreamSynchronize(sg->stream));
    HIP_TRY(hipMemcpy2D(labels, sizeof(int32_t) * sg->width, sg->d_img.p, sizeof(int32_t) * sg->pitch, sizeof(int32_t) * sg->width, sg->height,
                        hipMemcpyDeviceToHost));
    return YM_OK;
}
