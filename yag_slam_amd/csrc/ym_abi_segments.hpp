// ym_abi_segments.hpp -- C ABI: the segment graph of a prior map from its label image (ym_segments_*; ym_k_segments.hpp)
// Part of yagmatch.hip (included inside its extern "C" block); not a header of its own.
struct ym_segments {
    int device;
    int width, height, pitch; // the label image, resident on the device; pitch (elements) a multiple of 4
    int32_t min_label = 0, max_label = 0;
    OwnStream stream;
    DevBuf<int32_t> d_img;
    DevBuf<unsigned long long> sums, keys, first; // sums: count, sum_x, sum_y of every label, one after the other
    DevBuf<unsigned> counts, flags;
    DevBuf<int32_t> range, out_pairs, out_counts;
    DevBuf<long long> out_first;
    DevBuf<uint8_t> mask;
};

constexpr uint32_t kSegMaxSlots = 1u << 26; // the largest pair table the library grows to (20 bytes a slot)

static ym::SegArgs segments_args(const ym_segments *sg) {
    ym::SegArgs a{};
    a.img = sg->d_img.p; a.width = sg->width; a.height = sg->height; a.pitch = sg->pitch;
    a.flags = sg->flags.p;
    return a;
}

static dim3 segments_grid(const ym_segments *sg, int tile_h) {
    return dim3((unsigned)((sg->width + ym::kSegTileW - 1) / ym::kSegTileW), (unsigned)((sg->height + tile_h - 1) / tile_h));
}

// upload + the label range (one launch), so that every later call knows the labels' bounds
static int segments_upload(ym_segments *sg, const int32_t *labels, int pitch_elems) {
    const size_t n = (size_t)sg->pitch * sg->height;
    int rc; // (every allocation before the copy is queued: no return below leaves the caller's buffer the source of a copy in flight)
    if ((rc = sg->stream.create()) || (rc = sg->d_img.alloc(n)) || (rc = sg->range.ensure(2)) || (rc = sg->flags.ensure(4))) return rc;
    const size_t n_vec = (size_t)((sg->width + 3) / 4) * sg->height;
    const unsigned blocks = (unsigned)std::min<size_t>((n_vec + 255) / 256, ym::kSegRangeBlocks);
    const int32_t init[2] = {INT32_MAX, INT32_MIN};
    HIP_TRY(hipMemcpy(sg->range.p, init, sizeof init, hipMemcpyHostToDevice));
    // (the padding columns stay as they are: every kernel masks them by coordinate)
    HIP_TRY(hipMemcpy2D(sg->d_img.p, sizeof(int32_t) * sg->pitch, labels, sizeof(int32_t) * pitch_elems, sizeof(int32_t) * sg->width,
                        sg->height, hipMemcpyHostToDevice));
    ym::SegArgs a = segments_args(sg);
    a.range = sg->range.p;
    hipLaunchKernelGGL(ym::segment_range_kernel, dim3(blocks), dim3(256), 0, sg->stream, a);
    HIP_TRY(hipGetLastError());
    int32_t got[2];
    HIP_TRY(hipMemcpyAsync(got, sg->range.p, sizeof got, hipMemcpyDeviceToHost, sg->stream));
    HIP_TRY(hipStreamSynchronize(sg->stream));
    sg->min_label = got[0]; sg->max_label = got[1];
    return YM_OK;
}

ym_segments *ym_segments_create(int device, const int32_t *labels, int width, int height, int pitch_elems) {
    if (!labels || width < 1 || height < 1 || pitch_elems < width) { set_err(YM_ERR_INVALID, "bad label image"); return nullptr; }
    if (width > 65536 || height > 65536) {
        set_err(YM_ERR_INVALID, "label image of %d x %d pixels: at most 65536 x 65536 (the 64-bit sums stay exact)", width, height);
        return nullptr;
    }
    if (check_device(device) != YM_OK) return nullptr;
    DevGuard guard(device);
    if (guard.status() != YM_OK) return nullptr;
    ym_segments *sg = new ym_segments();
    sg->device = device; sg->width = width; sg->height = height; sg->pitch = (width + 3) / 4 * 4;
    if (segments_upload(sg, labels, pitch_elems) != YM_OK) { delete sg; return nullptr; } // (the error text is set)
    return sg;
}

int ym_segments_label_range(const ym_segments *sg, int32_t *min_label, int32_t *max_label) {
    if (!sg || !min_label || !max_label) return set_err(YM_ERR_INVALID, "null argument");
    *min_label = sg->min_label; *max_label = sg->max_label;
    return YM_OK;
}

int ym_segments_stats(ym_segments *sg, int n_labels, int64_t *count, int64_t *sum_x, int64_t *sum_y) {
    if (!sg) return set_err(YM_ERR_INVALID, "null segments");
    if (!count || !sum_x || !sum_y) return set_err(YM_ERR_INVALID, "null argument");
    if (n_labels < 1) return set_err(YM_ERR_INVALID, "n_labels %d: at least 1 (label 0)", n_labels);
    DEV_GUARD(sg->device);
    const size_t nl = (size_t)n_labels;
    int rc;
    if ((rc = sg->sums.ensure(3 * nl))) return rc;
    HIP_TRY(hipMemsetAsync(sg->sums.p, 0, 3 * nl * sizeof(unsigned long long), sg->stream));
    HIP_TRY(hipMemsetAsync(sg->flags.p, 0, 4 * sizeof(unsigned), sg->stream));
    ym::SegArgs a = segments_args(sg);
    a.n_labels = n_labels;
    a.count = sg->sums.p; a.sum_x = sg->sums.p + nl; a.sum_y = sg->sums.p + 2 * nl;
    hipLaunchKernelGGL(ym::segment_stats_kernel, segments_grid(sg, ym::kSegStatTileH), dim3(256), 0, sg->stream, a);
    HIP_TRY(hipGetLastError());
    unsigned flags[4];
    HIP_TRY(hipMemcpyAsync(flags, sg->flags.p, sizeof flags, hipMemcpyDeviceToHost, sg->stream));
    HIP_TRY(hipStreamSynchronize(sg->stream));
    // (the kernel tests every label itself and adds nothing for one outside: its flag is the one check of this call)
    if (flags[0]) return set_err(YM_ERR_INVALID, "a label outside [0, %d)", n_labels);
    // (the outputs are written only once the whole call has succeeded)
    HIP_TRY(hipMemcpy(count, a.count, nl * sizeof(int64_t), hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(sum_x, a.sum_x, nl * sizeof(int64_t), hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(sum_y, a.sum_y, nl * sizeof(int64_t), hipMemcpyDeviceToHost));
    return YM_OK;
}

int ym_segments_boundaries(ym_segments *sg, uint8_t *mask, int64_t mask_bytes) {
    if (!sg) return set_err(YM_ERR_INVALID, "null segments");
    const size_t n = (size_t)sg->width * sg->height;
    if (!mask || mask_bytes < 0 || (uint64_t)mask_bytes < n) return set_err(YM_ERR_INVALID, "mask buffer: %zu bytes needed", n);
    DEV_GUARD(sg->device);
    int rc;
    if ((rc = sg->mask.ensure(n))) return rc;
    ym::SegArgs a = segments_args(sg);
    a.mask = sg->mask.p;
    hipLaunchKernelGGL(ym::segment_edges_kernel<true>, segments_grid(sg, ym::kSegEdgeTileH), dim3(256), 0, sg->stream, a);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipStreamSynchronize(sg->stream));
    HIP_TRY(hipMemcpy(mask, sg->mask.p, n, hipMemcpyDeviceToHost));
    return YM_OK;
}

// one counting pass with a table of `slots`: YM_OK with *full = whether a pair found no slot, *used = the slots taken
static int segments_count_pairs(ym_segments *sg, uint32_t slots, bool *full, unsigned *used) {
    int rc;
    if ((rc = sg->keys.ensure(slots)) || (rc = sg->first.ensure(slots)) || (rc = sg->counts.ensure(slots))) return rc;
    HIP_TRY(hipMemsetAsync(sg->keys.p, 0xFF, (size_t)slots * sizeof(unsigned long long), sg->stream));
    HIP_TRY(hipMemsetAsync(sg->first.p, 0xFF, (size_t)slots * sizeof(unsigned long long), sg->stream));
    HIP_TRY(hipMemsetAsync(sg->counts.p, 0, (size_t)slots * sizeof(unsigned), sg->stream));
    HIP_TRY(hipMemsetAsync(sg->flags.p, 0, 4 * sizeof(unsigned), sg->stream));
    ym::SegArgs a = segments_args(sg);
    a.keys = sg->keys.p; a.pair_first = sg->first.p; a.pair_count = sg->counts.p; a.slots = slots;
    hipLaunchKernelGGL(ym::segment_edges_kernel<false>, segments_grid(sg, ym::kSegEdgeTileH), dim3(256), 0, sg->stream, a);
    HIP_TRY(hipGetLastError());
    unsigned flags[4];
    HIP_TRY(hipMemcpyAsync(flags, sg->flags.p, sizeof flags, hipMemcpyDeviceToHost, sg->stream));
    HIP_TRY(hipStreamSynchronize(sg->stream));
    *full = flags[1] != 0;
    *used = flags[2];
    return YM_OK;
}

int ym_segments_pairs(ym_segments *sg, int table_slots, int cap, int32_t *pairs, int32_t *counts, int64_t *first_index, int32_t *n_pairs) {
    if (!sg) return set_err(YM_ERR_INVALID, "null segments");
    if (!n_pairs || cap < 0 || table_slots < 0) return set_err(YM_ERR_INVALID, "bad argument");
    if (cap > 0 && (!pairs || !counts || !first_index)) return set_err(YM_ERR_INVALID, "null argument");
    if (sg->min_label < 0) return set_err(YM_ERR_INVALID, "a negative label (%d)", sg->min_label);
    DEV_GUARD(sg->device);
    // the table: the caller's size (rounded up to a power of two), or one slot per 16 pixels within [4096, 2^22]; a table
    // that turns out too small is counted again at four times the size -- a pair is never dropped
    uint32_t slots = 16;
    uint64_t want = table_slots > 0 ? (uint64_t)table_slots
                                    : std::min<uint64_t>(std::max<uint64_t>((uint64_t)sg->width * sg->height / 16, 4096), 1u << 22);
    want = std::min<uint64_t>(want, kSegMaxSlots);
    while (slots < want) slots <<= 1;
    bool full = true;
    unsigned used = 0;
    for (;;) {
        int rc = segments_count_pairs(sg, slots, &full, &used);
        if (rc != YM_OK) return rc;
        if (!full) break;
        if (slots >= kSegMaxSlots)
            return set_err(YM_ERR_UNSUPPORTED, "more label pairs than a table of %u slots holds", slots);
        slots = std::min<uint32_t>(slots << 2, kSegMaxSlots);
    }
    if ((int64_t)used > (int64_t)cap) {
        *n_pairs = (int32_t)used;
        return set_err(YM_ERR_INVALID, "%u pairs: the caller's arrays hold %d (n_pairs says how many are needed)", used, cap);
    }
    std::vector<int32_t> h_pairs(2 * (size_t)used), h_counts(used);
    std::vector<long long> h_first(used);
    if (used) {
        int rc;
        if ((rc = sg->out_pairs.ensure(2 * (size_t)used)) || (rc = sg->out_counts.ensure(used)) || (rc = sg->out_first.ensure(used))) return rc;
        ym::SegArgs a = segments_args(sg);
        a.keys = sg->keys.p; a.pair_first = sg->first.p; a.pair_count = sg->counts.p; a.slots = slots;
        a.out_pairs = sg->out_pairs.p; a.out_counts = sg->out_counts.p; a.out_first = sg->out_first.p;
        hipLaunchKernelGGL(ym::segment_compact_kernel, dim3((slots + 255) / 256), dim3(256), 0, sg->stream, a);
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipStreamSynchronize(sg->stream));
        HIP_TRY(hipMemcpy(h_pairs.data(), a.out_pairs, sizeof(int32_t) * 2 * used, hipMemcpyDeviceToHost));
        HIP_TRY(hipMemcpy(h_counts.data(), a.out_counts, sizeof(int32_t) * used, hipMemcpyDeviceToHost));
        HIP_TRY(hipMemcpy(h_first.data(), a.out_first, sizeof(long long) * used, hipMemcpyDeviceToHost));
    }
    // the reference's dict order: by the first boundary pixel that counted the pair (a pixel counts at most one pair, so
    // first indices are distinct and the order does not depend on where the table put the pairs)
    std::vector<uint32_t> order(used);
    for (uint32_t i = 0; i < used; i++) order[i] = i;
    std::sort(order.begin(), order.end(), [&](uint32_t p, uint32_t q) { return h_first[p] < h_first[q]; });
    for (uint32_t i = 0; i < used; i++) {
        const uint32_t o = order[i];
        pairs[2 * (size_t)i] = h_pairs[2 * (size_t)o];
        pairs[2 * (size_t)i + 1] = h_pairs[2 * (size_t)o + 1];
        counts[i] = h_counts[o];
        first_index[i] = (int64_t)h_first[o];
    }
    *n_pairs = (int32_t)used;
    return YM_OK;
}

void ym_segments_destroy(ym_segments *sg) {
    if (!sg) return;
    DevGuard guard(sg->device);
    delete sg;
}
