// ym_host_mapgrow.hpp -- host runtime: what every call that changes a resident correlation map is made of (ym_abi_maps.hpp:
// ym_map_add_scans, ym_map_update_scans, ym_map_reframe), and the one that only asks it a question (ym_map_seen_through).  The
// kernels are those of ym_k_mapgrow.hpp and ym_k_seenthrough.hpp, the window's integer arithmetic that of ym_map_window.hpp;
// DESIGN.md sections 15 to 17 and 19.
// Part of yagmatch.hip (included inside its anonymous namespace); not a header of its own.

// scans of one launch: the cells of every beam take 4 bytes, grid.y stays far below its limit
static const int kMapGrowChunk = 4096;

static_assert((int)ym::kMgX0 == (int)ym::kMuX0 && ym::kMgY0 == ym::kMgX0 + 1 && ym::kMgX1 == ym::kMgX0 + 2 && ym::kMgY1 == ym::kMgX0 + 3 &&
                  ym::kMuY0 == ym::kMuX0 + 1 && ym::kMuX1 == ym::kMuX0 + 2 && ym::kMuY1 == ym::kMuX0 + 3,
              "both statistics blocks keep their box in four consecutive slots, at the same place");

// ---- the checks of a map-changing call
int map_call_check(const ym_matcher *m, const ym_map *mp, const char *call) {
    if (!m || !mp) return set_err(YM_ERR_INVALID, "null argument");
    if (m->cfg.semantics != YM_SEM_YAGPY) return set_err(YM_ERR_UNSUPPORTED, "%s needs a YM_SEM_YAGPY matcher", call);
    if (mp->device != m->device) return set_err(YM_ERR_INVALID, "map lives on another device");
    return YM_OK;
}

// a list of scans ("scan", "removed scan", "held scan"): *max_n grows to its longest, *beams (where given) by all its beams
int map_scan_list(const ym_matcher *m, const ym_scan *const *scans, int n, const char *noun, int *max_n, size_t *beams = nullptr) {
    for (int i = 0; i < n; i++) {
        if (!scans[i] || scans[i]->device != m->device) return set_err(YM_ERR_INVALID, "%s %d is null or lives on another device", noun, i);
        *max_n = std::max(*max_n, scans[i]->n);
        if (beams) *beams += (size_t)scans[i]->n;
    }
    return YM_OK;
}

inline int map_ksize(const ym_matcher *m) { return 2 * m->geom.half_kernel + 1; }
inline size_t map_halo_bytes(int ks) { return (size_t)(ym::kMfTileW + ks - 1) * (size_t)(ym::kMfTileH + ks - 1); }

// what one launch holds: the (beam, tap) lanes of a scan, and -- for a call that recomputes -- the gather's tile and halo in LDS
int map_launch_limits(int max_n, int ks, bool recompute) {
    if ((double)max_n * ks * ks > 2.0e9) return set_err(YM_ERR_UNSUPPORTED, "%d beams x %d x %d taps: more than one launch holds", max_n, ks, ks);
    if (recompute && map_halo_bytes(ks) > 65536)
        return set_err(YM_ERR_UNSUPPORTED, "%d x %d taps: the recompute's tile and halo (%zu bytes) do not fit 64 KiB of LDS", ks, ks, map_halo_bytes(ks));
    return YM_OK;
}

// the float taps on the device, uploaded on the call's stream (every call: the table is small and the options may have changed it)
int map_taps_upload(ym_matcher *m) {
    int rc;
    if ((rc = m->kernel_f_dev.ensure(m->kernel_f.size()))) return rc;
    HIP_TRY(hipMemcpyAsync(m->kernel_f_dev.p, m->kernel_f.data(), m->kernel_f.size() * sizeof(double), hipMemcpyHostToDevice, m->stream));
    return YM_OK;
}

// the matcher's workspace for stamp passes over lists of up to `longest` scans
int map_workspace(ym_matcher *m, int longest, int max_n) {
    const int chunk = std::min(longest, kMapGrowChunk);
    int rc;
    if ((rc = m->grow_scans.ensure((size_t)chunk)) || (rc = m->grow_cells.ensure((size_t)chunk * max_n))) return rc;
    return YM_OK;
}

// ---- the kernels' argument structs for one target
struct MapTarget {
    double *cgrid; uint8_t *g8; uint32_t *stamps; uint8_t *dirty; // stamps, dirty: counted maps
    int width, height;
    // world position of lattice cell (0, 0) and the window's offset.  A counted map: its anchor and its window's integer offset; an
    // uncounted one: the caller's origin and 0.  (Not the same thing: anchor + offset * res and the caller's fp64 origin differ.)
    double ox, oy;
    int wx0, wy0;
    ymm::Box exclude; // ym_map_reframe: the overlap, whose counts were copied; empty for every other caller
};

struct MapPassArgs { ym::MapGrowArgs a; ym::MapForgetArgs f; ym::SeenArgs s; }; // (s: ym_map_seen_through fills it, zero elsewhere)

// (after map_workspace and map_taps_upload: the structs hold the workspace's pointers)
MapPassArgs map_pass_args(const ym_matcher *m, const MapTarget &t, int max_n) {
    MapPassArgs p;
    std::memset(&p, 0, sizeof p);
    const int ks = map_ksize(m);
    ym::MapGrowArgs &a = p.a;
    a.scans = m->grow_scans.p; a.max_n = max_n; a.width = t.width; a.height = t.height;
    a.ox = t.ox; a.oy = t.oy; a.res = m->cfg.resolution; a.wx0 = t.wx0; a.wy0 = t.wy0;
    a.ex0 = t.exclude.x0; a.ey0 = t.exclude.y0; a.ex1 = t.exclude.x1; a.ey1 = t.exclude.y1;
    a.cells = m->grow_cells.p; a.kernel = m->kernel_f_dev.p; a.ksize = ks;
    a.cgrid = t.cgrid; a.g8 = t.g8;
    ym::MapForgetArgs &f = p.f;
    f.cells = m->grow_cells.p; f.max_n = max_n; f.width = t.width; f.height = t.height;
    f.stamps = t.stamps; f.released = m->grow_released.p; f.dirty = t.dirty;
    f.kernel = m->kernel_f_dev.p; f.ksize = ks; f.cgrid = t.cgrid; f.g8 = t.g8;
    return p;
}

// ---- one call's host side of its asynchronous copies.  The caller holds it until its stream wait: the copies read `refs` and
// `init` and write `got` while the stream runs.
// The statistics in m->grow_stats: n_grow blocks of kMgStatSlots (one per kind of stamp pass), then -- for a counted target -- one of
// kMuStatSlots.
struct MapJob {
    enum { kMaxSlots = 2 * ym::kMgStatSlots + ym::kMuStatSlots };
    std::vector<YmScanRef> refs; // every scan of the call, in the order of its passes
    size_t used = 0;
    unsigned long long init[kMaxSlots], got[kMaxSlots];
    int n_slots = 0, upd = 0;    // upd: where the kMuStatSlots block begins

    // n_scans: over all passes.  Enqueues the statistics' initial values: zero, the boxes' minima at the largest value.
    int begin(ym_matcher *m, int n_scans, int n_grow, bool counted) {
        refs.assign((size_t)n_scans, YmScanRef());
        used = 0;
        upd = n_grow * ym::kMgStatSlots;
        n_slots = upd + (counted ? (int)ym::kMuStatSlots : 0);
        int rc;
        if ((rc = m->grow_stats.ensure((size_t)n_slots))) return rc;
        for (int i = 0; i < n_slots; i++) init[i] = got[i] = 0;
        for (int b = 0; b < n_grow; b++) init[b * ym::kMgStatSlots + ym::kMgX0] = init[b * ym::kMgStatSlots + ym::kMgY0] = ~0ull;
        if (counted) init[upd + ym::kMuX0] = init[upd + ym::kMuY0] = ~0ull;
        HIP_TRY(hipMemcpyAsync(m->grow_stats.p, init, sizeof(unsigned long long) * (size_t)n_slots, hipMemcpyHostToDevice, m->stream));
        return YM_OK;
    }
    // enqueues the copy of the statistics to `got`: valid after the caller's stream wait
    int fetch(ym_matcher *m) {
        HIP_TRY(hipMemcpyAsync(got, m->grow_stats.p, sizeof(unsigned long long) * (size_t)n_slots, hipMemcpyDeviceToHost, m->stream));
        return YM_OK;
    }
};

// ---- the stamp pass: `n` scans (at `poses`, [n][3], or at their own) through cells -> count -> smear, a chunk at a time.
// grow_block: the kMgStatSlots block of the job's statistics this pass counts in.
// kMapCountSeen changes nothing: seen_count_kernel reads the mask at the cells and writes scan c0 + i's counts and flags (pa.s).
enum MapCount { kMapCountNone, kMapCountAdd, kMapCountRemove, kMapCountSeen };

int map_stamp_pass(ym_matcher *m, MapJob &job, MapPassArgs pa, const ym_scan *const *scans, const double *poses, int n, MapCount count,
                   bool smear, int grow_block) {
    if (job.used + (size_t)n > job.refs.size()) return set_err(YM_ERR_INVALID, "the map job holds fewer scans than its passes stage");
    hipStream_t st = m->stream;
    ym::MapGrowArgs &a = pa.a;
    a.stats = m->grow_stats.p + grow_block * ym::kMgStatSlots;
    pa.f.stats = m->grow_stats.p + job.upd;
    const int kk = a.ksize * a.ksize;
    const dim3 beams((unsigned)((a.max_n + 255) / 256)), taps((unsigned)(((size_t)a.max_n * kk + 255) / 256));
    for (int c0 = 0; c0 < n; c0 += kMapGrowChunk) {
        const int B = std::min(kMapGrowChunk, n - c0);
        YmScanRef *hs = job.refs.data() + job.used;
        for (int i = 0; i < B; i++) hs[i] = scan_ref(scans[c0 + i], poses ? poses + 3 * (size_t)(c0 + i) : nullptr);
        job.used += (size_t)B;
        HIP_TRY(hipMemcpyAsync(m->grow_scans.p, hs, sizeof(YmScanRef) * (size_t)B, hipMemcpyHostToDevice, st));
        a.n_scans = B;
        hipLaunchKernelGGL(ym::map_grow_cells_kernel, dim3(B), dim3(1024), 0, st, a);
        if (count == kMapCountRemove) hipLaunchKernelGGL(ym::map_count_kernel<true>, dim3(beams.x, B), dim3(256), 0, st, pa.f);
        if (count == kMapCountAdd) hipLaunchKernelGGL(ym::map_count_kernel<false>, dim3(beams.x, B), dim3(256), 0, st, pa.f);
        if (count == kMapCountSeen) {
            ym::SeenArgs s = pa.s;
            s.counts += 2 * (size_t)c0;
            if (s.flags) s.flags += (size_t)c0 * (size_t)s.max_n;
            hipLaunchKernelGGL(ym::seen_count_kernel, dim3(B), dim3(256), 0, st, s);
        }
        if (smear) {
            hipLaunchKernelGGL(ym::map_grow_smear_kernel<false>, dim3(taps.x, B), dim3(256), 0, st, a);
            hipLaunchKernelGGL(ym::map_grow_smear_kernel<true>, dim3(taps.x, B), dim3(256), 0, st, a);
        }
        HIP_TRY(hipGetLastError());
    }
    return YM_OK;
}

// ---- the recompute: map_forget_gather_kernel over the tiles of `box`, in pieces of rows.  The caller has flagged the cells.
int map_recompute(ym_matcher *m, ym::MapForgetArgs f, const ymm::Box &box) {
    const ymm::TileGrid t = ymm::tile_grid(box, ym::kMfTileW, ym::kMfTileH);
    f.bx0 = t.bx0; f.bx1 = box.x1; f.by1 = box.y1;
    for (unsigned k = 0; k < ymm::row_pieces(t.tiles_y); k++) {
        const ymm::RowPiece p = ymm::row_piece(t.tiles_y, k);
        f.by0 = t.by0 + (int)p.first * ym::kMfTileH;
        hipLaunchKernelGGL(ym::map_forget_gather_kernel, dim3(t.tiles_x, p.count), dim3(256), map_halo_bytes(f.ksize), m->stream, f);
    }
    HIP_TRY(hipGetLastError());
    return YM_OK;
}

// ---- ym_map_reframe's mark: map_reframe_mark_kernel over `rect`, in pieces of rows
int map_reframe_mark(ym_matcher *m, ym::MapReframeArgs r, const ymm::Box &rect) {
    if (rect.empty()) return YM_OK;
    const unsigned rows = (unsigned)(rect.y1 - rect.y0);
    r.mx0 = rect.x0; r.mx1 = rect.x1; r.my1 = rect.y1;
    for (unsigned k = 0; k < ymm::row_pieces(rows); k++) {
        const ymm::RowPiece p = ymm::row_piece(rows, k);
        r.my0 = rect.y0 + (int)p.first;
        hipLaunchKernelGGL(ym::map_reframe_mark_kernel, dim3((unsigned)((r.mx1 - r.mx0 + 255) / 256), p.count), dim3(256), 0, m->stream, r);
    }
    HIP_TRY(hipGetLastError());
    return YM_OK;
}
