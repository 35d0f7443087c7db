/*
 * yagmatch.h -- C ABI of libyagmatch.so, the MI355X-native correlative scan matcher.
 *
 * Drop-in boundary for yag-slam's match_scan path.  The reference crosses into native code through
 * pybind11 (karto_scanmatcher==1.0.0, /root/reference/setup.py:46), not through a C API, so each
 * entry point below names the pybind11 object/method it replaces:
 *
 *   ym_create / ym_destroy        karto_scanmatcher.Wrapper(ScanMatcherConfig)
 *                                 /root/reference/yag_slam/scan_matching.py:33-38, /root/reference/test.py:24-25
 *   ym_scan_create / _set_pose    karto_scanmatcher.LocalizedRangeScan(LaserScanConfig, ranges, Pose2, Pose2, num, time)
 *                                 and its .corrected_pose setter
 *                                 /root/reference/yag_slam/models.py:37-39,67-75, /root/reference/test.py:27-36
 *   ym_match_scans                Wrapper.match_scan(query._scan, [b._scan ...], penalty, do_fine)
 *                                 /root/reference/yag_slam/scan_matching.py:40-42, /root/reference/test.py:38
 *   ym_match                      same call, for callers that hold plain range arrays (no resident scan)
 *   ym_match_batch, ym_batch_*    the serial chain loop of GraphSlam.try_to_close_loop
 *                                 /root/reference/yag_slam/graph_slam.py:217-236 (one query, many chains)
 *   ym_match_pairs, ym_pairs_create  N independent Wrapper.match_scan calls (N x /root/reference/yag_slam/graph_slam.py:326:
 *                                 N robots, or N segments of a log replayed side by side) in one enqueue: item i =
 *                                 query i against chain i
 *   ym_result                     the returned object's .response / .covariance / .best_pose
 *                                 /root/reference/yag_slam/scan_matching.py:42, /root/reference/test.py:39-41
 *
 * Conventions: POD only; the caller owns every input buffer and the library copies on entry; no
 * C++ exception crosses the boundary -- functions return YM_OK (0) or a negative YM_ERR_* and
 * ym_last_error() gives the text (thread-local).  One ym_matcher owns one HIP stream and one
 * device workspace: it is NOT re-entrant (the reference's matcher is not either: it owns a mutable
 * grid and is driven from one worker thread, /root/reference/ros1/slam_node_ros1:223-255).
 * Distinct matchers are independent.  There is no CPU fallback: without a usable HIP device
 * ym_create fails with YM_ERR_NO_DEVICE.
 */
#ifndef YAGMATCH_H
#define YAGMATCH_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define YM_VERSION 1

enum {
    YM_OK = 0,
    YM_ERR_INVALID = -1,     /* bad argument / bad config */
    YM_ERR_NO_DEVICE = -2,   /* no HIP device, or device index out of range */
    YM_ERR_HIP = -3,         /* a HIP runtime call failed */
    YM_ERR_UNSUPPORTED = -4, /* valid request this build cannot serve */
    YM_ERR_RANGE = -5,       /* Karto's "index out of range" / "unable to find best position" */
    YM_ERR_BUSY = -6         /* async slot still in flight / not submitted */
};

enum { YM_SEM_KARTO = 0, YM_SEM_YAGPY = 1 };

/* The 11 keys of yag-slam's config dict (/root/reference/yag_slam/helpers.py:339-351), Karto's
 * MinimumDistancePenalty, and the semantics switch. */
typedef struct ym_config {
    double angle_variance_penalty;
    double distance_variance_penalty;
    double coarse_search_angle_offset;
    double coarse_angle_resolution;
    double fine_search_angle_resolution;
    double range_threshold;
    double minimum_angle_penalty;
    double minimum_distance_penalty;
    double search_size;
    double resolution;
    double smear_deviation;
    int32_t use_response_expansion;
    int32_t semantics; /* YM_SEM_KARTO | YM_SEM_YAGPY */
} ym_config;

/* LaserScanConfig + ranges + corrected pose (/root/reference/yag_slam/models.py:25-39) */
typedef struct ym_scan_desc {
    const double *ranges; /* host pointer, n readings */
    int32_t n;
    int32_t reserved;
    double min_angle;
    double max_angle;
    double angle_increment;
    double min_range;
    double max_range;
    double range_threshold;
    double pose[3]; /* x, y, heading */
} ym_scan_desc;

typedef struct ym_result {
    double response;
    double pose[3];  /* best_pose x, y, heading */
    double cov[9];   /* row-major 3x3 covariance */
    double coarse_response; /* best response of the (last) coarse pass */
    int64_t hypotheses;     /* lattice points scored (all passes, incl. expansions) */
    int32_t coarse_dims[3]; /* nx, ny, ntheta */
    int32_t fine_dims[3];   /* nx, ny, ntheta (0 when !refine) */
    int32_t n_query_points; /* response normaliser */
    int32_t expansions;     /* response-expansion retries taken */
    int32_t status;         /* YM_OK or YM_ERR_RANGE for this item */
    int32_t reserved;       /* 0; ym_map_track: 1 when the step's correction was NOT applied (response < min_response: the scan
                               keeps its odometry prior), status staying 0 */
} ym_result;

typedef struct ym_matcher ym_matcher;
typedef struct ym_scan ym_scan;

/* ---- library / device ---- */
int ym_version(void);
/* first 16 hex digits of the SHA-256 of the sources this library was built from (csrc/Makefile): ties a profile to a build */
const char *ym_build_id(void);
int ym_device_count(void);
const char *ym_last_error(void);

/* ---- matcher ---- */
ym_matcher *ym_create(const ym_config *cfg, int device);
void ym_destroy(ym_matcher *m);
int ym_get_config(const ym_matcher *m, ym_config *out);
/* run on a caller-owned hipStream_t (e.g. torch's current stream); NULL -> the matcher's own */
int ym_set_stream(ym_matcher *m, void *hip_stream);
int ym_synchronize(ym_matcher *m);

/* ---- resident scans (device twin of LocalizedRangeScan) ----
 * ym_scan_create copies the readings (desc->ranges is free again on return) and costs one kernel launch without a
 * synchronisation (~20 us): the upload and the scan's chain structure complete on the device while the caller goes on,
 * and whoever uses the scan first waits for them.  The device memory comes from a per-device pool of the library:
 * ym_scan_destroy never synchronises the device (hipFree does), the block of a destroyed scan serves a later
 * ym_scan_create, and the pool keeps what it has allocated for the life of the process (35 KB per 1081-beam scan alive
 * at the same time). */
ym_scan *ym_scan_create(int device, const ym_scan_desc *desc);
/* n scans at once: what n ym_scan_create calls leave behind (the same host code per scan, the same kernel), in one pool transaction,
 * one upload and one launch per 2048 scans -- the reference builds one C++ scan per Python scan before match_scan
 * (/root/reference/yag_slam/models.py:25-39); a node that receives the scans of N robots per step, or a map file being loaded,
 * builds thousands.  out receives n handles.  All or nothing: on failure nothing stays allocated.  The scans come back complete
 * (nothing of their creation is still in flight).  ym_scans_destroy: n ym_scan_destroy calls in one pool transaction. */
int ym_scans_create(int device, const ym_scan_desc *descs, int n, ym_scan **out);
void ym_scans_destroy(ym_scan *const *scans, int n);
int ym_scan_set_pose(ym_scan *s, double x, double y, double heading);
/* n poses (x, y, heading) written to n scans in one call -- what the reference does scan by scan after every graph
 * optimisation (/root/reference/yag_slam/graph_slam.py:263-272: `vtx.obj.corrected_pose = ...` for EVERY vertex, one pybind11
 * write each, /root/reference/yag_slam/models.py:67-75).  All or nothing: a null entry fails the call before any pose is written. */
int ym_scans_set_poses(ym_scan *const *scans, const double *xyz, int n);
int ym_scan_get_pose(const ym_scan *s, double pose[3]);
int ym_scan_size(const ym_scan *s);
/* 1: the scan's trigger-chain structure, computed once at creation in the sensor frame, holds at every pose (no distance
 * test of the valid-point filter came within 1e-9 m^2 of its threshold); 0: the matchers recompute it per pose */
int ym_scan_structure_trusted(const ym_scan *s, int semantics);
void ym_scan_destroy(ym_scan *s);

/* ---- the hot path ---- */
int ym_match(ym_matcher *m, const ym_scan_desc *query, const ym_scan_desc *base, int n_base,
             int penalize, int refine, ym_result *out);
int ym_match_scans(ym_matcher *m, const ym_scan *query, const ym_scan *const *base, int n_base,
                   int penalize, int refine, ym_result *out);

/* The matcher calls of GraphSlam.process_scan for a whole trajectory, in one call
 * (/root/reference/yag_slam/graph_slam.py:306-339; the host loop a robot log is replayed with):
 *   for i = max(start, 1) .. n-1:
 *       prior_i     = corrected_{i-1} (+) (odom_i (-) odom_{i-1})                                graph_slam.py:320-324
 *       results[i]  = match(scans[i] at prior_i, scans[max(0, i - buffer_len) .. i-1], penalize, refine)
 *       corrected_i = results[i].pose                                                             graph_slam.py:326-337
 * with tiny_tf's planar Transform arithmetic ((+) composes, a (-) b = inverse(b) (+) a), operation for operation what
 * yag_slam_amd/transform.py does, so the poses are bit-identical to the per-scan calls.  scans[0 .. start) are the
 * running chain so far and keep their poses; every later scan's pose is set to its prior and then to its result (as
 * ym_scan_set_pose would).  odom = n poses (x, y, heading).  results = n entries, those of scans that are not matched
 * are zeroed.  Stops at the first scan whose match reports YM_ERR_RANGE in its result (its pose stays at the prior);
 * *n_done = index of the first scan NOT completed (n when all are).
 * device_chain != 0: no host round trip between steps either.  The steps are enqueued back to back, 128 at a time; the
 * kernel that ends step i leaves scan i's pose and scan i+1's prior in device memory, where step i+1's kernels read them,
 * and the host -- planning ahead of the device -- sizes each step's raster from poses it dead-reckons with the odometry
 * alone.  The priors are then composed with the DEVICE's cos / sin: poses and responses agree with the synchronous form
 * to rounding (~1e-12), not bit for bit.  A step whose cells leave the predicted rectangle, that Karto would abort, or
 * that needs a response expansion is detected on the device, the rest of its segment is skipped, and the step is repeated
 * synchronously.  Karto semantics, resident scans, buffer_len < 16; anything else runs synchronously. */
int ym_map_sequence(ym_matcher *m, ym_scan *const *scans, const double *odom, int n, int start, int buffer_len,
                    int penalize, int refine, int device_chain, ym_result *results, int32_t *n_done);

/* The same for ONE scan, for callers that receive their scans one at a time (GraphSlam.process_scan itself): prior =
 * chain[n_chain-1]'s pose (+) (odom_query (-) odom_last), the query's pose is set to it, the match runs against `chain`,
 * and the query's pose becomes the result's (it stays at the prior if result->status != 0).  Bit-identical to setting the
 * prior with ym_scan_set_pose and calling ym_match_scans; it only saves the caller the arithmetic and two calls. */
int ym_process_scan(ym_matcher *m, ym_scan *query, ym_scan *const *chain, int n_chain, const double *odom_last,
                    const double *odom_query, int penalize, int refine, ym_result *result);

/* counters of ym_map_sequence since ym_create: device-chained segments enqueued, segments a fault cut short, steps run
 * synchronously (all of them without device_chain) */
int ym_sequence_stats(const ym_matcher *m, int64_t *segments, int64_t *faults, int64_t *sync_steps);

/* Pipelined form: enqueue on the matcher's stream, collect later.  `slot` in [0, ym_async_slots). */
int ym_async_slots(const ym_matcher *m);
int ym_match_scans_async(ym_matcher *m, const ym_scan *query, const ym_scan *const *base, int n_base,
                         int penalize, int refine, int slot);
int ym_wait(ym_matcher *m, int slot, ym_result *out);

/* One query against n_chains candidate chains; chain c = scans[chain_offsets[c] .. chain_offsets[c+1]).
 * per_chain (nullable) receives every chain's result; best/best_chain (nullable) the arg-max over
 * response, ties to the lowest chain index. */
int ym_match_batch(ym_matcher *m, const ym_scan *query, const ym_scan *const *scans,
                   const int32_t *chain_offsets, int n_chains, int penalize, int refine,
                   ym_result *per_chain, ym_result *best, int32_t *best_chain);

/* The same as a reusable object + pipelined run.  A batch only remembers WHICH scans form the chains;
 * poses are read from the scans at every run.  If dev_best_out (nullable, DEVICE pointer to 8
 * doubles) is given, {response, chain_id_base + best chain, x, y, heading, cov_xx, cov_yy, cov_tt} of
 * the best chain is also left on the device, stream-ordered, as the payload of a cross-rank
 * arg-max (RCCL all-gather of one such record per rank).  That record is written before Karto's
 * response expansion (a host-side re-run of the items whose coarse response is 0): when an
 * expansion took place, ym_batch_wait rewrites it from the final results, so a caller that needs
 * the post-expansion record waits for the slot before it gathers. */
typedef struct ym_batch ym_batch;
ym_batch *ym_batch_create(ym_matcher *m, const ym_scan *query, const ym_scan *const *scans,
                          const int32_t *chain_offsets, int n_chains);
void ym_batch_destroy(ym_batch *b);
int ym_batch_size(const ym_batch *b);
int ym_batch_run_async(ym_matcher *m, const ym_batch *b, int penalize, int refine, int slot,
                       int64_t chain_id_base, void *dev_best_out);
int ym_batch_wait(ym_matcher *m, int slot, ym_result *per_chain, ym_result *best, int32_t *best_chain);

/* n_items INDEPENDENT matches in one enqueue: item i = queries[i] against scans[chain_offsets[i] .. chain_offsets[i+1])
 * -- what n_items separate Wrapper.match_scan(query_i._scan, chain_i, penalty, do_fine) calls compute
 * (/root/reference/yag_slam/scan_matching.py:40-42, called once per incoming scan at /root/reference/yag_slam/graph_slam.py:326),
 * item for item bit-identical to ym_match_scans(queries[i], chain i).  A query object may serve several items (it is projected,
 * and its (beam, angle) pair lists are built, once per distinct object); ym_match_batch is the special case of ONE query.
 * per_item receives n_items results.  ym_pairs_create gives the reusable form: the object is a ym_batch -- run it with
 * ym_batch_run_async / ym_batch_wait (whose best / best_chain then name the item with the highest response), free it with
 * ym_batch_destroy. */
int ym_match_pairs(ym_matcher *m, const ym_scan *const *queries, const ym_scan *const *scans,
                   const int32_t *chain_offsets, int n_items, int penalize, int refine, ym_result *per_item);
ym_batch *ym_pairs_create(ym_matcher *m, const ym_scan *const *queries, const ym_scan *const *scans,
                          const int32_t *chain_offsets, int n_items);

/* ---- one match split over several matchers by coarse angle (BASELINE configs[4] on 8 GPUs: one matcher per GPU) ----
 * Every rank rasterises the same grid and scores the coarse angles [k_begin, k_end) only, writing their responses at
 * their place in the caller-owned device volume dev_resp[nt][ny][nx] (doubles) and the per-(x, y) maxima of its slices
 * into dev_probs[ny][nx] (doubles, cleared by the call).  The caller then completes both across ranks on the matcher's
 * stream -- all-gather of the slices, element-wise MAX of dev_probs (RCCL) -- and calls _finish, which runs the rest of
 * the match (arg-max, tie mean, covariances, the fine pass) on the whole volume: the result is bit-identical to an
 * unsplit ym_match_scans on every rank.  Karto semantics only. */
int ym_coarse_dims(const ym_matcher *m, int32_t dims[3]); /* nx, ny, ntheta of the coarse lattice */
int ym_match_slice_begin(ym_matcher *m, const ym_scan *query, const ym_scan *const *base, int n_base, int penalize,
                         int refine, int k_begin, int k_end, double *dev_resp, double *dev_probs);
int ym_match_slice_finish(ym_matcher *m, ym_result *out);

/* ---- match against a prebuilt map (reference: Scan2DMatcherPy.match_scan_sets_with_map,
 * /root/reference/yag_slam/scan_matching.py:124-173; YM_SEM_YAGPY matchers only -- Karto has no such entry) ---- */
typedef struct ym_map ym_map;
/* occupancy_grid_map_to_correlation_grid (/root/reference/yag_slam/helpers.py:24-34): every pixel of `image` equal to
 * occupied_value becomes 1.0 and is max-smeared with the matcher's kernel (resolution, smear_deviation), on the device */
ym_map *ym_map_from_occupancy(ym_matcher *m, const uint8_t *image, int width, int height, int pitch, int occupied_value);
/* a correlation grid (float64 in [0, 1], row-major [y][x]) computed elsewhere */
ym_map *ym_map_from_grid(ym_matcher *m, const double *cgrid, int width, int height);
int ym_map_size(const ym_map *map, int *width, int *height);
int ym_map_read(const ym_map *map, double *out, int64_t out_count); /* the float grid, width*height entries */
void ym_map_destroy(ym_map *map);
/* ---- maps that take scans: the reference's add_scan_to_grid (yag_slam/helpers.py:105-131) into a map
 * that stays on the device, so that a map can start empty or a prior map can be kept current while scans are tracked in it.
 *   ym_map_create_empty  a map of zeros; the size limits and the YM_SEM_YAGPY-only rule of the two creators above.
 *   ym_map_add_scans     every point reading of every scan at the scan's current pose (LocalizedRangeScan.points(): the readings
 *                        that are neither NaN nor above the scan's range threshold; no view-point filter, as
 *                        occupancy_grid_map_to_correlation_grid has none) goes to the cell gx = rint((x - ox) / res),
 *                        gy = rint((y - oy) / res) -- world_to_grid, helpers.py:82-83: fp64 division, round half to even; res is the
 *                        matcher's resolution, (ox, oy) the world position of cell (0, 0).  Inside the map the cell becomes 1.0 and every
 *                        tap (sx, sy) of the matcher's float kernel raises cell (gy + sy - half, gx + sx - half) to max(current,
 *                        kernel[sy][sx]) where that cell exists; a reading outside the map, or whose quotient is not finite, is
 *                        dropped and counted.  Every write is a maximum, so the map does not depend on the order of points, of
 *                        scans or of calls: it is bit for bit what the reference's sequential loop leaves, and what
 *                        ym_map_from_occupancy makes of the image whose occupied pixels are the stamped cells.  The map must hold
 *                        values in [0, 1] (what all three creators give).  Both forms of the map -- the float grid ym_map_read
 *                        returns and the bytes every match reads -- are current when the call returns.  Runs on the matcher's
 *                        stream, synchronous, never throws.  n_scans == 0 (scans may then be null) and scans without a valid
 *                        reading change nothing.  stats (nullable): the readings seen, stamped and dropped, and a rectangle
 *                        [x0, x1) x [y0, y1) that holds every changed cell (all 0 when nothing was stamped).
 *                        A ym_locator copies the map when it is created: one made before an add does not see it.
 *   ym_map_clear         every cell back to zero.
 * YM_ERR_INVALID: a null argument, a negative n_scans, a null scan, a scan or a map on another device than the matcher.
 * YM_ERR_UNSUPPORTED: a matcher that is not YM_SEM_YAGPY. */
typedef struct ym_map_add_stats {
    int64_t points, stamped, dropped; /* points = stamped + dropped */
    int32_t x0, y0, x1, y1;           /* cells changed lie inside [x0, x1) x [y0, y1); empty: all 0 */
} ym_map_add_stats;
ym_map *ym_map_create_empty(ym_matcher *m, int width, int height);
int ym_map_add_scans(ym_matcher *m, ym_map *map, double ox, double oy, const ym_scan *const *scans, int n_scans,
                     ym_map_add_stats *stats /* or null */);
int ym_map_clear(ym_matcher *m, ym_map *map);
/* ---- maps that forget.  A maximum cannot be undone, so a map that is to let scans go keeps counts.
 *   ym_map_create_counted  an empty map like ym_map_create_empty's (the same size limits, YM_SEM_YAGPY only) that also holds
 *                        uint32 stamps[height][width], the number of readings currently stamped in each cell, and whose origin
 *                        (ox, oy) -- the world position of cell (0, 0) -- is fixed here.  Standing invariant: the float grid and the
 *                        bytes are what ym_map_from_occupancy makes of the image stamps > 0, bit for bit.  The maps of the other three
 *                        creators are not counted and behave as before.
 *   on a counted map     ym_map_add_scans also adds 1 to the count of every stamped reading's cell; ox, oy other than the map's give
 *                        YM_ERR_INVALID and change nothing.  ym_map_clear zeroes the counts too.
 *   ym_map_update_scans  takes remove[i] out at remove_poses[i] -- the pose it was ADDED at, which need not be its current one
 *                        (ym_occmap_accumulate takes poses the same way) -- and then adds add[j] at its current pose; a scan in both
 *                        lists is moved.  A removed reading takes its cell's count down by one; the cells whose count reaches zero are
 *                        released, and exactly the cells within the taps' reach of a released cell are recomputed from the counts (the
 *                        largest tap over the stamped cells that reach them, 1.0 on a stamped cell), after the added readings are in.
 *                        Everything else is left as it is: the call costs what the released cells reach, not what the map holds.  A
 *                        removed reading outside the map is dropped, as it was when it was added.  One that meets a count of zero --
 *                        the scan was not added at that pose: the caller's error -- changes nothing and is counted in
 *                        stats->unmatched; no count ever goes below zero and the invariant holds whatever is removed.  Runs on the
 *                        matcher's stream, synchronous, never throws; both forms of the map are current on return.  Either list
 *                        may be empty (its pointers may then be null).
 *   ym_map_counted       1 for a counted map, else 0 (a null map: 0).
 *   ym_map_read_stamps   the counts, width * height entries (a test hook).
 * YM_ERR_INVALID: a null argument, a negative count, a null scan, a scan or a map on another device than the matcher.
 * YM_ERR_UNSUPPORTED: a map that is not counted, a matcher that is not YM_SEM_YAGPY, taps so wide that a 64 x 4 tile with their
 * reach around it exceeds 64 KiB of LDS (more than 221 x 221; removal only).  A refused call changes nothing. */
typedef struct ym_map_update_stats {
    int64_t removed, added;   /* readings taken out of and stamped into the map */
    int64_t dropped;          /* readings of either list outside the map */
    int64_t unmatched;        /* removed readings that met a count of zero */
    int64_t released, gained; /* cells whose count fell to zero, cells whose count rose from zero */
    int32_t x0, y0, x1, y1;   /* cells changed lie inside [x0, x1) x [y0, y1); empty: all 0 */
} ym_map_update_stats;
ym_map *ym_map_create_counted(ym_matcher *m, int width, int height, double ox, double oy);
int ym_map_update_scans(ym_matcher *m, ym_map *map, const ym_scan *const *remove, const double *remove_poses /* [n_remove][3] */,
                        int n_remove, const ym_scan *const *add, int n_add, ym_map_update_stats *stats /* or null */);
int ym_map_counted(const ym_map *map);
int ym_map_read_stamps(const ym_map *map, uint32_t *out, int64_t out_count);
/* ---- maps whose window moves.  A map has a window in cells of an anchor lattice: an integer offset (x0, y0)
 * and a size.  The maps of the creators above have offset (0, 0); the anchor (ax, ay) of a counted map is the origin it was created
 * with and never changes.  On a counted map the cell of a reading is (rint((x - ax) / res) - x0, rint((y - ay) / res) - y0): the quotient
 * and the rounding of ym_map_add_scans, the offset subtracted afterwards, exactly -- a reading keeps its lattice cell wherever the
 * window lies.  The world origin of the window is ax + x0 * res, ay + y0 * res, computed as written from the anchor and the whole offset
 * (the library is built with -ffp-contract=off), never step by step: ym_map_add_scans accepts exactly that value on a counted map.
 *   ym_map_create_counted_window  ym_map_create_counted with a window offset: the yardstick of a reframe, and how a saved map is
 *                        restored.  ym_map_create_counted is its (0, 0) case.
 *   ym_map_window        the window of any map.
 *   ym_map_reframe       makes new cell (i, j) the old cell (i + dx, j + dy) in a window of width x height cells.  Counted maps:
 *                        held[i] at held_poses[i] are ALL the scans the map holds, at the poses they were added at (the convention of
 *                        ym_map_update_scans' remove_poses).  Afterwards grid, bytes and counts are bit for bit those of a fresh
 *                        ym_map_create_counted_window map with the same anchor, the new window and the same scans: a reading the
 *                        old window dropped and the new one contains is stamped now, a reading that left the window takes its count
 *                        with it, and a cell near a side that moved gains or loses the taps of stamped cells beyond that side.  The
 *                        kept cells are copied, the held scans' readings outside the old window are stamped, and only the cells
 *                        whose tap neighbourhood meets the two windows differently are recomputed from the counts.  Uncounted maps
 *                        (n_held must be 0) keep no scans and no origin: the overlap keeps its values, every other cell is zero, the
 *                        caller moves its origin, and what border cells would have received from readings dropped earlier is lost.
 *                        Transactional: the new window is built in memory of its own and traded in when it is complete; a call
 *                        that is refused or fails, allocation included, leaves the map as it was.  The check on the held list: the
 *                        counts of the kept cells must sum to the held readings that fall there; if not, stats->mismatch is their
 *                        difference, the call returns YM_ERR_INVALID and nothing is changed.  (The check counts; it does not compare
 *                        cell by cell.)  The identity (dx = dy = 0, the same size) does nothing and reports kept = width * height.
 *                        Runs on the matcher's stream, synchronous, never throws.  A ym_locator made before does not see it.
 * YM_ERR_INVALID: a null argument, a negative n_held, a size <= 0 or above 10^9 cells, an accumulated offset beyond +-2^30, a held
 * list on an uncounted map, a null scan, a scan or a map on another device, a mismatch.  YM_ERR_UNSUPPORTED: a matcher that is not
 * YM_SEM_YAGPY, on a counted map taps too wide for the recompute's LDS tile (ym_map_update_scans' limit). */
typedef struct ym_map_reframe_stats {
    int64_t kept;        /* cells copied from the old window */
    int64_t restamped;   /* readings of held scans the old window dropped and the new one holds */
    int64_t dropped;     /* readings of held scans outside the new window */
    int64_t recomputed;  /* cells recomputed from the counts */
    int64_t mismatch;    /* |sum of kept counts - held readings inside the overlap|; non-zero: nothing was changed */
    int32_t x0, y0, width, height; /* the window after the call */
} ym_map_reframe_stats;
int ym_map_reframe(ym_matcher *m, ym_map *map, int dx, int dy, int width, int height,
                   const ym_scan *const *held, const double *held_poses /* [n_held][3], the poses they were added at */,
                   int n_held, ym_map_reframe_stats *stats /* or null */);
int ym_map_window(const ym_map *map, int *x0, int *y0, int *width, int *height);
ym_map *ym_map_create_counted_window(ym_matcher *m, int width, int height, double ax, double ay, int x0, int y0);
/* ---- maps that notice change: which held readings do newer scans look straight through?
 *   ym_map_seen_through  held[i] at held_poses[i] -- the poses they were added at, ym_map_update_scans' convention; any subset of
 *                        what the map holds -- are counted against the viewers at their CURRENT poses.  Cells are the map's own
 *                        (rint((x - ax) / res) - x0, likewise y; a quotient that is not finite or does not fit an int32 yields no
 *                        cell), readings are valid by !(r > range_threshold || isnan(r)).  Every valid viewer reading gives a ray from
 *                        the viewer's sensor cell to the reading's cell (either may lie outside the window; a viewer without a sensor
 *                        cell walks no ray), over the cells of Grid::TraceLine: axes swapped if steep, walked from the lower major
 *                        coordinate, the minor coordinate floor((2 k dm + dM) / (2 dM)) cells on after k of dM major steps.  A cell
 *                        of the window is SWEPT when its distance to the reading's end of the walk (dM - k, or k where the walk
 *                        started there) is greater than `clearance` -- clearance 0 sweeps all but the end cell -- unless it lies
 *                        within Chebyshev distance `protect` of the end cell of ANY valid viewer reading (protect 0: the end cells
 *                        themselves).  A ray of 32768 major steps or more sweeps nothing (only a reading no sensor gives is that
 *                        long once the matcher is admitted, below).  counts[i] = (inside, seen): held[i]'s valid readings whose
 *                        cell lies in the window, and those of them whose cell is swept; flags (or null) [n_held][max_n], max_n the
 *                        longest held scan: 1 exactly for the readings counted in seen, 0 elsewhere; mask (or null, a test hook)
 *                        [height][width]: the swept cells after protection; stats (or null): the viewer rays and the sums of
 *                        both counts.  A viewer may be held: no special case.  Changes no byte of the map or its counts.  Runs on
 *                        the matcher's stream, synchronous, never throws.  n_held == 0 or n_viewers == 0 are fine (nothing swept).
 * YM_ERR_INVALID: a null argument that is not nullable, a negative count, clearance or protect, a null scan, a scan or a map on
 * another device.  YM_ERR_UNSUPPORTED: a map that is not counted, a matcher that is not YM_SEM_YAGPY or whose
 * range_threshold / resolution + 2 reaches 32768 cells (the walk is 32-bit), a protect neighbourhood times the longest viewer
 * beyond 2 * 10^9 lanes. */
typedef struct ym_map_seen_stats { int64_t rays; int64_t inside; int64_t seen; } ym_map_seen_stats;
int ym_map_seen_through(ym_matcher *m, const ym_map *map,
                        const ym_scan *const *held, const double *held_poses /* [n_held][3] */, int n_held,
                        const ym_scan *const *viewers, int n_viewers, int clearance, int protect,
                        int32_t *counts /* [n_held][2]: inside, seen */,
                        uint8_t *flags /* nullable, [n_held][max_n], max_n = the longest held scan */,
                        uint8_t *mask /* nullable test hook, [height][width]: the swept cells after protection */,
                        ym_map_seen_stats *stats /* nullable */);
/* one find_best_pose_non_symmetric pass (/root/reference/yag_slam/helpers.py:434-573) */
typedef struct ym_map_search {
    double xy_search, xy_step;       /* +- metres around the centre, lattice step */
    double angle_search, angle_step; /* +- radians, step */
    double grid_resolution;          /* cell size the pass uses for indexing the map and in the penalty */
    int32_t penalize;
    int32_t reserved;
} ym_map_search;
/* The query scans' point readings (at their own poses) are matched as ONE point set against the map whose cell (0, 0)
 * is at world (ox, oy): coarse pass around the mean of the query poses (coarse == NULL: the reference's constants
 * 0.25 m / 0.01 m / 0.1 rad / 0.01 rad, cell size 0.05, no penalty -- scan_matching.py:152-153), then, if refine, the fine
 * pass +-2 cells, +-0.01745 rad at 0.00349 with the matcher's resolution and `penalize`.  out->pose is the corrected
 * mean pose (x, y, heading); the caller moves every query by its difference to the uncorrected mean. */
int ym_match_map(ym_matcher *m, const ym_map *map, double ox, double oy, const ym_scan *const *queries, int n_queries,
                 int penalize, int refine, const ym_map_search *coarse, ym_result *out);

/* ---- localization mode: scans matched against a resident map without a graph.
 *   ym_match_map_many   stands for n_items separate Scan2DMatcherPy.match_scan_sets_with_map calls on one map
 *                       (/root/reference/yag_slam/scan_matching.py:124-173) in one enqueue and one wait: item i is the query set
 *                       queries[set_offsets[i] .. set_offsets[i+1]) (1 to 64 scans; sets may differ in size and point count), and
 *                       results[i] is byte for byte the ym_result of ym_match_map on that set alone -- response, pose, covariance,
 *                       coarse_response, dims, hypotheses, n_query_points, status.  An item whose status is not 0 (no query point,
 *                       empty lattice) leaves its neighbours alone.  The integer sums of both passes come from yag_map_kernel for
 *                       lattices up to 64 positions per axis and from the pair-by-pair kernel for wider ones (ym_debug_counters
 *                       [6], [7]).  The scratch of the call is bounded (256 MiB of volumes: 268 items with the reference's constants);
 *                       more items run as consecutive chunks inside the call, and no result depends on the chunk length (debug
 *                       option 47 forces it).  Uses the matcher's synchronous slot and stream; YM_SEM_YAGPY only; never throws.
 *   ym_map_track        stands for the loop a localization-only node runs per incoming scan -- the odometry prior of
 *                       GraphSlam.process_scan (/root/reference/yag_slam/graph_slam.py:320-324), then match_scan_sets_with_map([scan])
 *                       -- for n_tracks scan streams in lock-step.  Track r is scans[track_offsets[r] .. track_offsets[r+1]); odom
 *                       holds 3 doubles per scan, parallel to `scans`; the scans before `start` (>= 1) of a track carry their poses.
 *                       Step i of all tracks that still have a scan i is ONE ym_match_map_many enqueue of single-scan items.  Per
 *                       item: prior = pose[i-1] (+) ((-)odom[i-1] (+) odom[i]) with transform.py's operations on the host, the scan's
 *                       pose is set to it and the set {scan i} is matched (its centre is the prior's position).  status != 0: the track
 *                       ends, n_done[r] = i, the scan keeps the prior, the other tracks go on.  response < min_response: the scan keeps
 *                       the prior and results[..].reserved = 1 (status stays 0).  Otherwise the pose becomes (R.x, R.y, prior.heading
 *                       + R.heading): the rigid motion of a one-scan set about its own position.  results is parallel to `scans`
 *                       (entries of scans that are not matched are zeroed); n_done[r] = the track's length when it ran to its end.
 *                       Bit-identical to that loop made of ym_scan_set_pose and ym_match_map calls. */
int ym_match_map_many(ym_matcher *m, const ym_map *map, double ox, double oy, const ym_scan *const *queries,
                      const int32_t *set_offsets, int n_items, int penalize, int refine, const ym_map_search *coarse,
                      ym_result *results);
int ym_map_track(ym_matcher *m, const ym_map *map, double ox, double oy, ym_scan *const *scans, const double *odom,
                 const int32_t *track_offsets, int n_tracks, int start, int penalize, int refine, const ym_map_search *coarse,
                 double min_response, ym_result *results, int32_t *n_done);

/* ---- scan sets against chains: Scan2DMatcherPy.match_scan_sets (yag_slam/scan_matching.py:56-122; DESIGN.md
 * section 18).  The point readings of the query scans, at their own poses, are matched as ONE point set against the grid built from
 * the base scans.
 *   ym_match_sets       the centre is the mean of the query positions (Python's left-to-right sum / count), heading 0; the grid is the
 *                       reference's G x G cells, G = int(search_size / res + 1 + 2 range_threshold / res), its corner (G - 1) / 2 cells
 *                       below the centre; every point reading of every base scan (r <= the scan's threshold, not NaN) passes
 *                       validate_points with the position of the LAST query scan as view-point (the loop variable the reference leaves
 *                       behind at :72-80), is rounded half to even to its cell and max-stamped with the smear kernel, stamps and taps
 *                       outside the grid dropped; a base scan with fewer than two point readings contributes nothing.  Coarse pass:
 *                       the symmetric find_best_pose around the centre with search_size / 2, 2 res, coarse_search_angle_offset / 2,
 *                       coarse_angle_resolution and `penalize`, the penalty centred on the grid's centre; if `refine` the fine pass
 *                       around its result (+-2 res at res, +-0.01745 rad at 0.00349).  out->pose is the corrected centre (x, y,
 *                       heading), out->cov the coarse pass's xx, yy, xy and the fine pass's th (4 coarse_angle_resolution without it);
 *                       the caller moves the queries (the reference returns diff (+) query pose, diff = corrected centre (-) centre).
 *                       Query scans without a point reading add no point, but count in the mean and as the view-point; a set without
 *                       any point has out->status != 0.
 *   ym_match_sets_many  n_items such calls in one enqueue and one wait: item i is the set queries[set_offsets[i] .. set_offsets[i+1])
 *                       against the chain base[chain_offsets[i] .. chain_offsets[i+1]); results[i] is byte for byte the ym_result of
 *                       ym_match_sets on that item alone, and an item whose status is not 0 leaves its neighbours alone.  A launch
 *                       serves every item of a chunk; the scratch is bounded (512 MiB of grids, 256 MiB of volumes), more items run
 *                       as consecutive chunks inside the call and no result depends on the chunk length (debug option 48 forces it).
 *                       The integer sums of both passes come from yag_map_kernel -- one rounding per (point, lattice column or row)
 *                       -- for lattices up to 64 positions per axis and from the pair-by-pair kernel for wider ones or when debug
 *                       option 46 is 0 (ym_debug_counters [8], [9]).
 * Both use the matcher's synchronous slot and stream and never throw; the matcher's windows, point cache and pair lists are neither
 * read nor written.  After either, ym_debug_sums (dense [nt][ny][nx] with the item's own dims, as ym_debug_map_sums),
 * ym_debug_grid / ym_debug_grid_info (the G x G bytes of an item of the last chunk) and ym_debug_query_local (the set's points
 * relative to its centre) describe the call's items.
 * YM_ERR_INVALID: a null argument, n_items outside [1, 2^20], a negative offset or chain length, an empty set or one of more than 64
 * scans, a null scan, a scan on another device.  YM_ERR_UNSUPPORTED: a matcher that is not YM_SEM_YAGPY (Karto has no such call), a
 * scan of more than 6000 readings, a grid of more than 10^9 cells.  A refused call changes nothing. */
int ym_match_sets(ym_matcher *m, const ym_scan *const *queries, int n_queries, const ym_scan *const *base, int n_base,
                  int penalize, int refine, ym_result *out);
int ym_match_sets_many(ym_matcher *m, const ym_scan *const *queries, const int32_t *set_offsets, const ym_scan *const *base,
                       const int32_t *chain_offsets, int n_items, int penalize, int refine, ym_result *results);

/* ---- occupancy-grid rendering: karto_scanmatcher.create_occupancy_grid(scans, resolution, range_threshold)
 * (/root/reference/yag_slam/graph_slam.py:341-342, /root/reference/ros1/slam_node_ros1:187-202).  Every scan is ray-traced
 * from its pose (open_karto OccupancyGrid::CreateFromScans): cells count passes and end-point hits, a cell passed more
 * than twice is occupied when hits / passes > 0.1, else free.  image[y][x] uses the codes the ROS node reads: 0 occupied,
 * 200 unknown, 255 free; row 0 is the lowest y; cell (0, 0) is at world (offset_x, offset_y).  Parity unpinned (the
 * wheel's source is not in the reference tree).
 *   ym_occupancy_create_counted    (test hook: the same rendering by the same launches, and the handle also keeps a host copy
 *                                  of the two count arrays the image is decided from, which ym_occupancy_create frees unread)
 *   ym_occupancy_read_counts       (test hook: pass[height][width] = how often a ray crossed or ended in the cell, the valid
 *                                  end point counted twice; hits[height][width] = valid end points in it.  `cells` is the
 *                                  length of each array.  On a handle of ym_occupancy_create, or with cells < width * height,
 *                                  it fails and writes nothing.) */
typedef struct ym_occupancy ym_occupancy;
typedef struct ym_occupancy_info {
    int32_t width, height;
    double offset_x, offset_y, resolution;
} ym_occupancy_info;
ym_occupancy *ym_occupancy_create(const ym_scan *const *scans, int n_scans, double resolution, double range_threshold);
ym_occupancy *ym_occupancy_create_counted(const ym_scan *const *scans, int n_scans, double resolution, double range_threshold);
int ym_occupancy_get_info(const ym_occupancy *og, ym_occupancy_info *info);
int ym_occupancy_read(const ym_occupancy *og, uint8_t *image, int64_t image_bytes); /* width*height bytes */
int ym_occupancy_read_counts(const ym_occupancy *og, uint32_t *pass, uint32_t *hits, int64_t cells);
void ym_occupancy_destroy(ym_occupancy *og);

/* ---- the map the ROS node publishes: the rendered grid with its specks removed (ros1/slam_node_ros1:187-212, _make_map).
 * The filter, all integer: fg = (image == foreground); the components of fg under `connectivity` (8:
 * coordinates differ by at most 1 in both axes, cv2's default and the node's; 4: cells that share an edge); every cell of a
 * component of fewer than min_area cells becomes `fill`.  The node's loop also visits cv2's label 0, the background: with B =
 * the cells != foreground, 0 < B < min_area turns every one of them into `fill` too (background_filled = 1).  Every other
 * cell is unchanged; the result is not examined again.  foreground and fill in 0 .. 255, min_area >= 0, connectivity 4 or 8:
 * anything else is YM_ERR_INVALID before any launch.  width * height above 2^31 - 1: YM_ERR_UNSUPPORTED.  The output is the
 * same from run to run.  Parity: the rules are the node's by definition; cv2's labelling itself is unpinned (only areas are used).
 *   ym_image_despeckle                replaces slam_node_ros1:191-197 (static_only, cv2.connectedComponentsWithStats, the loop
 *                                     over its statistics) for any byte image; `pitch` bytes between rows; opts null: the
 *                                     node's 0 / 255 / 5 / 8.  `out` and `stats` are written only when the call succeeds.
 *   ym_occupancy_create_clean         replaces slam_node_ros1:188-197: the three launches of ym_occupancy_create, then the filter
 *                                     on the device image, then the single copy to the host.  ym_occupancy_get_info and
 *                                     ym_occupancy_read serve its handle like any other.
 *   ym_occupancy_get_despeckle_stats  what that filter counted (the node keeps no such figures; it replaces nothing of
 *                                     slam_node_ros1 and is there for logs and tests).  Fails on a handle of the other creators.
 * cleared_cells counts foreground cells only; the background rule's cells are background_cells when background_filled. */
typedef struct ym_despeckle_opts { int32_t foreground, fill, min_area, connectivity; } ym_despeckle_opts;
typedef struct ym_despeckle_stats { int64_t foreground_cells, components, removed_components, cleared_cells, background_cells;
                                    int32_t background_filled, reserved; } ym_despeckle_stats;
int ym_image_despeckle(int device, const uint8_t *image, int width, int height, int pitch,
                       const ym_despeckle_opts *opts, uint8_t *out /* width*height */, ym_despeckle_stats *stats /* may be null */);
ym_occupancy *ym_occupancy_create_clean(const ym_scan *const *scans, int n_scans, double resolution, double range_threshold,
                                        const ym_despeckle_opts *opts /* null: the node's 0 / 255 / 5 / 8 */);
int ym_occupancy_get_despeckle_stats(const ym_occupancy *og, ym_despeckle_stats *stats); /* fails on a handle of the other creators */

/* ---- the live occupancy grid: the counts of that rendering kept on the device and changed by exactly the rays that changed
 * (DESIGN.md section 14).  A publish then costs the new scans' rays plus threshold, filter and copy of the image, not the log.
 * The lattice: an ANCHOR fixed once (given at creation, or the bounding-box minimum of the first add) and never moved; a world
 * coordinate's cell is Round((p - anchor) / resolution).  The WINDOW is what is reported: per axis origin = Round((min - anchor) /
 * resolution) and size = Round((max - min) / resolution) of the running bounding box of everything ever added; cell (0, 0) of
 * every read is lattice cell (origin_x, origin_y), at world offset = anchor + origin * resolution.  With the anchor at the offset
 * of ym_occupancy_create's grid of the same scans, width, height, offset, counts and image are that grid's, bit for bit, in
 * whatever order and batches the scans were added.  The memory holds every cell a ray of an added scan can touch, also outside
 * today's window (rays clipped at the range threshold leave it), plus slack_cells on every side whenever it has to grow.
 *   ym_occmap_accumulate   adds (sign +1) or subtracts (sign -1) the rays of n scans traced at poses[n][3] (x, y, heading), or at
 *                          the scans' own poses when poses is null.  The library keeps no membership: a caller subtracts what it
 *                          added, at the pose it added it at.  Subtraction never shrinks window or memory.
 *   ym_occmap_clear        zero counts, no bounding box; the anchor and the memory stay.
 *   ym_occmap_read         the window's image [height][width] (codes as above), through the component filter when clean is not
 *                          null (stats, nullable, then receives its figures).  bytes must be width * height.
 *   ym_occmap_read_counts  the window's pass and hit counts, cells = width * height each.
 *   ym_occmap_debug_option development: option 1 = the form of the trace kernel, 0 a wave per ray (default), 1 a thread per ray.
 * Refused with YM_ERR_INVALID: null or foreign-device scans, n <= 0, a sign other than +-1, a subtraction or a read before any
 * add (or after a clear), sizes that are not the window's.  YM_ERR_UNSUPPORTED: a window without width or height on a read (adds
 * to it are fine), more than 2 * 10^9 cells, more than 2^31 - 1 where the filter runs, range_threshold / resolution >= 2^24,
 * coordinates more than 2^30 cells from the anchor.  Every entry is synchronous. */
typedef struct ym_occmap ym_occmap;
typedef struct ym_occmap_info {
    int32_t width, height;                  /* the window */
    double offset_x, offset_y, resolution;  /* offset = anchor + origin * resolution */
    double anchor_x, anchor_y;
    int32_t origin_x, origin_y;             /* the window's first cell in the anchor's lattice */
    int32_t alloc_width, alloc_height;      /* cells that have memory ... */
    int32_t alloc_origin_x, alloc_origin_y; /* ... from this lattice cell on */
    int64_t reallocations;                  /* times the counts moved into a larger buffer (the first allocation is not one) */
    int32_t has_anchor, added;              /* the anchor is decided; something was added since creation or the last clear */
} ym_occmap_info;
ym_occmap *ym_occmap_create(int device, double resolution, double range_threshold,
                            const double *anchor_xy /* null: the first add decides */, int slack_cells);
int ym_occmap_accumulate(ym_occmap *om, const ym_scan *const *scans, const double *poses /* [n][3] or null */, int n, int sign);
int ym_occmap_clear(ym_occmap *om);
int ym_occmap_get_info(const ym_occmap *om, ym_occmap_info *info);
int ym_occmap_read(ym_occmap *om, uint8_t *image, int64_t bytes, const ym_despeckle_opts *clean /* or null */,
                   ym_despeckle_stats *stats /* or null */);
int ym_occmap_read_counts(ym_occmap *om, uint32_t *pass, uint32_t *hits, int64_t cells);
int ym_occmap_debug_option(ym_occmap *om, int option, int value);
void ym_occmap_destroy(ym_occmap *om);

/* ---- virtual scans from an occupancy image: the ray casting of the ROS node's "start in a prior map" path
 * (ingest_base_map -> map_to_graphslam -> map_to_graph, /root/reference/ros1/slam_node_ros1:131-147,
 * /root/reference/yag_slam/splicing.py:82-107).  ym_raymap_trace is run_raytracing_sweep (raytracing.py:91-92) for
 * n_starts viewpoints at once: every (viewpoint, angle) pair walks trace_ray (raytracing.py:63-88) -- pixel units, x = column,
 * y = row of `image`, float32 point, one pixel per step, stop at a pixel < 210 (one more step after it, a 1000-pixel jump
 * after a pixel in (180, 210)) or when the rounded point leaves [1, w - 1) x [1, h - 1) -- bit for bit.  starts_xy =
 * n_starts (x, y) float64 (rounded to float32 as Point2 does; the rounded pixel must lie inside the image), dir_cs = n_angles
 * unit (cos, sin) pairs computed by the caller (no trig on the device).  end_xy[n_starts][n_angles][2] receives the end
 * points (RayInfo.end), length[n_starts][n_angles] |end - start| (RayInfo.length), *capped (nullable) the number of rays
 * that reached the iteration cap 2 (w + h) + 4 (0 on every valid input).  Images up to 65536 x 65536 pixels.  Synchronous;
 * n_starts or n_angles 0 returns YM_OK without a launch; on an invalid argument nothing is written. */
typedef struct ym_raymap ym_raymap; /* an occupancy image resident on one device */
ym_raymap *ym_raymap_create(int device, const uint8_t *image, int width, int height, int pitch);
int ym_raymap_trace(ym_raymap *rm, const double *starts_xy, int n_starts, const double *dir_cs, int n_angles, float *end_xy,
                    double *length, int64_t *capped);
/* the same walk with a direction table per viewpoint: dir_cs = [n_starts][n_angles] (cos, sin) -- a scan per pose hypothesis,
 * each cast along its own heading + beam angles, in one launch */
int ym_raymap_trace_each(ym_raymap *rm, const double *starts_xy, int n_starts, const double *dir_cs, int n_angles, float *end_xy,
                         double *length, int64_t *capped);
void ym_raymap_destroy(ym_raymap *rm);

/* ---- locate a scan set anywhere in a prebuilt map: the exact best hypotheses over the whole map and all headings, by
 * branch and bound over a max pyramid of the map (no counterpart in the reference, whose node is told
 * its initial pose).  YM_SEM_YAGPY matchers only.
 * Definition.  g8 = the map's byte grid (0 .. 100), W x H, cell (cx, cy) centred at world (ox + cx res, oy + cy res), res = the
 * matcher's resolution.  The point set is ym_match_map's: the valid point readings of all query scans at their own poses minus
 * the mean query position, heading 0; point_stride s keeps points 0, s, 2s, ...; nq = the number kept (1 .. 65536).  For
 * heading k with (c, s) = dir_cs[k] and point P: r = (P.x c - P.y s, P.y c + P.x s), d = (rint(r.x / res), rint(r.y / res)),
 * every |d| <= 32767 or the call fails with YM_ERR_UNSUPPORTED.  S(k, cx, cy) = sum over the points of
 * g8[cy + d.y][cx + d.x], a read outside the map counting 0, for cx in [0, W), cy in [0, H); response = S / (100 nq).
 * The call returns the top_k hypotheses with S >= ceil(min_response * 100 * nq), ordered by S descending, ties by ascending
 * index = (k H + cy) W + cx, and how many there are (fewer than top_k may exist) -- exactly this list whatever `levels`,
 * max_nodes or the launch order are.  pose = (ox + cx res, oy + cy res, atan2(sin_k, cos_k)): the set's centre.
 *   ym_locator_create    builds the pyramid (levels 0 .. L of window maxima over 2^j x 2^j cells, with their low-side margins) and
 *                        allocates the two frontier buffers of max_nodes entries (8 bytes each).  levels < 0: the largest L with
 *                        2^L <= min(W, H) / 4, at most 6.  An explicit L > 8, or one whose top-level node is wider than the map's short
 *                        side (2^L > min(W, H)), is REFUSED with YM_ERR_INVALID, not clamped.  max_nodes <= 0: 2^25; at most 2^30.  The
 *                        top-level nodes are searched in chunks: as many, in (k, Y, X) order, as can be fully expanded within
 *                        max_nodes entries; if a single one cannot, create fails with YM_ERR_INVALID before anything is launched.
 *                        Maps up to 65536 cells per axis.  The handle copies the map's bytes (the map may be destroyed) and uses the
 *                        matcher's stream and resolution (the matcher must outlive it).
 *   ym_locator_get_info  width, height, levels, max_nodes, device bytes held
 *   ym_locator_read_level (test hook) level `level` of the pyramid over [0, W) x [0, H), n >= W H bytes
 *   ym_locator_locate    opts null: top_k 16, point_stride 1, min_response 0.  out holds top_k entries; points_out (nullable)
 *                        receives the nq points the search used; stats (nullable) nq, the number of chunks, and per level the
 *                        nodes the exact pass scored and those that survived (at level 0: the leaves passed to the top-K merge),
 *                        and the nodes the probes scored besides.
 *                        n_angles * W * H must stay below 2^40 (YM_ERR_UNSUPPORTED).  Synchronous; never throws.
 *                        YM_ERR_INVALID: a null argument, n_queries outside [1, 64], a query that is null or on another device,
 *                        n_angles outside [1, 65536], top_k outside [1, 64], point_stride < 1 or no valid reading, min_response < 0.
 *                        On an error nothing is written.
 *   ym_locator_locate_places  the n_places best DISTINCT places (1 .. 16) under the same definition, point set, offsets, S, floor
 *                        ceil(min_response * 100 * nq) and total order.  Hypothesis (k, x, y) is NEAR a pick (k', x', y') iff
 *                        (x - x')^2 + (y - y')^2 <= sep_cells2 AND dk <= sep_headings, dk = |k - k'| and, with circular = 1,
 *                        dk = min(dk, n_angles - dk) (integers only).  Place 1 is the best hypothesis; place i + 1 the best one
 *                        that is near none of places 1 .. i; the list ends after n_places entries or when no hypothesis is left
 *                        -- exactly this list whatever `levels`, max_nodes or the launch order are.  Both separations 0: the
 *                        top n_places of ym_locator_locate.  n_places = 1: its top 1.  Every place is a search of its own
 *                        (branch and bound with top_k = 1 and the picks so far excluded), which is why n_places stops at 16.
 *                        out holds n_places entries; points_out as above; stats (nullable): nq, rounds = searches run (the places
 *                        found, + 1 if the last search found none), chunks, nodes the exact passes and the probes scored, summed
 *                        over the rounds and per round (round_nodes[i] = exact-pass + probe nodes of round i), and the leaves
 *                        (level 0) and nodes (above) the exact passes dropped unscored because all they cover is near a pick.
 *                        Checks, limits and codes are ym_locator_locate's; YM_ERR_INVALID besides: opts null, n_places outside
 *                        [1, 16], sep_cells2 < 0, sep_headings < 0, circular not 0 or 1.  On an error nothing is written. */
typedef struct ym_locator ym_locator;
typedef struct ym_locator_info {
    int32_t width, height, levels, reserved;
    int64_t max_nodes, bytes;
} ym_locator_info;
typedef struct ym_locate_opts {
    int32_t top_k, point_stride;
    double min_response;
} ym_locate_opts;
typedef struct ym_locate_candidate {
    int32_t score;          /* S */
    int32_t k, cx, cy;      /* heading index, cell */
    int64_t index;          /* (k H + cy) W + cx */
    double response;        /* S / (100 nq) */
    double pose[3];         /* world pose of the set's centre */
} ym_locate_candidate;
typedef struct ym_locate_stats {
    int32_t nq, chunks;
    int64_t nodes[9];       /* scored per level (index = level) */
    int64_t survivors[9];   /* of those, not pruned */
    int64_t probe_nodes;    /* scored besides, by the probes that raise the threshold before each chunk's exact pass */
} ym_locate_stats;
ym_locator *ym_locator_create(ym_matcher *m, const ym_map *map, int levels, int64_t max_nodes);
int ym_locator_get_info(const ym_locator *lc, ym_locator_info *info);
int ym_locator_read_level(const ym_locator *lc, int level, uint8_t *out, int64_t n);
int ym_locator_locate(ym_locator *lc, double ox, double oy, const ym_scan *const *queries, int n_queries, const double *dir_cs,
                      int n_angles, const ym_locate_opts *opts, ym_locate_candidate *out, int *n_found, double *points_out,
                      ym_locate_stats *stats);
typedef struct ym_locate_places_opts {
    int32_t n_places, point_stride;      /* 1 .. 16; >= 1 */
    double  min_response;                /* >= 0 */
    int64_t sep_cells2;                  /* >= 0 */
    int32_t sep_headings, circular;      /* >= 0; 0 or 1 */
} ym_locate_places_opts;
typedef struct ym_locate_places_stats {
    int32_t nq, rounds;                  /* rounds = searches run (places found, + 1 if the last found none) */
    int64_t chunks, nodes, probe_nodes;  /* summed over the rounds */
    int64_t excluded_leaves, excluded_nodes;
    int64_t round_nodes[16];             /* exact-pass + probe nodes scored in each round */
} ym_locate_places_stats;
int ym_locator_locate_places(ym_locator *lc, double ox, double oy, const ym_scan *const *queries, int n_queries, const double *dir_cs,
                             int n_angles, const ym_locate_places_opts *opts /* not null */, ym_locate_candidate *out /* n_places entries */,
                             int *n_found, double *points_out, ym_locate_places_stats *stats);
void ym_locator_destroy(ym_locator *lc);

/* ---- the segment graph of a prior map from its label image: the rest of map_to_graph (yag_slam/splicing.py:57-80 of the
 * reference).  `labels` is the segmentation of the map (segment_map's output: the caller's, or ym_segments_from_map's below), int32
 * [height][pitch_elems], x = column, y = row, 0 = no segment, 1 .. K = segments; 1 x 1 up to 65536 x 65536 pixels.
 * ym_segments_create uploads it and finds the smallest and largest label (ym_segments_label_range returns them).
 * ym_segments_stats replaces determine_centroids' per-segment image scans: count / sum_x / sum_y [n_labels], indexed by
 * LABEL (0 included), exact 64-bit integers; the centroid of label l is (sum_x[l] / count[l], sum_y[l] / count[l]) in
 * float64, bit for bit np.mean of the coordinate arrays.  Every label must lie in [0, n_labels): otherwise YM_ERR_INVALID.
 * ym_segments_boundaries writes skimage.segmentation.find_boundaries(labels) (defaults: connectivity 1, mode "thick") as
 * width * height bytes 0 / 1 -- restated from that library's documented behaviour: a pixel whose label differs from the
 * maximum or minimum over itself and its 4 neighbours inside the image; label 0 takes part like any other.
 * ym_segments_pairs replaces create_edges' loop over the boundary pixels: for a boundary pixel (y, x), y >= 2 and x >= 2,
 * whose window of rows y-2 .. y+1 and columns x-2 .. x+1 (clipped at the image) holds exactly two distinct non-zero labels
 * a < b, the pair (a - 1, b - 1) is counted.  It returns every counted pair, its count and the raster index y * width + x
 * of the first pixel that counted it, sorted by that index (the reference's dict order); an edge of the graph is a pair
 * with count > 3.  table_slots sizes the device hash table the pairs are counted in (0: sized by the library); a table
 * that turns out too small is counted again in a larger one, beyond 2^26 slots the call fails with YM_ERR_UNSUPPORTED -- a
 * pair is never dropped.  cap = the pairs the caller's arrays hold: with more pairs than that the call fails with
 * YM_ERR_INVALID and *n_pairs = the number needed, nothing else written.  A negative label fails with YM_ERR_INVALID.
 * Synchronous, on the handle's own stream; outputs are written only after the whole call succeeded. */
typedef struct ym_segments ym_segments; /* a label image resident on one device */
ym_segments *ym_segments_create(int device, const int32_t *labels, int width, int height, int pitch_elems);
int ym_segments_label_range(const ym_segments *sg, int32_t *min_label, int32_t *max_label);
int ym_segments_stats(ym_segments *sg, int n_labels, int64_t *count, int64_t *sum_x, int64_t *sum_y);
int ym_segments_boundaries(ym_segments *sg, uint8_t *mask, int64_t mask_bytes);
int ym_segments_pairs(ym_segments *sg, int table_slots, int cap, int32_t *pairs /* [cap][2] */, int32_t *counts, int64_t *first_index,
                      int32_t *n_pairs);
void ym_segments_destroy(ym_segments *sg);

/* ---- the map segmenter: a prior map's image to its label image on the device, the reference's segment_map
 * (yag_slam/splicing.py:32-55) without OpenCV or scikit-image.  `image` is uint8 [h][pitch bytes], x = column, y = row,
 * 1 x 1 up to 65536 x 65536 pixels.  The pre-processing is the reference's, bit for bit by definition: a[a < 254] = 0,
 * t = 255 - a, grey dilation then erosion of t with a close_size x close_size square (odd, 1 .. 31; pixels outside the image
 * take no part, OpenCV's default border for morphology), closed = 255 - t.  ym_map_free_space returns `closed` (w * h
 * bytes), its exact sum and its count of non-zero ("free") pixels.  The superpixel step is NOT scikit-image's SLIC (whose
 * masked initialisation draws random samples and whose connectivity pass is a sequential flood fill): PARITY with it is
 * UNPINNED, the rules are this library's own ("Map segmenter") and are pinned by tests/segmenter_ref.py.
 * Inside the mask the reference's image is constant and its compactness 0.01, so its SLIC is essentially spatial k-means on
 * the free pixels; that is what is defined:
 *   n_segments = int(sum // 600000 * density) unless opts->n_segments > 0; step = max(1, int(sqrt(n_free / n_segments) + 0.5));
 *   cells of step x step pixels anchored at pixel (0, 0); a cell at least a quarter free (4 count >= step^2) seeds a centre
 *   at the mean of its free pixels, centres numbered in raster order of cells; `iterations` Lloyd passes (fewer when a
 *   pass changes no pixel): a free pixel takes the nearest (dx^2 + dy^2 in fp64, ties to the lowest index) of the centres
 *   seeded in the 5 x 5 cells around its own, none if there is none; then every centre with pixels moves to their mean;
 *   every 4-connected component of equal assignment with at least min_size = (n_free // n_segments) // min_size_div pixels
 *   is a segment, numbered 1 .. K by its first pixel in raster order; smaller components become 0 -- a free pixel may end
 *   up in no segment.
 * ym_segments_from_map returns the label image resident as a ym_segments (stats, boundaries and pairs run on it in place;
 * ym_segments_labels reads it, w * h labels).  opts null: n_segments 0, density 1, close_size 11, iterations 10,
 * min_size_div 4, stage FINAL.  stage ASSIGNED leaves centre index + 1 of every pixel as the label image (the state before
 * the components: a test hook; info->segments is 0 and info->unlabelled -1 then).  info (nullable) receives the scalars above;
 * min_size saturates at 2^31 - 1, unlabelled = free pixels with label 0.  Errors (null handle or YM_ERR_INVALID, the text
 * names the argument): a null image, w or h out of range, pitch < w, close_size even or out of range, n_segments that
 * comes out below 1, no free pixel, no seeded cell; YM_ERR_UNSUPPORTED when the cells make more than 2^31 - 1 blocks.
 * Synchronous; outputs are written only after the whole call has succeeded. */
#define YM_SEGMENT_STAGE_FINAL 0
#define YM_SEGMENT_STAGE_ASSIGNED 1
typedef struct ym_segment_opts { int32_t n_segments /* 0: the 600000 rule */; double density; int32_t close_size, iterations, min_size_div, stage; } ym_segment_opts;
typedef struct ym_segment_info { int64_t sum, n_free; int32_t n_segments, step, seeds, segments, iterations_run, min_size; int64_t unlabelled; } ym_segment_info;
int ym_map_free_space(int device, const uint8_t *image, int w, int h, int pitch, int close_size, uint8_t *closed, int64_t *sum,
                      int64_t *n_free);
ym_segments *ym_segments_from_map(int device, const uint8_t *image, int w, int h, int pitch, const ym_segment_opts *opts,
                                  ym_segment_info *info);
int ym_segments_labels(ym_segments *sg, int32_t *labels, int64_t n);

/* ---- the pose graph and its optimiser: what the reference hands to the third-party sba_cpp.SPA2d (graph_slam.py:64,
 * 132-192, 262-272), in fp64 on one device.  The formulation is that of Konolige et al., "Efficient Sparse Pose Adjustment
 * for 2D Mapping" (2010); sba_cpp itself is not available to this project, so PARITY with it is UNPINNED: the semantics
 * are this library's own ("Pose-graph optimiser") and are pinned by tests/posegraph_ref.py.
 * Node i has a pose (x, y, theta); node 0 is held fixed.  A constraint a -> b with mean (zx, zy, ztheta) and information L
 * (3 x 3 row-major, stored as (L + L^T) / 2) has the residual e_xy = R(theta_a)^T (t_b - t_a) - z_xy, e_theta =
 * wrap(theta_b - theta_a - ztheta) into (-pi, pi]; chi2 = sum e^T L e.
 *   ym_graph_create / _destroy     SPA2d() and its destruction
 *   ym_graph_add_nodes             SPA2d.add_node(x, y, yaw, num), n at a time; num is the running count
 *   ym_graph_add_constraints       SPA2d.add_constraint(a, b, x, y, yaw, info), n at a time
 *   ym_graph_get_poses / _size     SPA2d.nodes (x, y, yaw of every node) and its length
 *   ym_graph_set_poses             (no SPA2d call: re-seeds poses, e.g. to replay an optimisation)
 *   ym_graph_chi2                  (no SPA2d call: chi2 at the current poses, over the enabled constraints; see ym_graph_cost)
 *   ym_graph_linearise             (test hook: chi2, the diagonal blocks of H = J^T L J and the gradient J^T L e, undamped,
 *                                  node 0 included)
 *   ym_graph_solve                 (test hook: ONE damped solve at the current poses, which do not change.  It linearises,
 *                                  assembles (H + lambda diag H) with node 0 held and the band chosen as ym_graph_optimize
 *                                  chooses it, and runs the solve once: delta3 = x, the conjugate-gradient iterate;
 *                                  precond3 (may be NULL) = z, the last application of the preconditioner.  max_cg_iters
 *                                  = 0 runs no iteration: x = 0 and z = band(A, band)^-1 b exactly, the factor and both
 *                                  substitutions alone.  flags: 1 converged, 2 a pivot was not positive, 4 breakdown;
 *                                  residual: |r| / |b| of the recursively updated r.  Fewer than two nodes or no constraint:
 *                                  zeros.  The arguments are checked as ym_graph_optimize checks them, the cap from 0.)
 *   ym_graph_optimize              SPA2d.compute(iters, lambda, use_csparse, init_tol, max_cg_iters): Levenberg-Marquardt on
 *                                  (H + lambda diag H) delta = -g; a step that lowers chi2 is kept and lambda halves (not
 *                                  below 1e-12), otherwise the poses stay and lambda doubles.  It stops after `iters` steps
 *                                  (status 0), when a kept step gains no more than 1e-9 chi2 (1), when chi2 <= 1e-18 of the
 *                                  initial chi2 (2), when lambda > 1e10 (3).  Each step is solved by conjugate gradients
 *                                  preconditioned with the Cholesky factor of the block band |i - j| <= band of the system
 *                                  (band -1: the largest |a - b| among the constraints with |a - b| <= 16; 0: block-Jacobi).
 *                                  exact != 0 (use_csparse): relative residual 1e-10, at most min(9 N, 20000) iterations,
 *                                  cg_tol and max_cg_iters ignored; else those two.  A solve that reaches its cap still
 *                                  yields a step, which is kept or not by the same rule.
 *   ym_graph_hold / _held          (no SPA2d call: the held set.)  Every node is held or free; node 0 is always held and cannot
 *                                  be released; a node is free when added.  ym_graph_hold holds (hold = 1) or releases (0) the
 *                                  n nodes given; a node that is in that state already stays so.  ym_graph_held writes 1 per
 *                                  held node into mask[n_nodes], n_nodes the graph's node count.  The set may change between
 *                                  calls; the next launch sees the new set.
 * The held set.  One step solves (H + lambda diag H) delta = -g over the FREE nodes; H, g and diag H are summed over all
 * constraints.  A constraint between a free and a held node adds its own diagonal block and gradient to the free node and
 * nothing else; one between two held nodes adds only its chi2 term, a constant that ym_graph_chi2, the report and the stop
 * rules count.  delta of a held node is exactly 0 and its pose after ym_graph_optimize is bit for bit the pose before (theta
 * is not wrapped); ym_graph_set_poses may still move it.  Solve order: slot 0 stands for the held nodes (identity row,
 * right-hand side zero), the free nodes take the slots 1 .. F in index order; with only node 0 held slot(i) = i.  The band
 * lives in slots: the block (a, b) is in the band iff both nodes are free and |slot(a) - slot(b)| <= band; band -1 picks the
 * largest |slot(a) - slot(b)| <= 16 among the constraints whose ends are free or node 0, 0 if there is none, and
 * ym_opt_report.band and band_used report it.  (A constraint at node 0 has no block in the band; it counts because it always
 * did, so that a graph with nothing else held picks the band it picked before.  One at any other held node does not count.)  The iteration cap of exact solves stays min(9 N, 20000), N the node count.  No free node, or no
 * constraint with a free end: ym_graph_optimize succeeds with zero steps (chi2_initial = chi2_final = the constant) and
 * ym_graph_solve returns zeros.  A free component without a held node behaves as a component not connected to node 0: the
 * damping keeps it definite.  ym_graph_linearise returns diag and grad of every node, held ones included; ym_graph_solve
 * returns [N][3] arrays whose rows of held nodes are zero.  The held set is not part of a map file: re-hold after loading.
 * Errors (ym_last_error): a node index out of range, a constraint from a node to itself, a value that is not finite, an
 * information matrix without a positive diagonal, a release of node 0 (ym_graph_hold applies nothing of a call it refuses).
 * Fewer than two nodes or no constraint: ym_graph_optimize succeeds with zero steps.  The adds, ym_graph_hold / _held and
 * ym_graph_size / _get_poses / _set_poses touch no device.  Synchronous, on the handle's stream. */
typedef struct ym_graph ym_graph;
ym_graph *ym_graph_create(int device);
void ym_graph_destroy(ym_graph *g);
int ym_graph_add_nodes(ym_graph *g, const double *xyt, int n); /* appended; index = running count */
int ym_graph_add_constraints(ym_graph *g, const int32_t *from_to, const double *mean_xyt, const double *info9, int n);
int ym_graph_size(const ym_graph *g, int32_t *nodes, int32_t *constraints);
int ym_graph_set_poses(ym_graph *g, int first, const double *xyt, int n);
int ym_graph_get_poses(const ym_graph *g, int first, double *xyt, int n);
int ym_graph_hold(ym_graph *g, const int32_t *nodes, int n, int hold /* 1: hold, 0: release */);
int ym_graph_held(const ym_graph *g, uint8_t *mask, int n_nodes); /* 1 per held node */
int ym_graph_chi2(ym_graph *g, double *chi2);
int ym_graph_linearise(ym_graph *g, double *chi2, double *diag9 /* [N][9] */, double *grad3 /* [N][3] */);
int ym_graph_solve(ym_graph *g, int band /* -1 auto, 0 .. 16 */, double lambda, double cg_tol, int max_cg_iters /* >= 0 */,
                   double *delta3 /* [N][3] */, double *precond3 /* [N][3], may be NULL */, int32_t *band_used,
                   int32_t *cg_iterations, double *residual, int32_t *flags);
typedef struct ym_opt_params { int32_t iters, exact, max_cg_iters, band /* -1 auto */; double lambda0, cg_tol; } ym_opt_params;
typedef struct ym_opt_report { double chi2_initial, chi2_final, lambda_final; int32_t lm_steps, accepted, cg_iterations, band, status; } ym_opt_report;
int ym_graph_optimize(ym_graph *g, const ym_opt_params *p, ym_opt_report *out);

/* Robust kernels and switchable constraints.  A constraint's index is its place in the order of
 * ym_graph_add_constraints.  Each has a kind, a parameter p > 0 and an enabled flag; it is YM_ROBUST_NONE and enabled when
 * added.  With s = e^T L e its cost term is rho(s) and its weight w(s) = rho'(s):
 *   YM_ROBUST_NONE            rho = s                                       w = 1
 *   YM_ROBUST_HUBER (k)       rho = s if s <= k^2, else 2 k sqrt(s) - k^2   w = 1 if s <= k^2, else k / sqrt(s)
 *   YM_ROBUST_CAUCHY (c)      rho = c^2 log1p(s / c^2)                      w = 1 / (1 + s / c^2)
 *   YM_ROBUST_GEMAN_MCCLURE   rho = c^2 s / (c^2 + s)                       w = (c^2 / (c^2 + s))^2
 *   disabled (any kind)       rho = 0                                       w = 0
 * The objective is F = sum rho.  A step of ym_graph_optimize linearises with H = sum w J^T L J and g = sum w J^T L e, the
 * weights taken at the current poses (first-order re-weighting, no second-order term), and every rule that speaks of chi2 --
 * keep or reject, the gain stop, the 1e-18 stop -- uses F; ym_opt_report.chi2_initial and chi2_final hold F.  ym_graph_linearise
 * returns F and the weighted blocks and gradient, ym_graph_solve solves the weighted system.  A graph whose constraints are
 * all YM_ROBUST_NONE and enabled gets, bit for bit, what it got before there were kinds (w = 1.0, rho = s).
 *   ym_graph_set_robust    the kind and parameter of the n constraints given (the parameter is stored for YM_ROBUST_NONE too)
 *   ym_graph_enable        enables (enable = 1) or disables (0) the n constraints given.  Disabling is refused if it would
 *                          leave a free node without an enabled constraint (its block would be singular); a node held at the
 *                          time of the call is not checked, and a later release of it is the caller's business
 *   ym_graph_edge_terms    s[M] and w[M] at the current poses; s of a disabled constraint is still its e^T L e, its w is 0
 *   ym_graph_cost          F at the current poses.  ym_graph_chi2 stays the plain sum of s over the enabled constraints
 * Errors: a constraint index out of range, a kind that is none of the four, a parameter that is not finite and positive, the
 * refused disable.  A call that fails applies nothing.  ym_graph_set_robust and ym_graph_enable touch no device. */
enum { YM_ROBUST_NONE = 0, YM_ROBUST_HUBER = 1, YM_ROBUST_CAUCHY = 2, YM_ROBUST_GEMAN_MCCLURE = 3 };
int ym_graph_set_robust(ym_graph *g, const int32_t *edges, int n, int kind, double param);
int ym_graph_enable(ym_graph *g, const int32_t *edges, int n, int enable /* 1: enable, 0: disable */);
int ym_graph_edge_terms(ym_graph *g, double *s /* [M] */, double *w /* [M] */);
int ym_graph_cost(ym_graph *g, double *cost);

/* ---- introspection for parity tests (state of the LAST completed synchronous match) ---- */
typedef struct ym_grid_info {
    int32_t width, height, pitch; /* device window (bytes) */
    int32_t origin_x, origin_y;   /* window cell (0,0) in Karto storage coordinates (incl. border) */
    int32_t storage_w, storage_h; /* Karto's full storage size the window is cut from */
    int32_t roi_x, roi_y, roi_w, roi_h;
    double offset_x, offset_y;    /* world coordinate of ROI cell (0,0) */
} ym_grid_info;
int ym_debug_grid_info(ym_matcher *m, int item, ym_grid_info *info);
int ym_debug_grid(ym_matcher *m, int item, uint8_t *out, int64_t out_bytes); /* height*pitch bytes */
/* integer correlation sums [itheta][iy][ix] of pass 0 (coarse) / 1 (fine) */
int ym_debug_sums(ym_matcher *m, int item, int pass, uint32_t *out, int64_t out_count);
/* test hook: the same of item `item` of the last MAP call (ym_match_map_many; ym_match_map: item 0), dense with the item's own nx,
 * ny, nt: out_count >= nx ny nt.  A call of more than 128 items keeps the sums of its last chunk only. */
int ym_debug_map_sums(ym_matcher *m, int item, int pass, uint32_t *out, int64_t out_count);
/* query points in the sensor frame (xy interleaved), returns count via *n */
int ym_debug_query_local(ym_matcher *m, int item, double *out_xy, int32_t cap, int32_t *n);
/* window cell coordinates of the rasterised base points of `item`, per base scan slot:
 * out[(slot*max_n + i)*2 + {0,1}] = wx, wy  or (INT32_MIN, INT32_MIN) for filtered points */
int ym_debug_cells(ym_matcher *m, int item, int32_t *out, int64_t out_count, int32_t *max_n);
/* the region correlate's pair lists of query slot `slot` of the last call, as bin_kernel left them ("The pair-list
 * contract"), with the geometry they were built for and what the builder read of the slot's representative item `qrep`.
 * YM_ERR_INVALID: the last call built no such lists (its correlate was not correlate_region_kernel), or no such slot.
 * Lists reused from an earlier call (option 45) are read like freshly built ones.  With all five arrays NULL only *info is filled (the sizes to allocate); otherwise all five
 * are written, and nothing is written when the call fails:
 *   ctrig   [nt][2]                 cos, sin of qrep's coarse angles
 *   starts  [lparts][nbins + 1]     first entry of bin region * lnw + (angle - part * lnw), positions in `entries`
 *   flags   [lparts]                padded total of the part, or -1: the part has no list (its entries are unspecified)
 *   entries [lparts][entries_pstride]
 *   rbox    [nregions][lparts]      rmin | rmax << 8 | xmin << 16 | xmax << 24 of the patch origins inside the region */
typedef struct ym_pair_list_info {
    int32_t nt, lnw, lparts, nbins;  /* coarse angles; angles per list part, parts; bins per part = nregions * lnw */
    int32_t nrx, nry, nregions;      /* regions along x and y of class space */
    int32_t rg_h, rg_cls, rg_zero;   /* class rows per region, LDS bytes per class image, LDS offset of the all-zero patch */
    int32_t ng;                      /* sets of 16-bit sums per (item, angle) */
    int32_t qrep, cx0, cy0, nq;      /* the item that stands for the slot; its first hypothesis cell; its valid readings */
    int32_t n_slots;                 /* query slots of the call */
    int64_t entries_pstride;         /* entries a part has room for */
    double off_x, off_y;             /* qrep's grid offset */
    double ylat[2];                  /* qrep's lattice origin ("yagpy" semantics: the addends of the lookup cells) */
} ym_pair_list_info;
int ym_debug_pair_lists(ym_matcher *m, int slot, ym_pair_list_info *info, double *ctrig, int32_t *starts, int32_t *flags,
                        uint16_t *entries, uint32_t *rbox);

/* test hook: what find_best_pose pass `pass` (0 coarse, 1 fine) of item `item` of the last synchronous YM_SEM_YAGPY call computed with --
 * the last call being a chain call (ym_match_scans, ym_match_batch, ym_match_pairs; kind 0), a map call (ym_match_map,
 * ym_match_map_many, ym_map_track; kind 1) or a set call (ym_match_sets, ym_match_sets_many; kind 2).  With it the rule
 * np.round(((xvals[i] + r) - o) / res) can be restated on the host from the device's own operands (tests/yag_ties_ref.py): everything
 * after the cosines, the sines and the points is IEEE arithmetic.  It reads only and changes no result.  With the three arrays NULL
 * only *info is filled (the sizes to allocate); otherwise all three are written, and nothing is written when the call fails:
 *   axes    [nx + ny + nt]  xvals, yvals, tvals: numpy.arange's values as the device computes them, computed again from the item's state
 *   trig    [nt][2]         cos, sin of tvals[k] as the kernels of the pass take them (the same functions on the same operand)
 *   points  [nq][2]         the item's point set: sensor-frame readings (kind 0), the world readings moved by the set's centre (1, 2) */
typedef struct ym_yag_frame {
    int32_t kind, pass;
    int32_t nx, ny, nt, nq;
    int32_t grid_w, grid_h;          /* the grid of the rule's bounds test: cells (0 .. grid_w, 0 .. grid_h) count */
    int32_t roi_w;                   /* the matcher's grid side G (the lattice guard's M = |ox| + |oy| + 2 G res) */
    int32_t win_origin, win_w, pitch; /* the device window inside that grid (kind 0; the whole grid otherwise) and its row pitch */
    int32_t lat_nx, lat_ny, lat_nt;  /* kind 0, pass 0: the lattice the production correlate kernels were launched on (0: they were not) */
    int32_t step_cells;              /* ... and its step in cells */
    int32_t regular;                 /* kind 0: the lattice proof's decision for the item */
    int32_t map_split;               /* kinds 1, 2: blocks that shared an (item, angle) of the coarse pass */
    double ox, oy, res;              /* the corner and the cell size the pass indexed with */
    double search_xy, step_xy, search_t, step_t; /* find_best_pose's arguments */
    double centre[3];                /* ... and its search centre */
} ym_yag_frame;
int ym_debug_yag_frame(ym_matcher *m, int item, int pass, ym_yag_frame *info, double *axes, double *trig, double *points);

/* Switches of the parity tests: every row names a path the tests force so that each kernel and each host decision is compared with
 * the oracle (or with the default path) bit for bit.  None changes a result.  Development and timing switches that no test uses
 * (2 - 5, 9, 23, 26, 29, 34, 36, 38, 40, 42) are described where they are implemented, yag_slam_amd/csrc/ym_abi_debug.hpp.
 *
 *   option  value                          effect
 *   ------  -----------------------------  ------------------------------------------------------------------------------------------
 *    6      0 / 1 / 2                      finish stage: by batch size / fine + final kernels / the one-block finish kernel
 *    7      0 / 1 / 2                      point cache of resident base scans: on / off / drop every entry now
 *    8      KiB                            point cache limit (small values force the start-over path)
 *   10      1                              order-dependent smear rule always through the global-memory kernel
 *   11      256 / 1024 / 0                 threads per finish block (0 = by batch size)
 *   12      1                              keep the coarse integer sums for ym_debug_sums whatever the call (default: fewer than 8
 *                                          items on a lattice of at most 65536 hypotheses)
 *   13      0 / 1 / 2                      merging of consecutive beams with equal lookup offsets in the direct correlate: by grid
 *                                          coarseness / always / never
 *   14      0 / 1 / 2 / 3 / 4              coarse correlate of batches: region correlate on lattices up to 26 x 32 and gather correlate
 *                                          on others up to 48 x 64 / always the direct kernel / the LDS correlates' per-cell path / their
 *                                          "lists do not fit" path / the gather correlate also where the region correlate would run
 *   15      n                              waves per region-correlate block / angles per wave of the gather correlate
 *   16      n                              raster blocks per item on batches (0 = sized by the previous call's longest tile list)
 *   17      n                              blocks per item of the gather correlate (each takes a share of the angles)
 *   18      n / -1                         hit slots per entry of the raster's work list / no hit lists
 *   19      n                              units per LDS buffer of the gather correlate (small values cut regions into chunks)
 *   20      bytes                          LDS a gather block may use (small values make the regions small)
 *   21      2                              the region correlate leaves the scoring of its sums to the score kernel
 *   24      0                              trigger chains of base scans recomputed at every pose (not from the creation-time structure)
 *   25      tiles                          margin around the raster rectangle a device-chained step predicts (negative: every step faults)
 *   28      n / 0                          batch size from which BOTH LDS correlates replace the direct kernel (>= 8) / the defaults
 *                                          (gather correlate 64, region correlate 48)
 *   30      32 / 64 / 0                    rows per raster tile whatever the call / the host's choice
 *   31      0                              a synchronous match waits for the creation launch of a just-created query scan
 *   37      1                              the raster's row pass by bit scans instead of its tables
 *   39      1                              every call writes the column planes and the region correlate stages from them
 *   41      n                              items up to which the order-dependent smear rule runs in its split form (8; 0 = never)
 *   45      0                              the pair lists of a single-query batch are built at every call (default: a call whose query,
 *                                          pose, window and lattice equal those of the last list build finds them in place)
 *   46      0 / 2                          YM_SEM_YAGPY, 0: both passes scored pair by pair, the Python rule as written -- set calls too (default: the coarse
 *                                          pass's integer sums come from the production correlate kernels wherever the item's roundings
 *                                          provably form a lattice: ym_debug_counters; the fine pass's are taken row by row);
 *                                          2: the default, with the fine pass reading its rows byte by byte (the path of a row whose
 *                                          columns do not fit one 8-byte read)
 *   47      n / 0                          items per chunk of ym_match_map_many whatever its scratch budget says / by the budget
 *   48      n / 0                          items per chunk of ym_match_sets_many whatever its scratch budgets say / by the budgets
 *   49      1                              the angular covariance gathers the scan again at the mean pose's cell even where that cell
 *                                          is one of the fine lattice's and the fine pass's sums already hold the answer
 *
 * Options 0, 32, 33, 35, 43 and 44 chose between correlate forms that no longer exist: YM_ERR_INVALID, like any unknown option.
 */
int ym_debug_option(ym_matcher *m, int option, int value);

/* counters since ym_create, out[0 .. min(count, YM_DEBUG_COUNTERS)):
 *   [0] YM_SEM_YAGPY items whose coarse sums came from the production correlate kernels, [1] items that fell back to the pair-by-pair
 *   kernel (a rounding tie that falls differently along the lattice, a read outside the device window, an np.arange longer than the launch
 *   lattice), [2] (point, angle) pairs that needed the hypothesis-by-hypothesis check, [3] pairs that failed it;
 *   [4] single-query batches that found their pair lists in place (option 45);
 *   [5] the coarse correlate the LAST call launched: 0 correlate_kernel, 1 correlate_region_kernel, 2 gather_kernel, -1 none;
 *   [6] items of ym_match_map_many whose sums came from yag_map_kernel, [7] items it left to the pair-by-pair kernel (a coarse
 *   lattice of more than 64 positions on an axis);
 *   [8] items of ym_match_sets / ym_match_sets_many whose sums came from yag_map_kernel, [9] items left to the pair-by-pair kernel (a
 *   coarse lattice of more than 64 positions on an axis, or option 46 = 0) */
#define YM_DEBUG_COUNTERS 10
int ym_debug_counters(ym_matcher *m, int64_t *out, int32_t count);

/* test hook: the bytes of device memory and of pinned host memory that the library's handles hold right now, in this process (every
 * handle of every device; the scan pool's slabs, which outlive their scans on purpose, are not counted).  A handle that is created,
 * used and destroyed leaves both numbers exactly where they were. */
int ym_debug_live_bytes(int64_t *device_bytes, int64_t *pinned_bytes);

/* development aid: 100 MHz wall-clock stamps written by block 0 of each kernel at phase boundaries.
 * Reads the stamps of the last call into out[0..count) (count <= 32), then switches stamping on/off. */
int ym_debug_stamps(ym_matcher *m, int enable, uint64_t *out, int32_t count);

/* ---- profiling: HIP-event timing of the correlate kernel on the matcher's stream ---- */
int ym_profile_enable(ym_matcher *m, int on);
/* which: 0 = correlate (coarse), 1 = raster, 2 = whole call; returns accumulated ms and launch count */
int ym_profile_read(ym_matcher *m, int which, double *ms_total, int64_t *launches, int reset);
/* point cache of the matcher (what Karto's LocalizedRangeScan keeps in m_PointReadings until the pose is set again):
 * scans found current / scans (re)projected since the matcher was created */
int ym_cache_stats(const ym_matcher *m, int64_t *hits, int64_t *misses);

#ifdef __cplusplus
}
#endif
#endif /* YAGMATCH_H */
