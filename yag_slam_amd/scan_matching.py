"""Matcher plugin: drop-in for /root/reference/yag_slam/scan_matching.py:29-42 (Scan2DMatcherCpp).

`ScanMatcher(config_dict, loop).match_scan(query, base_scans, penalty, do_fine)` returns the
reference's `ScanMatcherResult(response, covariance, best_pose, meta)` namedtuple; `.config` is the
attribute bag yag-slam serialises (graph_slam.py:82-83).  All numerics run in libyagmatch.so on
the MI355X; this file only marshals scans and results across the ctypes boundary.
"""
import ctypes as C
import os
import struct
from collections import namedtuple

import numpy as np

from . import _capi
from .config import default_config, default_config_loop, make_config
from .models import LocalizedRangeScan
from .transform import Transform

ScanMatcherResult = namedtuple('ScanMatcherResult', ['response', 'covariance', 'best_pose', 'meta'])


def _pose_of(scan):
    p = scan.corrected_pose
    return float(p.x), float(p.y), float(p.euler[-1])


def _desc_of(scan, keep):
    """ym_scan_desc from any duck-typed LocalizedRangeScan (host ranges are uploaded per call)."""
    d = _capi.YmScanDesc()
    r = np.ascontiguousarray(scan.ranges, dtype=np.float64)
    keep.append(r)
    d.ranges = r.ctypes.data_as(C.POINTER(C.c_double))
    d.n = int(r.shape[0])
    d.min_angle = float(scan.min_angle)
    d.max_angle = float(getattr(scan, "max_angle", scan.min_angle + (d.n - 1) * scan.angle_increment))
    d.angle_increment = float(scan.angle_increment)
    d.min_range = float(scan.min_range)
    d.max_range = float(getattr(scan, "max_range", 0.0))
    d.range_threshold = float(scan.range_threshold)
    d.pose[0], d.pose[1], d.pose[2] = _pose_of(scan)
    return d


# one unpack of the whole ym_result instead of ~30 ctypes field reads (a few microseconds of a 60 us match)
_RESULT_STRUCT = struct.Struct("<d3d9ddq3i3i4i")
assert _RESULT_STRUCT.size == C.sizeof(_capi.YmResult)


def _result(r):
    v = _RESULT_STRUCT.unpack_from(r)
    meta = {
        "coarse_response": v[13], "hypotheses": v[14], "coarse_dims": v[15:18], "fine_dims": v[18:21],
        "n_query_points": v[21], "expansions": v[22], "status": v[23],
    }
    return ScanMatcherResult(v[0], [list(v[4:7]), list(v[7:10]), list(v[10:13])], Transform(v[1], v[2], 0.0, v[3]), meta)


# numpy view of an array of ym_result (include/yagmatch.h): converting a batch result field by field through ctypes
# costs ~8 us per chain, more than the GPU spends on it
_RESULT_DTYPE = np.dtype([("response", "<f8"), ("pose", "<f8", (3,)), ("cov", "<f8", (9,)), ("coarse_response", "<f8"),
                          ("hypotheses", "<i8"), ("coarse_dims", "<i4", (3,)), ("fine_dims", "<i4", (3,)),
                          ("n_query_points", "<i4"), ("expansions", "<i4"), ("status", "<i4"), ("reserved", "<i4")])
assert _RESULT_DTYPE.itemsize == C.sizeof(_capi.YmResult)


class BatchResults(object):
    """The per-chain results of a batch as a read-only sequence of ScanMatcherResult, built when an entry is looked at:
    a loop closure asks for the few chains above its thresholds, and 4096 result objects cost more Python time (4.5 ms)
    than the GPU spends on the 4096 matches.  `.array` is the numpy record view of the ym_result array
    (include/yagmatch.h): response, pose, cov, coarse_response, hypotheses, coarse_dims, fine_dims, n_query_points,
    expansions, status -- the form to filter and sort in."""

    __slots__ = ("array",)

    def __init__(self, array):
        self.array = array

    def __len__(self):
        return int(self.array.shape[0])

    def _one(self, i):
        r = self.array[i]
        p = r["pose"]
        return ScanMatcherResult(float(r["response"]), r["cov"].reshape(3, 3).tolist(), Transform(float(p[0]), float(p[1]), 0.0, float(p[2])),
                                 {"coarse_response": float(r["coarse_response"]), "hypotheses": int(r["hypotheses"]),
                                  "coarse_dims": tuple(r["coarse_dims"].tolist()), "fine_dims": tuple(r["fine_dims"].tolist()),
                                  "n_query_points": int(r["n_query_points"]), "expansions": int(r["expansions"]),
                                  "status": int(r["status"])})

    def __getitem__(self, i):
        if isinstance(i, slice):
            return [self._one(j) for j in range(*i.indices(len(self)))]
        n = len(self)
        if i < 0:
            i += n
        if not 0 <= i < n:
            raise IndexError("chain index out of range")
        return self._one(i)

    def __iter__(self):
        return (self._one(i) for i in range(len(self)))

    def best(self):
        """index of the chain with the highest response (the first of equals, like ym_batch_wait's best_chain)"""
        return int(np.argmax(self.array["response"])) if len(self) else -1


def _results(per, check=False):
    """BatchResults over a copy of a ctypes array of YmResult.  check: raise like match_scan does when any chain reports
    Karto's "unable to find best position / index out of range"."""
    a = np.frombuffer(per, dtype=_RESULT_DTYPE).copy()
    if check and a["status"].any():
        bad = int(np.flatnonzero(a["status"])[0])
        raise _capi.YmError(int(a["status"][bad]), "Mapper FATAL ERROR - unable to find best position / index out of range "
                            "(chain %d)" % bad)
    return BatchResults(a)


class ScanMatcher(object):
    """MI355X correlative scan matcher behind yag-slam's matcher plugin surface."""

    def __init__(self, config_dict=None, loop=False, semantics="karto", device=0):
        cfg = default_config if not loop else default_config_loop
        cfg = cfg.copy()
        if config_dict:
            cfg.update(config_dict)
        self.config = make_config(cfg)
        self.semantics = semantics
        self.device = int(device)
        self._lib = _capi.lib()
        self._cfg = _capi.config_struct(self.config, semantics)
        self._m = self._lib.ym_create(C.byref(self._cfg), self.device)
        if not self._m:
            raise _capi.YmError(-1, _capi.last_error())
        # development only, and only on request: YM_DEVELOPMENT=1 YM_DEBUG_OPTIONS="14=1,21=2" -> ym_debug_option on every
        # matcher of the process.  Without YM_DEVELOPMENT an inherited YM_DEBUG_OPTIONS changes nothing in a library user.
        if os.environ.get("YM_DEVELOPMENT") == "1":
            for kv in filter(None, (t.strip() for t in os.environ.get("YM_DEBUG_OPTIONS", "").split(","))):
                try:
                    k, v = (int(t) for t in kv.split("="))
                except ValueError:
                    raise ValueError("YM_DEBUG_OPTIONS: cannot read %r (expected option=value, both integers)" % kv)
                self.debug_option(k, v)

    def close(self):
        if getattr(self, "_m", None):
            self._lib.ym_destroy(self._m)
            self._m = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # ---- handles -------------------------------------------------------------------------
    def _native(self, scan):
        """ym_scan* of a resident scan (our LocalizedRangeScan), else None.  Like the reference's C++ twin
        (/root/reference/yag_slam/models.py:67-75) the device twin follows the pose through the `corrected_pose`
        setter, so nothing is re-sent here."""
        if isinstance(scan, LocalizedRangeScan):
            return scan.native(self.device)
        return None

    def _push_pose(self, scan):
        """re-send the current corrected pose (for poses mutated in place, behind the setter's back)"""
        h = self._native(scan)
        if h is not None:
            x, y, t = _pose_of(scan)
            _capi.check(self._lib.ym_scan_set_pose(h, x, y, t))

    # ---- the plugin call -------------------------------------------------------------------
    def match_scan(self, query, base_scans, penalty=True, do_fine=False):
        res = _capi.YmResult()
        dev = self.device
        handles = [s._native if (type(s) is LocalizedRangeScan and s._native is not None and s._native_device == dev)
                   else self._native(s) for s in (query, *base_scans)]
        if None not in handles:
            nb = len(handles) - 1
            arr = (C.c_void_p * max(1, nb))(*handles[1:])
            rc = self._lib.ym_match_scans(self._m, handles[0], arr, nb, 1 if penalty else 0, 1 if do_fine else 0, C.byref(res))
            if rc:
                _capi.check(rc)
        else:
            keep = []
            q = _desc_of(query, keep)
            b = (_capi.YmScanDesc * max(1, len(base_scans)))(*[_desc_of(s, keep) for s in base_scans])
            _capi.check(self._lib.ym_match(self._m, C.byref(q), b, len(base_scans), int(bool(penalty)),
                                           int(bool(do_fine)), C.byref(res)))
        if res.status != 0:
            raise _capi.YmError(res.status, "Mapper FATAL ERROR - unable to find best position / index out of range")
        return _result(res)

    def map_sequence(self, scans, start, buffer_len, penalty=True, do_fine=True, device_chain=False):
        """The matcher calls of `GraphSlam.process_scan` (/root/reference/yag_slam/graph_slam.py:320-337) for
        scans[start:], scans[:start] being the running chain so far: odometry prior from `odom_pose`, match against the
        last `buffer_len` scans, `corrected_pose` = the match's pose -- one library call (`ym_match_scans` in a host
        loop without Python).  Every scan must be resident (our LocalizedRangeScan).  Returns the results of
        scans[start:]; raises like `match_scan` at the first scan Karto would abort on (the scans before it are done).
        device_chain: no host round trip between the steps either (the device hands each step's pose to the next;
        include/yagmatch.h) -- the priors are then composed with the device's cos / sin, so poses agree with the
        step-by-step form to rounding, not bit for bit."""
        self.sequence_done = []  # (before anything can raise: a caller's except branch must not see the previous call's results)
        n = len(scans)
        handles = (C.c_void_p * max(1, n))(*[self._require_native(s) for s in scans])
        odom = np.empty((max(1, n), 3), dtype=np.float64)
        for i, s in enumerate(scans):
            p = s.odom_pose
            odom[i, 0], odom[i, 1], odom[i, 2] = p.x, p.y, p.euler[-1]
        per = (_capi.YmResult * max(1, n))()
        done = C.c_int32(0)
        rc = self._lib.ym_map_sequence(self._m, handles, odom.ctypes.data_as(C.POINTER(C.c_double)), n, int(start),
                                       int(buffer_len), int(bool(penalty)), int(bool(do_fine)), int(bool(device_chain)),
                                       per, C.byref(done))
        first = max(int(start), 1)
        res = _results(per)[first:done.value] if done.value > first else []
        for s, r in zip(scans[first:done.value], res):
            s._corrected_pose = r.best_pose  # (the device twin already has it)
        self.sequence_done = res  # (the scans matched before an error: SequentialMapper.process_scans commits them)
        if rc:  # (a library error: the scans matched so far keep their results, Python and device twins agree)
            _capi.check(rc)
        if done.value < n:
            bad = scans[done.value]
            pose = (C.c_double * 3)()
            _capi.check(self._lib.ym_scan_get_pose(bad._native, pose))
            bad._corrected_pose = Transform(pose[0], pose[1], 0.0, pose[2])  # the prior, where the per-scan path leaves it
            raise _capi.YmError(per[done.value].status, "Mapper FATAL ERROR - unable to find best position / index out of "
                                "range (scan %d of the sequence)" % done.value)
        return res

    def process_scan(self, query, chain, penalty=True, do_fine=True):
        """`GraphSlam.process_scan`'s matcher work for one scan in one library call (`ym_process_scan`): the odometry
        prior from `chain[-1]` and the two `odom_pose`s, the match, `query.corrected_pose` = the result.  Resident scans
        only (returns None otherwise: the caller does it the long way).  Same bits as the three separate steps."""
        dev = self.device
        scans = (query, *chain)
        for s in scans:
            if type(s) is not LocalizedRangeScan or s._native is None or s._native_device != dev:
                if not isinstance(s, LocalizedRangeScan):
                    return None
                s.native(dev)
        n = len(chain)
        arr = (C.c_void_p * n)(*[s._native for s in chain])
        lo, qo = chain[-1].odom_pose, query.odom_pose
        a = (C.c_double * 3)(lo.x, lo.y, lo.euler[-1])
        b = (C.c_double * 3)(qo.x, qo.y, qo.euler[-1])
        res = _capi.YmResult()
        rc = self._lib.ym_process_scan(self._m, query._native, arr, n, a, b, 1 if penalty else 0, 1 if do_fine else 0, C.byref(res))
        if rc:
            _capi.check(rc)
        pose = (C.c_double * 3)()
        if res.status != 0:
            _capi.check(self._lib.ym_scan_get_pose(query._native, pose))
            query._corrected_pose = Transform(pose[0], pose[1], 0.0, pose[2])  # (the prior, where the long way leaves it)
            raise _capi.YmError(res.status, "Mapper FATAL ERROR - unable to find best position / index out of range")
        r = _result(res)
        query._corrected_pose = r.best_pose  # (the device twin already has it)
        return r

    def sequence_stats(self):
        """(device-chained segments, segments cut short by a fault, synchronous steps) of map_sequence so far"""
        a, b, c = C.c_int64(0), C.c_int64(0), C.c_int64(0)
        _capi.check(self._lib.ym_sequence_stats(self._m, C.byref(a), C.byref(b), C.byref(c)))
        return int(a.value), int(b.value), int(c.value)

    def match_scan_batch(self, query, chains, penalty=False, do_fine=False):
        """One query against many candidate chains (the loop of graph_slam.py:217-236 in one call).
        Returns (per_chain_results, best_index)."""
        flat, offs = [], [0]
        for ch in chains:
            flat.extend(ch)
            offs.append(len(flat))
        hq = self._require_native(query)
        hs = (C.c_void_p * max(1, len(flat)))(*self._handles(flat))
        co = (C.c_int32 * len(offs))(*offs)
        per = (_capi.YmResult * len(chains))()
        best = _capi.YmResult()
        bi = C.c_int32(-1)
        _capi.check(self._lib.ym_match_batch(self._m, hq, hs, co, len(chains), int(bool(penalty)), int(bool(do_fine)),
                                             per, C.byref(best), C.byref(bi)))
        return _results(per, check=True), int(bi.value)

    def make_batch(self, query, chains):
        """Reusable (query, chains) batch for the pipelined loop-closure path."""
        return MatchBatch(self, query, chains)

    def match_pairs(self, queries, chains, penalty=True, do_fine=False):
        """len(queries) INDEPENDENT matches in one enqueue: item i = `match_scan(queries[i], chains[i], penalty, do_fine)`
        (N x /root/reference/yag_slam/graph_slam.py:326 -- N robots, or N segments of a log replayed side by side), item for
        item bit-identical to the single calls.  Returns the per-item results (BatchResults)."""
        if len(queries) != len(chains):
            raise ValueError("match_pairs needs one chain per query (%d queries, %d chains)" % (len(queries), len(chains)))
        if not queries:
            return BatchResults(np.zeros(0, dtype=_RESULT_DTYPE))
        flat, offs = [], [0]
        for ch in chains:
            flat.extend(ch)
            offs.append(len(flat))
        hq = (C.c_void_p * len(queries))(*self._handles(queries))
        hs = (C.c_void_p * max(1, len(flat)))(*self._handles(flat))
        co = (C.c_int32 * len(offs))(*offs)
        per = (_capi.YmResult * len(chains))()
        _capi.check(self._lib.ym_match_pairs(self._m, hq, hs, co, len(chains), int(bool(penalty)), int(bool(do_fine)), per))
        return _results(per, check=True)

    def make_pairs_batch(self, queries, chains):
        """Reusable form of `match_pairs` (resident on the device, runnable many times; poses are read at every run)."""
        return MatchBatch(self, queries, chains, pairs=True)

    def _handles(self, scans):
        """ym_scan* of every scan; the twins that already live on this device are taken without a call"""
        dev, out = self.device, []
        for s in scans:
            h = getattr(s, "_native", None)
            if h is None or getattr(s, "_native_device", None) != dev or not isinstance(s, LocalizedRangeScan):
                h = self._require_native(s)
            out.append(h)
        return out

    def _require_native(self, scan):
        h = self._native(scan)
        if h is None:
            raise TypeError("match_scan_batch needs yag_slam_amd.models.LocalizedRangeScan instances")
        return h

    # ---- one match split over several matchers by coarse angle (yag_slam_amd.dist.AngleSplitMatcher) -----------------
    def coarse_dims(self):
        """(nx, ny, ntheta) of the coarse lattice of this matcher's config"""
        d = (C.c_int32 * 3)()
        _capi.check(self._lib.ym_coarse_dims(self._m, d))
        return tuple(d[:])

    def slice_begin(self, query, base_scans, penalty, do_fine, k_begin, k_end, dev_resp, dev_probs):
        """Enqueue the match up to the score stage for coarse angles [k_begin, k_end); responses and per-(x, y) maxima go
        to the caller's device buffers (raw pointers).  No host wait."""
        hq = self._require_native(query)
        arr = (C.c_void_p * max(1, len(base_scans)))(*self._handles(base_scans))
        _capi.check(self._lib.ym_match_slice_begin(self._m, hq, arr, len(base_scans), int(bool(penalty)), int(bool(do_fine)),
                                                   int(k_begin), int(k_end), C.c_void_p(dev_resp), C.c_void_p(dev_probs)))

    def slice_finish(self):
        """The rest of the match on the completed volume; returns the ScanMatcherResult of the whole match."""
        res = _capi.YmResult()
        _capi.check(self._lib.ym_match_slice_finish(self._m, C.byref(res)))
        if res.status != 0:
            raise _capi.YmError(res.status, "Mapper FATAL ERROR - unable to find best position / index out of range")
        return _result(res)

    # ---- match against a prebuilt map (Scan2DMatcherPy.match_scan_sets_with_map, scan_matching.py:124-173) ------------
    def correlation_grid_from_occupancy(self, map_im, occupied_value=0):
        """Device counterpart of `occupancy_grid_map_to_correlation_grid(map_im, res, smear_deviation, occupied_value)`
        (/root/reference/yag_slam/helpers.py:24-34) with this matcher's resolution and smear: returns a resident
        CorrelationMap (`.to_numpy()` gives the float grid the reference function returns)."""
        im = np.ascontiguousarray(map_im, dtype=np.uint8)
        if im.ndim != 2:
            raise ValueError("occupancy image must be 2-D")
        h = self._lib.ym_map_from_occupancy(self._m, im.ctypes.data_as(C.POINTER(C.c_uint8)), im.shape[1], im.shape[0],
                                            im.strides[0], int(occupied_value))
        if not h:
            raise _capi.YmError(-1, _capi.last_error())
        return CorrelationMap(self, h)

    def upload_correlation_grid(self, cgrid):
        """A correlation grid computed elsewhere (2-D float array, 0..1) as a resident CorrelationMap."""
        g = np.ascontiguousarray(cgrid, dtype=np.float64)
        if g.ndim != 2:
            raise ValueError("correlation grid must be 2-D")
        h = self._lib.ym_map_from_grid(self._m, g.ctypes.data_as(C.POINTER(C.c_double)), g.shape[1], g.shape[0])
        if not h:
            raise _capi.YmError(-1, _capi.last_error())
        return CorrelationMap(self, h)

    def empty_correlation_map(self, width, height, counted=False, ox=None, oy=None, window=None):
        """A resident CorrelationMap of `height` x `width` zeros, to be filled with `CorrelationMap.add_scans`.
        counted=True (`ym_map_create_counted`): the map also counts the readings stamped in each cell, so that scans can be
        taken out again (`remove_scans`, `sync`); (ox, oy) is its anchor, the world position of cell (0, 0) of the lattice its
        window lies in, for good.  window=(x0, y0) (`ym_map_create_counted_window`): the map's cell (0, 0)
        is cell (x0, y0) of that lattice and its `origin` is anchor + offset * resolution; without it the window starts at the
        anchor.  `CorrelationMap.reframe` moves the window of either kind of map."""
        if not counted:
            if ox is not None or oy is not None or window is not None:
                raise ValueError("empty_correlation_map: only a counted map has an origin and a window offset of its own")
            h = self._lib.ym_map_create_empty(self._m, int(width), int(height))
        else:
            if ox is None or oy is None:
                raise ValueError("empty_correlation_map: a counted map needs its origin (ox, oy)")
            if window is None:
                h = self._lib.ym_map_create_counted(self._m, int(width), int(height), float(ox), float(oy))
            else:
                x0, y0 = (int(v) for v in window)
                h = self._lib.ym_map_create_counted_window(self._m, int(width), int(height), float(ox), float(oy), x0, y0)
        if not h:
            raise _capi.YmError(-1, _capi.last_error())
        return CorrelationMap(self, h, origin=(float(ox), float(oy)) if counted else None, offset=window or (0, 0))

    def match_scan_sets_with_map(self, cgrid, ox, oy, query_scans, penalty=True, do_fine=True, coarse=None):
        """The reference's signature (scan_matching.py:124): the point readings of all `query_scans` are matched as one
        set against the map `cgrid` (CorrelationMap or 2-D float array) whose cell (0, 0) lies at world (ox, oy).
        Returns ScanMatcherResult(response, covariance, [corrected pose of every query scan], meta).
        `coarse`: dict overriding the coarse pass the reference hard-codes (xy_search 0.25, xy_step 0.01,
        angle_search 0.1, angle_step 0.01, grid_resolution 0.05, penalize False)."""
        own = not isinstance(cgrid, CorrelationMap)
        mp = self.upload_correlation_grid(cgrid) if own else cgrid
        try:
            hs = (C.c_void_p * len(query_scans))(*[self._require_native(q) for q in query_scans])
            cs = None
            if coarse:
                cs = _capi.YmMapSearch(float(coarse.get("xy_search", 0.25)), float(coarse.get("xy_step", 0.01)),
                                       float(coarse.get("angle_search", 0.1)), float(coarse.get("angle_step", 0.01)),
                                       float(coarse.get("grid_resolution", 0.05)), int(bool(coarse.get("penalize", False))), 0)
            res = _capi.YmResult()
            _capi.check(self._lib.ym_match_map(self._m, mp._h, float(ox), float(oy), hs, len(query_scans), int(bool(penalty)),
                                               int(bool(do_fine)), C.byref(cs) if cs else None, C.byref(res)))
        finally:
            if own:
                mp.close()
        if res.status != 0:
            raise _capi.YmError(res.status, "empty search lattice or no query point")
        r = _result(res)
        # scan_matching.py:136-139,167-173: the search centre is the mean query position with heading 0; every query is
        # moved by (corrected centre - centre)
        xs = [float(q.corrected_pose.x) for q in query_scans]
        ys = [float(q.corrected_pose.y) for q in query_scans]
        oxy = Transform.from_position_euler(sum(xs) / float(len(xs)), sum(ys) / float(len(ys)), 0, 0, 0, 0)
        diff = r.best_pose - oxy
        r.meta["centre"] = (oxy.x, oxy.y, 0.0)
        r.meta["corrected_centre"] = (r.best_pose.x, r.best_pose.y, r.best_pose.euler[-1])
        return ScanMatcherResult(r.response, r.covariance, [q.corrected_pose + diff for q in query_scans], r.meta)

    # ---- localization mode: many sets against one map, scan streams followed through it --------
    @staticmethod
    def _map_search(coarse):
        if not coarse:
            return None
        return _capi.YmMapSearch(float(coarse.get("xy_search", 0.25)), float(coarse.get("xy_step", 0.01)),
                                 float(coarse.get("angle_search", 0.1)), float(coarse.get("angle_step", 0.01)),
                                 float(coarse.get("grid_resolution", 0.05)), int(bool(coarse.get("penalize", False))), 0)

    def match_map_batch(self, cmap, ox, oy, query_sets, penalty=True, do_fine=True, coarse=None, strict=True):
        """N independent `match_scan_sets_with_map` calls on one resident map in ONE enqueue (`ym_match_map_many`): item i
        matches the scans of `query_sets[i]` (1 to 64 scans; sets may differ) as one point set.  Returns a list of
        ScanMatcherResult, each built exactly as `match_scan_sets_with_map` builds its own for that set alone -- the same
        bits, the same meta keys ("centre", "corrected_centre", ...), best_pose = the wrapper's pose list -- plus
        meta["rigid_poses"]: the set moved rigidly about its centre (what `locate_in_map` returns).  An item the matcher cannot
        serve (no query point, empty lattice) raises as the single call does, or with strict=False is None in the list; its
        neighbours are unaffected.  Empty input or an empty set: ValueError before the library is touched."""
        sets = [list(s) for s in query_sets]
        if not sets:
            raise ValueError("match_map_batch: no query set")
        for i, s in enumerate(sets):
            if not s:
                raise ValueError("match_map_batch: query set %d is empty" % i)
        if not isinstance(cmap, CorrelationMap):
            raise TypeError("match_map_batch needs a resident CorrelationMap (correlation_grid_from_occupancy / upload_correlation_grid)")
        flat, offs = [], [0]
        for s in sets:
            flat.extend(s)
            offs.append(len(flat))
        hs = (C.c_void_p * len(flat))(*[self._require_native(q) for q in flat])
        co = (C.c_int32 * len(offs))(*offs)
        cs = self._map_search(coarse)
        per = (_capi.YmResult * len(sets))()
        _capi.check(self._lib.ym_match_map_many(self._m, cmap._h, float(ox), float(oy), hs, co, len(sets), int(bool(penalty)),
                                                int(bool(do_fine)), C.byref(cs) if cs else None, per))
        out = []
        for i, (s, res) in enumerate(zip(sets, per)):
            if res.status != 0:
                if strict:
                    raise _capi.YmError(res.status, "empty search lattice or no query point (item %d)" % i)
                out.append(None)
                continue
            out.append(_map_set_result(res, s))
        return out

    # ---- scan sets against chains ----------------------------------------------------------------
    def match_scan_sets(self, query_scans, base_scans, penalty=True, do_fine=True):
        """The reference's signature (scan_matching.py:56): the point readings of all `query_scans` (1 to 64) are matched as one
        set against the grid built from `base_scans` -- centred on the mean query position, filtered from the position of the
        LAST query scan, as the reference does.  Returns ScanMatcherResult(response, covariance, [pose of every query scan], meta);
        the poses are the reference's `diff + q.corrected_pose` (:121), which is not a rigid motion of the set:
        meta["rigid_poses"] is.  meta also holds "centre", "corrected_centre", "coarse_response", "coarse_dims", "fine_dims",
        "n_query_points".  `"yagpy"` matchers only; a set without a point reading raises YmError."""
        qs, bs = list(query_scans), list(base_scans)
        if not qs:
            raise ValueError("match_scan_sets: no query scan")
        hq = (C.c_void_p * len(qs))(*[self._require_native(q) for q in qs])
        hb = (C.c_void_p * max(1, len(bs)))(*[self._require_native(b) for b in bs])
        res = _capi.YmResult()
        _capi.check(self._lib.ym_match_sets(self._m, hq, len(qs), hb, len(bs), int(bool(penalty)), int(bool(do_fine)), C.byref(res)))
        if res.status != 0:
            raise _capi.YmError(res.status, "empty search lattice or no query point")
        return _scan_set_result(res, qs)

    def match_scan_sets_batch(self, query_sets, chains, penalty=True, do_fine=True, strict=True):
        """N independent `match_scan_sets` calls in ONE enqueue (`ym_match_sets_many`): item i matches the scans of
        `query_sets[i]` as one point set against `chains[i]`.  A single set -- a flat list of scans -- given with N chains is matched
        against each of them (the loop-closure use).  Returns a list of ScanMatcherResult, each built exactly as `match_scan_sets`
        builds its own for that item alone.  An item the matcher cannot serve (no query point, empty lattice) raises as the single
        call does, or with strict=False is None in the list; its neighbours are unaffected.  Empty input or an empty set:
        ValueError before the library is touched."""
        sets, chs = list(query_sets), [list(c) for c in chains]
        if not sets or not chs:
            raise ValueError("match_scan_sets_batch: no query set or no chain")
        if not isinstance(sets[0], (list, tuple)):
            sets = [sets] * len(chs)  # one set, broadcast over the chains
        else:
            sets = [list(s) for s in sets]
        if len(sets) != len(chs):
            raise ValueError("match_scan_sets_batch: %d query sets and %d chains" % (len(sets), len(chs)))
        for i, s in enumerate(sets):
            if not s:
                raise ValueError("match_scan_sets_batch: query set %d is empty" % i)
        fq, oq, fb, ob = [], [0], [], [0]
        for s, c in zip(sets, chs):
            fq.extend(s)
            oq.append(len(fq))
            fb.extend(c)
            ob.append(len(fb))
        hq = (C.c_void_p * len(fq))(*[self._require_native(q) for q in fq])
        hb = (C.c_void_p * max(1, len(fb)))(*[self._require_native(b) for b in fb])
        per = (_capi.YmResult * len(sets))()
        _capi.check(self._lib.ym_match_sets_many(self._m, hq, (C.c_int32 * len(oq))(*oq), hb, (C.c_int32 * len(ob))(*ob), len(sets),
                                                 int(bool(penalty)), int(bool(do_fine)), per))
        out = []
        for i, (s, res) in enumerate(zip(sets, per)):
            if res.status != 0:
                if strict:
                    raise _capi.YmError(res.status, "empty search lattice or no query point (item %d)" % i)
                out.append(None)
                continue
            out.append(_scan_set_result(res, s))
        return out

    def track_in_map(self, cmap, ox, oy, tracks, start=1, penalty=True, do_fine=True, coarse=None, min_response=0.0):
        """Follow scan streams through a resident map without growing a graph (`ym_map_track`).  `tracks`: a list of scans
        (one stream) or a list of such lists (streams in lock-step: step i of every track that still has a scan i is one
        enqueue).  Every scan carries `odom_pose`; the scans before `start` (>= 1) of a track carry their `corrected_pose`.
        Per scan: prior = previous corrected pose + odometry increment (graph_slam.py:320-324), the one-scan set is matched
        against the map, and `corrected_pose` becomes the set's rigid correction -- or stays the prior when the response is
        below `min_response` (meta["accepted"] False) or when the matcher cannot serve the scan, which ends its track.
        Returns per track (results, n_done): results[i] is None for the scans before `start` and from n_done on; a single
        stream given as a plain list returns its one pair."""
        tracks = list(tracks)
        single = bool(tracks) and not isinstance(tracks[0], (list, tuple))
        if single:
            tracks = [tracks]
        tracks = [list(t) for t in tracks]
        if not tracks:
            raise ValueError("track_in_map: no track")
        for r, t in enumerate(tracks):
            if not t:
                raise ValueError("track_in_map: track %d is empty" % r)
        if int(start) < 1:
            raise ValueError("track_in_map: start must be at least 1 (scan 0 of a track carries its pose)")
        if not isinstance(cmap, CorrelationMap):
            raise TypeError("track_in_map needs a resident CorrelationMap")
        flat, offs = [], [0]
        for t in tracks:
            flat.extend(t)
            offs.append(len(flat))
        n = len(flat)
        hs = (C.c_void_p * n)(*[self._require_native(s) for s in flat])
        odom = np.empty((n, 3), dtype=np.float64)
        for i, s in enumerate(flat):
            p = s.odom_pose
            odom[i, 0], odom[i, 1], odom[i, 2] = p.x, p.y, p.euler[-1]
        co = (C.c_int32 * len(offs))(*offs)
        cs = self._map_search(coarse)
        per = (_capi.YmResult * n)()
        done = (C.c_int32 * len(tracks))()
        rc = self._lib.ym_map_track(self._m, cmap._h, float(ox), float(oy), hs, odom.ctypes.data_as(C.POINTER(C.c_double)), co,
                                    len(tracks), int(start), int(bool(penalty)), int(bool(do_fine)), C.byref(cs) if cs else None,
                                    float(min_response), per, done)
        # (the device twins hold what the call left, whatever its outcome: the Python side follows them)
        pose = (C.c_double * 3)()
        out = []
        for r, t in enumerate(tracks):
            nd = int(done[r]) if rc == 0 else len(t)
            res = [None] * len(t)
            for i in range(int(start), len(t)):
                if i > nd:
                    break
                _capi.check(self._lib.ym_scan_get_pose(hs[offs[r] + i], pose))
                t[i]._corrected_pose = Transform(pose[0], pose[1], 0.0, pose[2])
                if i < nd and rc == 0:
                    one = per[offs[r] + i]
                    m_ = _result(one)
                    m_.meta["accepted"] = one.reserved == 0
                    res[i] = m_
            out.append((res, nd))
        if rc:
            _capi.check(rc)
        return out[0] if single else out

    # ---- locate a scan set anywhere in a map (ym_locator_*) -------------------------------------
    def map_locator(self, cmap, levels=None, max_nodes=None):
        """A MapLocator over the resident CorrelationMap `cmap`: its max pyramid and search buffers on the device.
        levels: pyramid levels above the map (None: by the map's size); max_nodes: frontier entries per buffer (None: 2^25)."""
        return MapLocator(self, cmap, levels, max_nodes)

    def locate_in_map(self, cmap, ox, oy, query_scans, refine=True, polish_top=1, places=None, min_separation=(1.0, 0.5), **kw):
        """One shot: where in the map `cmap` (cell (0, 0) at world (ox, oy)) were `query_scans` taken, as one rigid set?
        The exact best hypothesis over all cells and headings (`MapLocator.locate`, keywords passed on), then, with `refine`,
        polished: copies of the scans are moved to the located poses and matched with `match_scan_sets_with_map` (coarse
        window +-2 cells and +- one heading step, then its fine pass).  Returns a ScanMatcherResult whose best_pose holds one
        pose per query scan and whose meta["candidates"] is the located list.  The polish's correction is applied as a rigid
        motion about the set's centre (the wrapper's own list, which composes the correction in each scan's frame as the
        reference does, is meta["wrapper_poses"]).  Raises ValueError when no hypothesis reaches min_response.
        polish_top = K > 1: the first K located candidates are polished in one `match_map_batch`; the best polished response
        wins, a tie going to the earlier candidate, and all K polished results are meta["polished"] (best_pose of each: its
        rigid pose list).
        places = K (1 .. 16): the candidates are the K best distinct places (`MapLocator.locate_places` with
        `min_separation` = (metres, radians) and the keywords), not the top of one list.  With `refine`, all places found are
        polished in one `match_map_batch` and the best polished response wins, as with polish_top; meta["places"] holds the
        polished results in place order and meta["ambiguity"] the second-best polished response over the best (0.0 with one
        place): near 1, the map has another place that explains the scans as well."""
        with self.map_locator(cmap) as loc:
            if places is not None:
                cands = loc.locate_places(query_scans, ox, oy, n_places=int(places), min_separation=min_separation, **kw)
                polish_top = max(2, len(cands))  # every place found goes through the batch polish
            else:
                cands = loc.locate(query_scans, ox, oy, **kw)
            stats, step = loc.last_stats, loc.last_heading_step
        if not cands:
            raise ValueError("locate_in_map: no hypothesis reaches min_response = %g" % kw.get("min_response", 0.0))
        best = cands[0]
        meta = {"candidates": cands, "stats": stats}
        if not refine:
            return ScanMatcherResult(best.response, None, list(best.poses), meta)
        res = float(self.config.resolution)
        if int(polish_top) > 1:
            sets = []
            for cand in cands[:int(polish_top)]:
                moved = []
                for q, p in zip(query_scans, cand.poses):
                    c = q.copy()
                    c.corrected_pose = p
                    moved.append(c)
                sets.append(moved)
            rs = self.match_map_batch(cmap, ox, oy, sets, True, True,
                                      coarse=dict(xy_search=2 * res, xy_step=res / 4, angle_search=step, angle_step=step / 20,
                                                  grid_resolution=res))
            r = _pick_polished(rs, meta)
            if places is not None:
                ranked = sorted(p.response for p in rs)
                r.meta["places"] = r.meta["polished"]
                r.meta["ambiguity"] = float(ranked[-2] / ranked[-1]) if len(ranked) > 1 and ranked[-1] > 0 else 0.0
            return r
        moved = []
        for q, p in zip(query_scans, best.poses):
            c = q.copy()
            c.corrected_pose = p
            moved.append(c)
        r = self.match_scan_sets_with_map(cmap, ox, oy, moved, True, True,
                                          coarse=dict(xy_search=2 * res, xy_step=res / 4, angle_search=step, angle_step=step / 20,
                                                      grid_resolution=res))
        c0, c1 = r.meta["centre"], r.meta["corrected_centre"]
        meta.update(r.meta)
        meta["wrapper_poses"] = r.best_pose
        poses = _move_rigidly([m_.corrected_pose for m_ in moved], c0[0], c0[1], c1[0], c1[1], c1[2] - c0[2])
        return ScanMatcherResult(r.response, r.covariance, poses, meta)

    # ---- pipelined form ----------------------------------------------------------------------
    def match_scan_async(self, query, base_scans, penalty=True, do_fine=False, slot=0):
        hq = self._require_native(query)
        arr = (C.c_void_p * max(1, len(base_scans)))(*self._handles(base_scans))
        _capi.check(self._lib.ym_match_scans_async(self._m, hq, arr, len(base_scans), int(bool(penalty)),
                                                   int(bool(do_fine)), int(slot)))

    def wait(self, slot=0):
        res = _capi.YmResult()
        _capi.check(self._lib.ym_wait(self._m, int(slot), C.byref(res)))
        return _result(res)

    def synchronize(self):
        _capi.check(self._lib.ym_synchronize(self._m))

    def set_stream(self, stream_handle):
        """Run on a caller-owned HIP stream (e.g. torch.cuda.current_stream().cuda_stream); None = own."""
        _capi.check(self._lib.ym_set_stream(self._m, C.c_void_p(stream_handle) if stream_handle else None))

    # ---- introspection for the parity tests --------------------------------------------------
    def debug_grid(self, item=0):
        info = _capi.YmGridInfo()
        _capi.check(self._lib.ym_debug_grid_info(self._m, item, C.byref(info)))
        buf = np.zeros((info.height, info.pitch), dtype=np.uint8)
        _capi.check(self._lib.ym_debug_grid(self._m, item, buf.ctypes.data_as(C.POINTER(C.c_uint8)), buf.size))
        return buf[:, :info.width], info

    def debug_sums(self, pass_=0, item=0, dims=None):
        nx, ny, nt = dims
        buf = np.zeros((nt, ny, nx), dtype=np.uint32)
        _capi.check(self._lib.ym_debug_sums(self._m, item, pass_, buf.ctypes.data_as(C.POINTER(C.c_uint32)), buf.size))
        return buf

    def debug_map_sums(self, pass_=0, item=0, dims=None):
        """the [nt][ny][nx] integer sums of item `item` of the last map call (match_map_batch; match_scan_sets_with_map: item 0)"""
        nx, ny, nt = dims
        buf = np.zeros((nt, ny, nx), dtype=np.uint32)
        _capi.check(self._lib.ym_debug_map_sums(self._m, int(item), int(pass_), buf.ctypes.data_as(C.POINTER(C.c_uint32)), buf.size))
        return buf

    def debug_query_local(self, item=0, cap=8192):
        buf = np.zeros((cap, 2))
        n = C.c_int32()
        _capi.check(self._lib.ym_debug_query_local(self._m, item, buf.ctypes.data_as(C.POINTER(C.c_double)), cap,
                                                   C.byref(n)))
        return buf[:n.value].copy()

    def debug_cells(self, item=0, cap=1 << 16):
        """Window cells (wx, wy) of the base readings that were rasterised, [slot][beam]; INT32_MIN = filtered."""
        buf = np.zeros((cap, 2), dtype=np.int32)
        max_n = C.c_int32()
        _capi.check(self._lib.ym_debug_cells(self._m, item, buf.ctypes.data_as(C.POINTER(C.c_int32)), buf.size,
                                             C.byref(max_n)))
        return buf.reshape(-1, 2), max_n.value

    def debug_pair_lists(self, slot=0):
        """The region correlate's pair lists of query slot `slot` of the last call (include/yagmatch.h, ym_debug_pair_lists): a dict
        of the geometry they were built for (ints), `ctrig` [nt][2], `starts` [lparts][nbins + 1], `flags` [lparts], `entries`
        [lparts][entries_pstride] and `rbox` [nregions][lparts][4] = rmin, rmax, xmin, xmax."""
        info = _capi.YmPairListInfo()
        none = (None,) * 5
        _capi.check(self._lib.ym_debug_pair_lists(self._m, int(slot), C.byref(info), *none))
        ctrig = np.zeros((info.nt, 2))
        starts = np.zeros((info.lparts, info.nbins + 1), dtype=np.int32)
        flags = np.zeros(info.lparts, dtype=np.int32)
        entries = np.zeros((info.lparts, info.entries_pstride), dtype=np.uint16)
        rbox = np.zeros((info.nregions, info.lparts), dtype=np.uint32)
        _capi.check(self._lib.ym_debug_pair_lists(self._m, int(slot), C.byref(info), ctrig.ctypes.data_as(C.POINTER(C.c_double)),
                                                  starts.ctypes.data_as(C.POINTER(C.c_int32)), flags.ctypes.data_as(C.POINTER(C.c_int32)),
                                                  entries.ctypes.data_as(C.POINTER(C.c_uint16)), rbox.ctypes.data_as(C.POINTER(C.c_uint32))))
        out = {n: int(getattr(info, n)) for n, _ in _capi.YmPairListInfo._fields_[:17]}
        out.update(slot=int(slot), off_x=info.off_x, off_y=info.off_y, ylat=(info.ylat[0], info.ylat[1]), ctrig=ctrig, starts=starts,
                   flags=flags, entries=entries,
                   rbox=np.stack([rbox & 255, (rbox >> 8) & 255, (rbox >> 16) & 255, rbox >> 24], axis=-1).astype(np.int32))
        return out

    def debug_yag_frame(self, item=0, pass_=0):
        """What find_best_pose pass `pass_` of item `item` of the last "yagpy" call computed with (include/yagmatch.h,
        ym_debug_yag_frame): a dict of the pass's geometry, `xvals`, `yvals`, `tvals`, `trig` [nt][2] = the device's (cos, sin) of
        every angle and `points` [nq][2] = the item's point set."""
        info = _capi.YmYagFrame()
        _capi.check(self._lib.ym_debug_yag_frame(self._m, int(item), int(pass_), C.byref(info), None, None, None))
        axes = np.zeros(info.nx + info.ny + info.nt)
        trig = np.zeros((info.nt, 2))
        pts = np.zeros((info.nq, 2))
        dp = C.POINTER(C.c_double)
        _capi.check(self._lib.ym_debug_yag_frame(self._m, int(item), int(pass_), C.byref(info), axes.ctypes.data_as(dp),
                                                 trig.ctypes.data_as(dp), pts.ctypes.data_as(dp)))
        out = {n: (int if t is C.c_int32 else float)(getattr(info, n)) for n, t in _capi.YmYagFrame._fields_[:-1]}
        out["pass"] = out.pop("pass_")
        out.update(centre=tuple(info.centre), xvals=axes[:info.nx].copy(), yvals=axes[info.nx:info.nx + info.ny].copy(),
                   tvals=axes[info.nx + info.ny:].copy(), trig=trig, points=pts)
        return out

    def debug_option(self, option, value):
        _capi.check(self._lib.ym_debug_option(self._m, int(option), int(value)))

    def debug_stamps(self, enable=True):
        buf = (C.c_uint64 * 32)()
        _capi.check(self._lib.ym_debug_stamps(self._m, int(bool(enable)), buf, 32))
        return list(buf)

    def cache_stats(self):
        """(hits, misses) of the matcher's point cache since it was created"""
        h, ms = C.c_int64(0), C.c_int64(0)
        _capi.check(self._lib.ym_cache_stats(self._m, C.byref(h), C.byref(ms)))
        return int(h.value), int(ms.value)

    def debug_counters(self):
        """dict of the matcher's counters since it was created (include/yagmatch.h, ym_debug_counters)"""
        buf = (C.c_int64 * 10)()
        _capi.check(self._lib.ym_debug_counters(self._m, buf, 10))
        return dict(yag_fast_items=int(buf[0]), yag_fallback_items=int(buf[1]), yag_pairs_checked=int(buf[2]),
                    yag_pairs_failed=int(buf[3]), list_cache_hits=int(buf[4]), map_kernel_items=int(buf[6]), map_fallback_items=int(buf[7]),
                    sets_kernel_items=int(buf[8]), sets_fallback_items=int(buf[9]),
                    last_correlate={-1: None, 0: "correlate_kernel", 1: "correlate_region_kernel", 2: "gather_kernel"}[int(buf[5])])

    def profile(self, on=True):
        _capi.check(self._lib.ym_profile_enable(self._m, int(bool(on))))

    def profile_read(self, which=0, reset=True):
        ms, n = C.c_double(), C.c_int64()
        _capi.check(self._lib.ym_profile_read(self._m, which, C.byref(ms), C.byref(n), int(bool(reset))))
        return ms.value, n.value


MapAddStats = namedtuple("MapAddStats", ["points", "stamped", "dropped", "x0", "y0", "x1", "y1"])
MapUpdateStats = namedtuple("MapUpdateStats", ["removed", "added", "dropped", "unmatched", "released", "gained", "x0", "y0", "x1", "y1"])
MapReframeStats = namedtuple("MapReframeStats", ["kept", "restamped", "dropped", "recomputed", "mismatch", "x0", "y0", "width", "height"])
SeenThrough = namedtuple("SeenThrough", ["scans", "inside", "seen", "flags"])


class CorrelationMap(object):
    """A correlation grid resident on the device (ym_map): built from an occupancy image, uploaded, or made empty and
    filled with `add_scans`.  `revision` starts at 0 and goes up by one with every call that changed a cell -- an `add_scans`
    that stamped something, a `remove_scans` or `sync` that took something out or put something in -- and with every `clear`:
    what was derived from the map (a MapLocator) compares it with the revision it was made at.

    A counted map (`ScanMatcher.empty_correlation_map(w, h, counted=True, ox=..., oy=...)`) can also
    forget: `counted` is True, `origin` its fixed (ox, oy), and it keeps every scan it holds with the pose it was added at, as
    LiveOccupancyGrid does, so `remove_scans` and `sync` take out exactly what went in whatever happened to the scan's pose
    since.  `scan in cmap` and `len(cmap)` speak of the held scans.  On any other map `counted` is False, `origin` None, and
    the methods that forget raise ValueError.

    Every map has a `window` (x0, y0, width, height) in cells of the lattice it started in, which `reframe` moves or resizes
    (DESIGN.md section 17); a counted map's `anchor` is its first origin and stays, its `origin` follows the window."""

    def __init__(self, matcher, handle, origin=None, offset=(0, 0)):
        self.m, self._h = matcher, handle
        w, h = C.c_int32(), C.c_int32()
        _capi.check(matcher._lib.ym_map_size(handle, C.byref(w), C.byref(h)))
        self.shape = (h.value, w.value)
        self.revision = 0
        # `origin` is the anchor; a window that does not start at the anchor's cell (0, 0) has its own origin (section 17)
        self.counted, self._anchor, self._offset = origin is not None, origin, (int(offset[0]), int(offset[1]))
        self.origin = origin
        if origin is not None and self._offset != (0, 0):
            res = float(matcher._cfg.resolution)
            self.origin = (origin[0] + self._offset[0] * res, origin[1] + self._offset[1] * res)
        self._held = {}  # counted maps: id(scan) -> (the scan, the pose it was added at); insertion-ordered

    def add_scans(self, ox, oy, scans):
        """The reference's `add_scan_to_grid` (helpers.py:105-131) on the device (`ym_map_add_scans`): every point reading
        `scan.points()` yields at the scan's current pose is stamped into the map whose cell (0, 0) lies at world (ox, oy)
        and max-smeared with the matcher's kernel; readings outside the map are dropped and counted.  The map does not
        depend on the order of scans or calls.  Returns MapAddStats(points, stamped, dropped, x0, y0, x1, y1): the changed
        cells lie inside [x0, x1) x [y0, y1).
        On a counted map (ox, oy) must be the map's origin and no scan may be held already (ValueError, before the library
        is touched); the scans are then held at the poses they have now."""
        scans = list(scans)
        counted = getattr(self, "counted", False)
        if counted:
            if (float(ox), float(oy)) != self.origin:
                raise ValueError("add_scans: this counted map's origin is %r, not (%r, %r)" % (self.origin, ox, oy))
            self._distinct(scans, "add_scans", held=False)
        hs = (C.c_void_p * max(1, len(scans)))(*[self.m._require_native(q) for q in scans])
        poses = [_pose_of(q) for q in scans] if counted else None
        st = _capi.YmMapAddStats()
        _capi.check(self.m._lib.ym_map_add_scans(self.m._m, self._h, float(ox), float(oy), hs, len(scans), C.byref(st)))
        if counted:
            for q, pose in zip(scans, poses):
                self._held[id(q)] = (q, pose)
        if st.stamped > 0:
            self.revision += 1
        return MapAddStats(st.points, st.stamped, st.dropped, st.x0, st.y0, st.x1, st.y1)

    def clear(self):
        """every cell back to zero (`ym_map_clear`); a counted map forgets the scans it held"""
        _capi.check(self.m._lib.ym_map_clear(self.m._m, self._h))
        if getattr(self, "counted", False):
            self._held = {}
        self.revision += 1

    # ---- counted maps: the scans held, and letting them go (ym_map_update_scans)
    def _need_counted(self, what):
        if not getattr(self, "counted", False):
            raise ValueError("%s: this map keeps no counts; make it with empty_correlation_map(w, h, counted=True, ox=..., oy=...)" % what)

    def _distinct(self, scans, what, held):
        seen = set()
        for i, q in enumerate(scans):
            if id(q) in seen:
                raise ValueError("%s: scan %d is in the list twice" % (what, i))
            seen.add(id(q))
            if (id(q) in self._held) != held:
                raise ValueError("%s: scan %d is %s" % (what, i, "not held" if held else "already held"))

    def __len__(self):
        self._need_counted("len")
        return len(self._held)

    def __bool__(self):  # (a map is a map however many scans it holds)
        return True

    def __contains__(self, scan):
        self._need_counted("in")
        return id(scan) in self._held

    def _update(self, remove, add):
        """`remove` out at the poses they were added at and `add` in at their current ones, in one library call"""
        if not remove and not add:
            return MapUpdateStats(*([0] * 10))
        lib = self.m._lib
        rs = (C.c_void_p * max(1, len(remove)))(*[self.m._require_native(q) for q in remove])
        ads = (C.c_void_p * max(1, len(add)))(*[self.m._require_native(q) for q in add])
        old = np.array([self._held[id(q)][1] for q in remove], dtype=np.float64).reshape(len(remove), 3)
        new = [_pose_of(q) for q in add]
        st = _capi.YmMapUpdateStats()
        _capi.check(lib.ym_map_update_scans(self.m._m, self._h, rs, old.ctypes.data_as(C.POINTER(C.c_double)), len(remove), ads,
                                            len(add), C.byref(st)))
        for q in remove:
            del self._held[id(q)]
        for q, pose in zip(add, new):
            self._held[id(q)] = (q, pose)
        if st.removed > 0 or st.added > 0:
            self.revision += 1
        out = MapUpdateStats(st.removed, st.added, st.dropped, st.unmatched, st.released, st.gained, st.x0, st.y0, st.x1, st.y1)
        if st.unmatched > 0:
            raise RuntimeError("CorrelationMap: %d removed readings met a count of zero: the map's counts and the scans it is "
                               "said to hold disagree (%r)" % (st.unmatched, out))
        return out

    def remove_scans(self, scans):
        """Take held scans out of a counted map, at the poses they were added at.  A scan that is not held raises ValueError
        before the library is touched.  Returns MapUpdateStats(removed, added, dropped, unmatched, released, gained, x0, y0,
        x1, y1): readings, then cells, then the rectangle that holds every changed cell."""
        self._need_counted("remove_scans")
        scans = list(scans)
        self._distinct(scans, "remove_scans", held=True)
        return self._update(scans, [])

    def sync(self, scans=None):
        """Move every held scan among `scans` (None: all held scans; scans that are not held are passed over) whose current
        pose differs from the one it was added at: out at the old pose and in at the new one, in one library call.  The cost
        is that of the moved scans.  Returns MapUpdateStats."""
        self._need_counted("sync")
        if scans is not None:
            scans = list(scans)
            if len({id(q) for q in scans}) != len(scans):
                raise ValueError("sync: a scan is in the list twice")
        moved = self.moved_scans(scans)
        return self._update(moved, moved)

    def moved_scans(self, scans=None):
        """the held scans among `scans` (None: all held scans) whose current pose differs from the one they were added at"""
        self._need_counted("moved_scans")
        if scans is None:
            scans = [e[0] for e in self._held.values()]
        return [q for q in scans if id(q) in self._held and self._held[id(q)][1] != _pose_of(q)]

    def update_scans(self, remove, add):
        """`remove_scans(remove)` and `add_scans(ox, oy, add)` in ONE library call (`ym_map_update_scans`): the removed scans go
        out first.  A scan may be in both lists (it is moved); otherwise the rules of the two methods hold.  Returns
        MapUpdateStats."""
        self._need_counted("update_scans")
        remove, add = list(remove), list(add)
        self._distinct(remove, "update_scans (remove)", held=True)
        going = {id(q) for q in remove}
        self._distinct([q for q in add if id(q) not in going], "update_scans (add)", held=False)
        if len({id(q) for q in add}) != len(add):
            raise ValueError("update_scans (add): a scan is in the list twice")
        return self._update(remove, add)

    # ---- noticing change (ym_map_seen_through)
    def seen_through(self, viewers, scans=None, clearance=2, protect=1, flags=False):
        """Which held readings do the `viewers` (scans at their current poses, held or not) look straight through?  A viewer's
        ray from its sensor cell to a reading's cell sweeps the cells it crosses more than `clearance` cells before its end; a
        cell within `protect` cells of any viewer reading's end is never swept (DESIGN.md section 19 states the rule).  `scans`:
        a subset of the held scans (None: all, in held order), counted at the poses they were added at; one that is not held
        raises ValueError before the library is touched.  Returns SeenThrough(scans, inside, seen, flags): per scan the valid
        readings whose cell lies in the window and those of them whose cell is swept (int arrays), and -- with flags=True -- a
        boolean array per scan, True exactly for the readings counted in `seen` (else None).  The map does not change.  The
        defaults come from a numpy prototype on one synthetic room, not from a device or a real log."""
        self._need_counted("seen_through")
        viewers = list(viewers)
        scans = [e[0] for e in self._held.values()] if scans is None else list(scans)
        self._distinct(scans, "seen_through", held=True)
        for name, v in (("clearance", clearance), ("protect", protect)):
            if isinstance(v, bool) or not isinstance(v, (int, np.integer)) or v < 0:
                raise ValueError("seen_through: %s %r: an integer of at least 0" % (name, v))
        n, max_n = len(scans), max([len(q.ranges) for q in scans] + [1])
        hs = (C.c_void_p * max(1, n))(*[self.m._require_native(q) for q in scans])
        vs = (C.c_void_p * max(1, len(viewers)))(*[self.m._require_native(q) for q in viewers])
        poses = np.array([self._held[id(q)][1] for q in scans], dtype=np.float64).reshape(n, 3)
        counts = np.zeros((n, 2), dtype=np.int32)
        fl = np.zeros((n, max_n), dtype=np.uint8) if flags else None
        _capi.check(self.m._lib.ym_map_seen_through(
            self.m._m, self._h, hs, poses.ctypes.data_as(C.POINTER(C.c_double)), n, vs, len(viewers), int(clearance), int(protect),
            counts.ctypes.data_as(C.POINTER(C.c_int32)), fl.ctypes.data_as(C.POINTER(C.c_uint8)) if flags else None, None, None))
        per_scan = [fl[i, :len(q.ranges)].astype(bool) for i, q in enumerate(scans)] if flags else None
        return SeenThrough(scans, counts[:, 0].astype(np.int64), counts[:, 1].astype(np.int64), per_scan)

    def debug_swept_mask(self, viewers, clearance=2, protect=1):
        """test hook: the cells the viewers sweep after protection, uint8 of the map's shape (`ym_map_seen_through`'s mask)"""
        self._need_counted("debug_swept_mask")
        viewers = list(viewers)
        vs = (C.c_void_p * max(1, len(viewers)))(*[self.m._require_native(q) for q in viewers])
        mask = np.zeros(self.shape, dtype=np.uint8)
        st = _capi.YmMapSeenStats()
        _capi.check(self.m._lib.ym_map_seen_through(self.m._m, self._h, None, None, 0, vs, len(viewers), int(clearance), int(protect), None,
                                                    None, mask.ctypes.data_as(C.POINTER(C.c_uint8)), C.byref(st)))
        return mask, int(st.rays)

    # ---- the window (ym_map_reframe)
    @property
    def anchor(self):
        """a counted map's first origin: world position of cell (0, 0) of the lattice its window moves in (None on other maps)"""
        a = getattr(self, "_anchor", None)
        return a if a is not None else getattr(self, "origin", None)

    @property
    def window(self):
        """(x0, y0, width, height): the map's cell (0, 0) is cell (x0, y0) of the anchor's lattice"""
        x0, y0 = getattr(self, "_offset", (0, 0))
        return (x0, y0, self.shape[1], self.shape[0])

    def reframe(self, dx, dy, width=None, height=None):
        """Move or resize the window (`ym_map_reframe`): new cell (i, j) is the old cell (i + dx, j + dy), in a window of `width` x
        `height` cells (None: as now).  A counted map is afterwards, bit for bit, the map a fresh counted map with the same
        anchor, the new window and the same held scans would be -- readings the old window dropped are stamped, readings that
        left it take their counts along, cells near a side that moved are recomputed -- and `origin` becomes
        anchor + offset * resolution, computed from the first origin, never step by step; the scans stay held.  Any other map
        keeps no scans and no origin: the overlap keeps its values, every other cell is zero, the caller moves its own origin by
        (dx, dy) cells, and what the border cells would have received from readings dropped earlier is lost.
        `revision` goes up unless the call was the identity.  Returns MapReframeStats(kept, restamped, dropped, recomputed,
        mismatch, x0, y0, width, height); RuntimeError if the counts and the held scans disagree (nothing was changed)."""
        old = self.window
        width = old[2] if width is None else int(width)
        height = old[3] if height is None else int(height)
        dx, dy = int(dx), int(dy)
        counted = getattr(self, "counted", False)
        held = [e for e in self._held.values()] if counted else []
        hs = (C.c_void_p * max(1, len(held)))(*[self.m._require_native(q) for q, _ in held])
        poses = np.array([pose for _, pose in held], dtype=np.float64).reshape(len(held), 3)
        st = _capi.YmMapReframeStats()
        rc = self.m._lib.ym_map_reframe(self.m._m, self._h, dx, dy, width, height, hs, poses.ctypes.data_as(C.POINTER(C.c_double)),
                                        len(held), C.byref(st))
        out = MapReframeStats(st.kept, st.restamped, st.dropped, st.recomputed, st.mismatch, st.x0, st.y0, st.width, st.height)
        if st.mismatch != 0:
            raise RuntimeError("CorrelationMap: the kept cells' counts and the held scans' readings there differ by %d: the map's "
                               "counts and the scans it is said to hold disagree; nothing was changed (%r)" % (st.mismatch, out))
        _capi.check(rc)
        if (dx, dy, width, height) != (0, 0, old[2], old[3]):
            anchor = self.anchor
            self._offset = (old[0] + dx, old[1] + dy)
            self.shape = (height, width)
            if counted:
                res = float(self.m._cfg.resolution)
                self._anchor = anchor
                self.origin = (anchor[0] + self._offset[0] * res, anchor[1] + self._offset[1] * res)
            self.revision += 1
        return out

    def stamps(self):
        """the number of readings stamped in each cell of a counted map (uint32, the map's shape)"""
        self._need_counted("stamps")
        out = np.empty(self.shape, dtype=np.uint32)
        _capi.check(self.m._lib.ym_map_read_stamps(self._h, out.ctypes.data_as(C.POINTER(C.c_uint32)), out.size))
        return out

    def to_numpy(self):
        out = np.empty(self.shape, dtype=np.float64)
        _capi.check(self.m._lib.ym_map_read(self._h, out.ctypes.data_as(C.POINTER(C.c_double)), out.size))
        return out

    def close(self):
        if getattr(self, "_h", None):
            self.m._lib.ym_map_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def _map_set_result(res, query_scans):
    """the ScanMatcherResult `match_scan_sets_with_map` builds from the library's ym_result of one set, and meta["rigid_poses"]"""
    r = _result(res)
    # scan_matching.py:136-139,167-173: the search centre is the mean query position with heading 0; every query is moved by
    # (corrected centre - centre)
    xs = [float(q.corrected_pose.x) for q in query_scans]
    ys = [float(q.corrected_pose.y) for q in query_scans]
    oxy = Transform.from_position_euler(sum(xs) / float(len(xs)), sum(ys) / float(len(ys)), 0, 0, 0, 0)
    diff = r.best_pose - oxy
    r.meta["centre"] = (oxy.x, oxy.y, 0.0)
    r.meta["corrected_centre"] = (r.best_pose.x, r.best_pose.y, r.best_pose.euler[-1])
    c0, c1 = r.meta["centre"], r.meta["corrected_centre"]
    r.meta["rigid_poses"] = _move_rigidly([q.corrected_pose for q in query_scans], c0[0], c0[1], c1[0], c1[1], c1[2] - c0[2])
    return ScanMatcherResult(r.response, r.covariance, [q.corrected_pose + diff for q in query_scans], r.meta)


def _scan_set_result(res, query_scans):
    """the ScanMatcherResult `match_scan_sets` builds from the library's ym_result of one set"""
    r = _result(res)
    # scan_matching.py:68-71,116-121: the centre is the mean query position with heading 0; every query is moved by
    # (corrected centre - centre), composed from the LEFT: diff + q.corrected_pose, the reference's operand order
    xs = [float(q.corrected_pose.x) for q in query_scans]
    ys = [float(q.corrected_pose.y) for q in query_scans]
    oxy = Transform.from_position_euler(sum(xs) / float(len(xs)), sum(ys) / float(len(ys)), 0, 0, 0, 0)
    diff = r.best_pose - oxy
    r.meta["centre"] = (oxy.x, oxy.y, 0.0)
    r.meta["corrected_centre"] = (r.best_pose.x, r.best_pose.y, r.best_pose.euler[-1])
    c0, c1 = r.meta["centre"], r.meta["corrected_centre"]
    r.meta["rigid_poses"] = _move_rigidly([q.corrected_pose for q in query_scans], c0[0], c0[1], c1[0], c1[1], c1[2] - c0[2])
    return ScanMatcherResult(r.response, r.covariance, [diff + q.corrected_pose for q in query_scans], r.meta)


def _pick_polished(polished, meta):
    """`locate_in_map(polish_top=K)`: the best of the K polished candidates (the first of equals), as the result locate_in_map returns"""
    best = 0
    for i, r in enumerate(polished):
        if r.response > polished[best].response:
            best = i
    r = polished[best]
    meta = dict(meta)
    meta.update(r.meta)
    meta["wrapper_poses"] = r.best_pose
    meta["polished"] = [ScanMatcherResult(p.response, p.covariance, p.meta["rigid_poses"], p.meta) for p in polished]
    meta["polished_index"] = best
    return ScanMatcherResult(r.response, r.covariance, r.meta["rigid_poses"], meta)


LocateCandidate = namedtuple("LocateCandidate", ["score", "response", "index", "k", "cx", "cy", "pose", "poses"])


def _move_rigidly(poses, cx, cy, nx, ny, dyaw):
    """the poses after the rigid motion that turns the plane by dyaw about (cx, cy) and takes that point to (nx, ny)"""
    c, s = np.cos(dyaw), np.sin(dyaw)
    return [Transform(nx + c * (p.x - cx) - s * (p.y - cy), ny + s * (p.x - cx) + c * (p.y - cy), 0.0, p.euler[-1] + dyaw)
            for p in poses]


def filter_min_separation(candidates, metres, radians):
    """Greedy, best first: a candidate is dropped when a better kept one lies within BOTH `metres` and `radians` of it
    (headings compared modulo 2 pi).  `candidates` carry `.pose` (x, y, euler) and come best first."""
    kept = []
    for c in candidates:
        for b in kept:
            da = (c.pose.euler[-1] - b.pose.euler[-1] + np.pi) % (2 * np.pi) - np.pi
            if np.hypot(c.pose.x - b.pose.x, c.pose.y - b.pose.y) <= metres and abs(da) <= radians:
                break
        else:
            kept.append(c)
    return kept


class MapLocator(object):
    """Where in a resident map was a scan set taken?  The exact top-K of the integer correlation score over every cell and
    heading, by branch and bound over a max pyramid of the map on the device (ym_locator)."""

    def __init__(self, matcher, cmap, levels=None, max_nodes=None):
        self.m = matcher
        self._h = matcher._lib.ym_locator_create(matcher._m, cmap._h, -1 if levels is None else int(levels),
                                                 0 if max_nodes is None else int(max_nodes))
        if not self._h:
            raise _capi.YmError(-1, _capi.last_error())
        info = _capi.YmLocatorInfo()
        _capi.check(matcher._lib.ym_locator_get_info(self._h, C.byref(info)))
        self.shape, self.levels, self.max_nodes, self.bytes = (info.height, info.width), info.levels, info.max_nodes, info.bytes
        self.last_stats, self.last_points, self.last_heading_step, self.last_separation = None, None, None, None
        # the pyramid holds a copy of the map as it is now: a map that takes scans afterwards leaves it stale
        self._cmap, self._revision = cmap, getattr(cmap, "revision", 0)

    def read_level(self, level):
        """test hook: level `level` of the pyramid over the map's own cells"""
        out = np.empty(self.shape, dtype=np.uint8)
        _capi.check(self.m._lib.ym_locator_read_level(self._h, int(level), out.ctypes.data_as(C.POINTER(C.c_uint8)), out.size))
        return out

    def locate(self, query_scans, ox, oy, n_angles=360, headings=None, top_k=16, min_response=0.0, point_stride=1,
               min_separation=None):
        """The `top_k` best hypotheses (LocateCandidate: score, response, index, k, cx, cy, pose = Transform of the set's
        centre, poses = every query scan's pose after the rigid motion that takes the centre -- the mean query position,
        heading 0 -- to `pose`), best first, ties by ascending index.  headings: explicit angles (default 2 pi k / n_angles).
        min_separation = (metres, radians): the device's best 64 are filtered greedily (filter_min_separation) before the
        first top_k are returned.  That only THINS the best 64, which are nearly always neighbours of the best in cell and
        heading: a runner-up place that scores below the best place's own halo is not among them.  For the K best distinct
        places over the whole volume use `locate_places`.  `.last_stats`: dict(nq, chunks, nodes and survivors per level, probe_nodes); `.last_points`: the point set."""
        self._check_revision()
        headings, dir_cs = self._heading_table(n_angles, headings)
        want = 64 if min_separation is not None else int(top_k)
        if min_separation is not None and not 1 <= int(top_k) <= 64:
            raise ValueError("top_k must be in [1, 64]")
        hs = (C.c_void_p * max(1, len(query_scans)))(*[self.m._require_native(q) for q in query_scans])
        opts = _capi.YmLocateOpts(want, int(point_stride), float(min_response))
        out = (_capi.YmLocateCandidate * max(1, want))()
        n_found, stats = C.c_int(0), _capi.YmLocateStats()
        cap = sum(len(q.ranges) for q in query_scans)
        pts = np.zeros((max(1, cap), 2))
        _capi.check(self.m._lib.ym_locator_locate(self._h, float(ox), float(oy), hs, len(query_scans),
                                                  dir_cs.ctypes.data_as(C.POINTER(C.c_double)), dir_cs.shape[0], C.byref(opts), out,
                                                  C.byref(n_found), pts.ctypes.data_as(C.POINTER(C.c_double)), C.byref(stats)))
        self.last_stats = dict(nq=stats.nq, chunks=stats.chunks, nodes=list(stats.nodes), survivors=list(stats.survivors),
                               probe_nodes=stats.probe_nodes)
        self.last_points = pts[:stats.nq].copy()
        self.last_heading_step = self._heading_step(headings)
        cands = self._candidates(query_scans, out[:n_found.value])
        if min_separation is not None:
            cands = filter_min_separation(cands, float(min_separation[0]), float(min_separation[1]))[:int(top_k)]
        return cands

    def locate_places(self, query_scans, ox, oy, n_places=4, min_separation=(1.0, 0.5), separation_cells=None, n_angles=360,
                      headings=None, min_response=0.0, point_stride=1):
        """The `n_places` (1 .. 16) best DISTINCT places, as LocateCandidates in place order: place 1 is the best hypothesis
        of all, place i + 1 the best one that is near none of places 1 .. i -- exact over every cell and heading, not a
        thinning of a top list (`ym_locator_locate_places`; one search per place).  Two hypotheses
        are near when BOTH their cells lie within the cell separation and their heading indices within the heading
        separation.  separation_cells = (sep_cells2, sep_headings): the squared cell distance and the heading steps, taken
        as they are; otherwise from min_separation = (metres, radians): sep_cells2 = int((metres / res) ** 2 + 1e-6),
        sep_headings = int(radians / step + 1e-6), step = the heading table's step (`last_heading_step`).  Heading indices
        are compared on a circle exactly when `headings` is None (the full turn 2 pi k / n_angles).
        `.last_separation`: (sep_cells2, sep_headings, circular) as used; `.last_stats`: dict(nq, rounds, chunks, nodes,
        probe_nodes, excluded_leaves, excluded_nodes, round_nodes); `.last_points`: the point set."""
        self._check_revision()
        circular = 1 if headings is None else 0
        headings, dir_cs = self._heading_table(n_angles, headings)
        step = self._heading_step(headings)
        if separation_cells is not None:
            sep_cells2, sep_headings = int(separation_cells[0]), int(separation_cells[1])
        else:
            sep_cells2 = int((float(min_separation[0]) / float(self.m.config.resolution)) ** 2 + 1e-6)
            sep_headings = int(float(min_separation[1]) / step + 1e-6)
        want = int(n_places)
        hs = (C.c_void_p * max(1, len(query_scans)))(*[self.m._require_native(q) for q in query_scans])
        opts = _capi.YmLocatePlacesOpts(want, int(point_stride), float(min_response), sep_cells2, sep_headings, circular)
        out = (_capi.YmLocateCandidate * max(1, want))()
        n_found, stats = C.c_int(0), _capi.YmLocatePlacesStats()
        cap = sum(len(q.ranges) for q in query_scans)
        pts = np.zeros((max(1, cap), 2))
        _capi.check(self.m._lib.ym_locator_locate_places(self._h, float(ox), float(oy), hs, len(query_scans),
                                                         dir_cs.ctypes.data_as(C.POINTER(C.c_double)), dir_cs.shape[0], C.byref(opts), out,
                                                         C.byref(n_found), pts.ctypes.data_as(C.POINTER(C.c_double)), C.byref(stats)))
        self.last_stats = dict(nq=stats.nq, rounds=stats.rounds, chunks=stats.chunks, nodes=stats.nodes, probe_nodes=stats.probe_nodes,
                               excluded_leaves=stats.excluded_leaves, excluded_nodes=stats.excluded_nodes,
                               round_nodes=list(stats.round_nodes)[:stats.rounds])
        self.last_points = pts[:stats.nq].copy()
        self.last_heading_step = step
        self.last_separation = (sep_cells2, sep_headings, circular)
        return self._candidates(query_scans, out[:n_found.value])

    @staticmethod
    def _heading_table(n_angles, headings):
        """(headings, their (cos, sin) rows) -- by default the full turn 2 pi k / n_angles"""
        if headings is None:
            headings = 2.0 * np.pi * np.arange(int(n_angles)) / float(int(n_angles))
        headings = np.ascontiguousarray(headings, dtype=np.float64).reshape(-1)
        return headings, np.ascontiguousarray(np.stack([np.cos(headings), np.sin(headings)], axis=1))

    @staticmethod
    def _heading_step(headings):
        return float(2.0 * np.pi / len(headings)) if len(headings) < 2 else float(abs(headings[1] - headings[0]))

    @staticmethod
    def _candidates(query_scans, found):
        """the library's candidates as LocateCandidates: every query scan moved rigidly with the set's centre"""
        xs = [float(q.corrected_pose.x) for q in query_scans]
        ys = [float(q.corrected_pose.y) for q in query_scans]
        cx, cy = sum(xs) / float(len(xs)), sum(ys) / float(len(ys))
        cands = []
        for c in found:
            pose = Transform(c.pose[0], c.pose[1], 0.0, c.pose[2])
            cands.append(LocateCandidate(c.score, c.response, c.index, c.k, c.cx, c.cy, pose,
                                         _move_rigidly([q.corrected_pose for q in query_scans], cx, cy, pose.x, pose.y, c.pose[2])))
        return cands

    def _check_revision(self):
        now = getattr(self._cmap, "revision", 0)
        if now != self._revision:
            raise ValueError("MapLocator: the map has changed since this locator was made (revision %d, now %d): "
                             "make a new locator with map_locator(cmap)" % (self._revision, now))

    def close(self):
        if getattr(self, "_h", None):
            self.m._lib.ym_locator_destroy(self._h)
            self._h = None

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class MatchBatch(object):
    """One query against many candidate chains, resident on the device, runnable many times.

    Replaces the serial `for chain in chains: loop_matcher.match_scan(scan, chain, False, False)` of
    /root/reference/yag_slam/graph_slam.py:217-220 by one enqueue per batch."""

    def __init__(self, matcher, query, chains, pairs=False):
        """pairs: `query` is a sequence of queries, item i = query[i] against chains[i] (ScanMatcher.make_pairs_batch)"""
        self.m = matcher
        self.query = query
        self.chains = [list(c) for c in chains]
        self._queries = list(query) if pairs else [query]
        if pairs and len(self._queries) != len(self.chains):
            raise ValueError("a pairs batch needs one chain per query")
        flat, offs = [], [0]
        for ch in self.chains:
            flat.extend(ch)
            offs.append(len(flat))
        self._flat = flat
        hs = (C.c_void_p * max(1, len(flat)))(*matcher._handles(flat))
        co = (C.c_int32 * len(offs))(*offs)
        if pairs:
            hq = (C.c_void_p * max(1, len(self._queries)))(*matcher._handles(self._queries))
            self._h = matcher._lib.ym_pairs_create(matcher._m, hq, hs, co, len(self.chains))
        else:
            hq = matcher._require_native(query)
            self._h = matcher._lib.ym_batch_create(matcher._m, hq, hs, co, len(self.chains))
        if not self._h:
            raise _capi.YmError(-1, _capi.last_error())
        self.n = len(self.chains)

    @classmethod
    def from_handles(cls, matcher, query_handles, scan_handles, offsets):
        """A pairs batch over raw ym_scan* arrays (numpy uint64; models.ScanBlock.handles): item i = query_handles[i] against
        scan_handles[offsets[i]:offsets[i + 1]].  No Python object per scan; the caller keeps the scans alive while the batch is used."""
        self = cls.__new__(cls)
        self.m, self.query, self.chains, self._queries, self._flat = matcher, None, None, None, None
        qh = np.ascontiguousarray(query_handles, dtype=np.uint64)
        sh = np.ascontiguousarray(scan_handles, dtype=np.uint64)
        co = np.ascontiguousarray(offsets, dtype=np.int32)
        if co.shape[0] != qh.shape[0] + 1:
            raise ValueError("a pairs batch needs one chain per query")
        self._h = matcher._lib.ym_pairs_create(matcher._m, qh.ctypes.data_as(C.POINTER(C.c_void_p)), sh.ctypes.data_as(C.POINTER(C.c_void_p)),
                                               co.ctypes.data_as(C.POINTER(C.c_int32)), int(qh.shape[0]))
        if not self._h:
            raise _capi.YmError(-1, _capi.last_error())
        self.n = int(qh.shape[0])
        return self

    def close(self):
        if getattr(self, "_h", None):
            try:
                self.m._lib.ym_batch_destroy(self._h)
            except Exception:
                pass
            self._h = None

    def __del__(self):
        self.close()

    def push_poses(self):
        """Write the scans' current corrected poses through to their device twins."""
        scans = self._queries + self._flat
        hs = self.m._handles(scans)
        xyz = np.array([_pose_of(s) for s in scans], dtype=np.float64).reshape(len(scans), 3)
        _capi.check(self.m._lib.ym_scans_set_poses((C.c_void_p * len(hs))(*hs), xyz.ctypes.data_as(C.POINTER(C.c_double)), len(hs)))

    def run_async(self, penalty=False, do_fine=False, slot=0, chain_id_base=0, dev_best_out=None):
        _capi.check(self.m._lib.ym_batch_run_async(self.m._m, self._h, int(bool(penalty)), int(bool(do_fine)), int(slot),
                                                   int(chain_id_base), C.c_void_p(dev_best_out) if dev_best_out else None))

    def wait(self, slot=0, per_chain=True):
        per = (_capi.YmResult * self.n)() if per_chain else None
        best = _capi.YmResult()
        bi = C.c_int32(-1)
        _capi.check(self.m._lib.ym_batch_wait(self.m._m, int(slot), per, C.byref(best), C.byref(bi)))
        return (_results(per, check=True) if per_chain else None), _result(best), int(bi.value)


# names the reference exports (scan_matching.py:32,224)
Scan2DMatcherCpp = ScanMatcher
Scan2DMatcher = ScanMatcher
