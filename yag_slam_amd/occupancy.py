"""Occupancy-grid rendering: drop-in for `karto_scanmatcher.create_occupancy_grid(scans, resolution, range_threshold)`
as yag-slam calls it (/root/reference/yag_slam/graph_slam.py:341-342, /root/reference/ros1/slam_node_ros1:187-202,
/root/reference/yag_slam/helpers.py:595-603).  The returned object has what those callers touch: `.image` (uint8,
[height][width], 0 occupied / 200 unknown / 255 free), `.width`, `.height`, `.offset` (`.x`, `.y`: world position of
cell (0, 0)).  Rendered on the device from the scans' resident twins (include/yagmatch.h, ym_occupancy_*).  The wheel's
algorithm is not in the reference tree: restated from open_karto's OccupancyGrid, parity unpinned.

The map the ROS node publishes (slam_node_ros1:187-212, `_make_map`) is that grid with its specks removed and its codes
rewritten: `despeckle`, `create_clean_occupancy_grid`, `ros_codes` and `ros_map` give it with nothing but this package
installed (the filter runs on the device, ym_image_despeckle / ym_occupancy_create_clean).

`LiveOccupancyGrid` keeps the counts of that rendering on the device between publishes and changes them by the rays of the scans
that were added, moved or dropped (ym_occmap_*): a publish no longer costs the whole log."""
import ctypes as C
import math

import numpy as np

from . import _capi
from .transform import Pose2


class OccupancyGrid(object):
    def __init__(self, image, offset, resolution):
        self.image = image
        self.height, self.width = image.shape
        self.offset = offset
        self.resolution = resolution


def _handle(s, device):
    """ym_scan* of one element: a scan's device twin, or a handle as a plain int, a numpy integer (an element of
    ScanBlock.handles), a ctypes pointer or None (a null scan, which the library refuses)"""
    if hasattr(s, "native"):
        return s.native(device)
    if s is None or isinstance(s, C.c_void_p):
        return s
    return int(s)


def _scan_array(scans, device):
    handles = [_handle(s, device) for s in getattr(scans, "handles", scans)]
    return (C.c_void_p * max(1, len(handles)))(*handles), len(handles)


def create_occupancy_grid(scans, resolution, range_threshold, device=0, counts=False):
    """scans: yag_slam_amd.models.LocalizedRangeScan (or their native handles, as the reference passes `v.obj._scan`), or a
    models.ScanBlock.  counts=True (a test hook, ym_occupancy_create_counted): the grid also has `.passes` and `.hits`, uint32
    [height][width], the counts the image is decided from."""
    L = _capi.lib()
    arr, n = _scan_array(scans, device)
    create = L.ym_occupancy_create_counted if counts else L.ym_occupancy_create
    h = create(arr, n, float(resolution), float(range_threshold))
    if not h:
        raise _capi.YmError(-1, _capi.last_error())
    try:
        info = _capi.YmOccupancyInfo()
        _capi.check(L.ym_occupancy_get_info(h, C.byref(info)))
        image = np.empty((info.height, info.width), dtype=np.uint8)
        _capi.check(L.ym_occupancy_read(h, image.ctypes.data_as(C.POINTER(C.c_uint8)), image.size))
        if counts:
            passes, hits = np.empty(image.shape, dtype=np.uint32), np.empty(image.shape, dtype=np.uint32)
            u32 = C.POINTER(C.c_uint32)
            _capi.check(L.ym_occupancy_read_counts(h, passes.ctypes.data_as(u32), hits.ctypes.data_as(u32), image.size))
    finally:
        L.ym_occupancy_destroy(h)
    g = OccupancyGrid(image, Pose2(info.offset_x, info.offset_y, 0.0), info.resolution)
    if counts:
        g.passes, g.hits = passes, hits
    return g


STAT_NAMES = ("foreground_cells", "components", "removed_components", "cleared_cells", "background_cells", "background_filled")


def _filter_opts(foreground, fill, min_area, connectivity):
    """the filter's arguments as a YmDespeckleOpts; ValueError before the library is touched"""
    vals = {}
    for name, v in (("foreground", foreground), ("fill", fill), ("min_area", min_area), ("connectivity", connectivity)):
        if isinstance(v, (bool, np.bool_)) or not isinstance(v, (int, np.integer)):
            raise ValueError("%s %r: an integer" % (name, v))
        vals[name] = int(v)
    for name in ("foreground", "fill"):
        if not 0 <= vals[name] <= 255:
            raise ValueError("%s %d: 0 .. 255" % (name, vals[name]))
    if not 0 <= vals["min_area"] <= 2 ** 31 - 1:
        raise ValueError("min_area %d: 0 .. 2^31 - 1" % vals["min_area"])
    if vals["connectivity"] not in (4, 8):
        raise ValueError("connectivity %d: 4 or 8" % vals["connectivity"])
    return _capi.YmDespeckleOpts(vals["foreground"], vals["fill"], vals["min_area"], vals["connectivity"])


def _stats_dict(st):
    return {name: int(getattr(st, name)) for name in STAT_NAMES}


def despeckle(image, foreground=0, fill=255, min_area=5, connectivity=8, device=0, stats=False):
    """The node's cleanup (slam_node_ros1:191-197) for any 2-D uint8 array, on the device: every `connectivity`-connected
    component of `image == foreground` with fewer than min_area cells becomes `fill`; and, the node's loop visiting cv2's
    label 0 as well, so do the other cells when there are fewer than min_area (and at least one) of them.  Returns a new
    array, or (array, dict of STAT_NAMES) with stats=True.  Rows need not be contiguous (a slice's stride travels as the
    pitch); anything else is copied first."""
    opts = _filter_opts(foreground, fill, min_area, connectivity)
    if not isinstance(image, np.ndarray) or image.dtype != np.uint8 or image.ndim != 2:
        raise ValueError("image: a 2-D uint8 array")
    h, w = image.shape
    if h < 1 or w < 1:
        raise ValueError("image of %d x %d cells" % (w, h))
    if w * h > 2 ** 31 - 1:
        raise ValueError("image of %d x %d cells: at most 2^31 - 1" % (w, h))
    if image.strides[1] != 1 or image.strides[0] < w or image.strides[0] > 2 ** 31 - 1:
        image = np.ascontiguousarray(image)
    out = np.empty((h, w), dtype=np.uint8)
    st = _capi.YmDespeckleStats()
    u8 = C.POINTER(C.c_uint8)
    L = _capi.lib()
    _capi.check(L.ym_image_despeckle(int(device), image.ctypes.data_as(u8), w, h, int(image.strides[0]), C.byref(opts),
                                     out.ctypes.data_as(u8), C.byref(st)))
    return (out, _stats_dict(st)) if stats else out


def create_clean_occupancy_grid(scans, resolution, range_threshold, min_area=5, connectivity=8, device=0):
    """create_occupancy_grid, then the node's cleanup of the occupied cells (0 -> 255 in components under min_area cells) on
    the device image before its one copy to the host.  The grid has `.stats` (dict of STAT_NAMES)."""
    opts = _filter_opts(0, 255, min_area, connectivity)
    L = _capi.lib()
    arr, n = _scan_array(scans, device)
    h = L.ym_occupancy_create_clean(arr, n, float(resolution), float(range_threshold), C.byref(opts))
    if not h:
        raise _capi.YmError(-1, _capi.last_error())
    try:
        info = _capi.YmOccupancyInfo()
        _capi.check(L.ym_occupancy_get_info(h, C.byref(info)))
        image = np.empty((info.height, info.width), dtype=np.uint8)
        _capi.check(L.ym_occupancy_read(h, image.ctypes.data_as(C.POINTER(C.c_uint8)), image.size))
        st = _capi.YmDespeckleStats()
        _capi.check(L.ym_occupancy_get_despeckle_stats(h, C.byref(st)))
    finally:
        L.ym_occupancy_destroy(h)
    g = OccupancyGrid(image, Pose2(info.offset_x, info.offset_y, 0.0), info.resolution)
    g.stats = _stats_dict(st)
    return g


_ROS_TABLE = np.zeros(256, dtype=np.int8)
_ROS_TABLE[0], _ROS_TABLE[200], _ROS_TABLE[255] = 100, -1, 0  # slam_node_ros1:199-202
_ROS_KNOWN = np.zeros(256, dtype=bool)
_ROS_KNOWN[[0, 200, 255]] = True


def ros_codes(image):
    """a rendered grid's codes as nav_msgs/OccupancyGrid wants them (slam_node_ros1:199-202): 0 -> 100, 200 -> -1, 255 -> 0,
    int8 [height][width].  Any other value is not a rendered grid's: ValueError."""
    image = np.asarray(image)
    if image.dtype != np.uint8 or image.ndim != 2:
        raise ValueError("image: a 2-D uint8 array")
    if not _ROS_KNOWN[image].all():
        bad = np.unique(image[~_ROS_KNOWN[image]])
        raise ValueError("image holds %s: a rendered grid has 0, 200 and 255 only" % bad[:5].tolist())
    return _ROS_TABLE[image]


class RosMap(object):
    """what `_make_map` puts into its message: `.data` (int8 [height][width]; `.data.ravel()` is `map_msg.data`), `.width`,
    `.height`, `.resolution`, `.origin` (the grid offset); `.stats` as create_clean_occupancy_grid counts them"""

    def __init__(self, data, origin, resolution, stats):
        self.data = data
        self.height, self.width = data.shape
        self.origin = origin
        self.resolution = resolution
        self.stats = stats


def ros_map(scans, resolution, range_threshold, **filter_opts):
    """slam_node_ros1:187-209 without ROS: render, clean (filter_opts: min_area, connectivity, device), rewrite the codes"""
    g = create_clean_occupancy_grid(scans, resolution, range_threshold, **filter_opts)
    return RosMap(ros_codes(g.image), g.offset, g.resolution, g.stats)


def _pose_of(scan):
    p = scan.corrected_pose
    return (float(p.x), float(p.y), float(p.euler[-1]))


class LiveOccupancyGrid(object):
    """Pass and hit counts resident on the device, in a lattice that never moves.  `anchor` (x, y) fixes
    the lattice; None: the bounding-box minimum of the first add does.  With the anchor at `create_occupancy_grid(S, ...).offset`
    the grid holding S is that rendering bit for bit, however S was added.  `slack_cells`: cells of memory added on every side
    whenever the memory has to grow (0: every growing add reallocates).

    The object keeps every scan it holds and the pose it traced it at, so a removal subtracts exactly what was added whatever
    has happened to the scan's pose since.  `add`, `remove` and `sync` take LocalizedRangeScans (`add` also a models.ScanBlock,
    at its scans' own poses); their argument errors are raised before the library is touched, and an empty list is a no-op."""

    def __init__(self, resolution, range_threshold, anchor=None, slack_cells=64, device=0):
        resolution, range_threshold = float(resolution), float(range_threshold)
        if not (resolution > 0 and range_threshold > 0 and math.isfinite(resolution) and math.isfinite(range_threshold)):
            raise ValueError("resolution and range_threshold must be > 0")
        if isinstance(slack_cells, (bool, np.bool_)) or not isinstance(slack_cells, (int, np.integer)) or not 0 <= slack_cells <= 2 ** 30:
            raise ValueError("slack_cells %r: an integer, 0 .. 2^30" % (slack_cells,))
        if anchor is not None:
            anchor = tuple(float(v) for v in anchor)
            if len(anchor) != 2 or not all(math.isfinite(v) for v in anchor):
                raise ValueError("anchor %r: two finite numbers" % (anchor,))
        self.resolution, self.range_threshold, self.anchor = resolution, range_threshold, anchor
        self.slack_cells, self.device = int(slack_cells), int(device)
        self._held = {}    # key -> (the scan or its block, ym_scan*, the pose it was traced at); insertion-ordered
        self._h = None     # ym_occmap*, created on first use
        self._form = 0

    # ---- the library
    def _native(self):
        L = _capi.lib()
        if self._h is None:
            a = None if self.anchor is None else (C.c_double * 2)(*self.anchor)
            h = L.ym_occmap_create(self.device, self.resolution, self.range_threshold, a, self.slack_cells)
            if not h:
                raise _capi.YmError(-1, _capi.last_error())
            self._h = h
            if self._form:
                _capi.check(L.ym_occmap_debug_option(h, 1, self._form))
        return L, self._h

    def _accumulate(self, entries, sign):
        """entries: (ym_scan*, pose) pairs"""
        if not entries:
            return
        L, h = self._native()
        arr = (C.c_void_p * len(entries))(*[e[0] for e in entries])
        poses = np.array([e[1] for e in entries], dtype=np.float64).reshape(len(entries), 3)
        _capi.check(L.ym_occmap_accumulate(h, arr, poses.ctypes.data_as(C.POINTER(C.c_double)), len(entries), int(sign)))

    def _set_trace_form(self, form):
        """development: 0 = a wave per ray (the default), 1 = a thread per ray; same counts"""
        if form not in (0, 1):
            raise ValueError("trace form %r: 0 or 1" % (form,))
        self._form = form
        if self._h is not None:
            _capi.check(_capi.lib().ym_occmap_debug_option(self._h, 1, form))

    def close(self):
        h, self._h = getattr(self, "_h", None), None
        self._held = {}
        if h is not None:
            _capi.lib().ym_occmap_destroy(h)

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # ---- membership
    def __len__(self):
        return len(self._held)

    def __contains__(self, scan):
        return id(scan) in self._held

    def _distinct(self, scans, what):
        scans = list(scans)
        seen = set()
        for i, s in enumerate(scans):
            if not hasattr(s, "native"):
                raise ValueError("%s: element %d is not a LocalizedRangeScan" % (what, i))
            if id(s) in seen:
                raise ValueError("%s: scan %d is in the list twice" % (what, i))
            seen.add(id(s))
        return scans

    def _add(self, scans, poses):
        """distinct scans that are not held, traced at `poses`"""
        entries = [(s.native(self.device), pose) for s, pose in zip(scans, poses)]
        self._accumulate(entries, +1)
        for s, e in zip(scans, entries):
            self._held[id(s)] = (s,) + e

    def add(self, scans):
        if hasattr(scans, "handles"):  # a models.ScanBlock: its scans at their own poses
            handles = [int(v) for v in scans.handles]
            for i, v in enumerate(handles):
                if ("h", v) in self._held:
                    raise ValueError("add: scan %d of the block is already held" % i)
            if not handles:
                return
            L = _capi.lib()
            entries = []
            for v in handles:
                pose = (C.c_double * 3)()
                _capi.check(L.ym_scan_get_pose(v, pose))
                entries.append((v, tuple(pose)))
            self._accumulate(entries, +1)
            for v, pose in entries:
                self._held[("h", v)] = (scans, v, pose)
            return
        scans = self._distinct(scans, "add")
        for i, s in enumerate(scans):
            if id(s) in self._held:
                raise ValueError("add: scan %d is already held" % i)
        self._add(scans, [_pose_of(s) for s in scans])

    def remove(self, scans):
        scans = self._distinct(scans, "remove")
        for i, s in enumerate(scans):
            if id(s) not in self._held:
                raise ValueError("remove: scan %d is not held" % i)
        if not scans:
            return
        self._accumulate([self._held[id(s)][1:] for s in scans], -1)
        for s in scans:
            del self._held[id(s)]

    def clear(self):
        """no scans, zero counts, no bounding box; the anchor (once decided) and the memory stay"""
        self._held = {}
        if self._h is not None:
            _capi.check(_capi.lib().ym_occmap_clear(self._h))

    def sync(self, scans):
        """Make the grid hold exactly `scans` at their current corrected poses.  Members that have not moved are not touched,
        moved ones go out at the pose they were traced at and in at the new one; when more than half of `scans` would have to be
        traced again, everything is cleared and added instead (the same counts, a window that starts over).  Returns the route
        taken: "none", "update" or "rebuild"."""
        scans = self._distinct(scans, "sync")
        poses = [_pose_of(s) for s in scans]
        held = self._held
        target = {id(s) for s in scans}
        gone = [k for k in held if k not in target]
        fresh = [i for i, s in enumerate(scans) if id(s) not in held]
        moved = [i for i, s in enumerate(scans) if id(s) in held and held[id(s)][2] != poses[i]]
        if not gone and not fresh and not moved:
            return "none"
        if 2 * (len(fresh) + len(moved)) > len(scans) or not scans:
            self.clear()
            self._add(scans, poses)
            return "rebuild"
        out = [held[k][1:] for k in gone] + [held[id(scans[i])][1:] for i in moved]
        self._accumulate(out, -1)
        for k in gone + [id(scans[i]) for i in moved]:
            del held[k]
        self._add([scans[i] for i in moved + fresh], [poses[i] for i in moved + fresh])
        return "update"

    # ---- reading
    @property
    def info(self):
        st = _capi.YmOccmapInfo()
        L, h = self._native()
        _capi.check(L.ym_occmap_get_info(h, C.byref(st)))
        return {name: getattr(st, name) for name, _ in _capi.YmOccmapInfo._fields_}

    def _read(self, opts, counts=False):
        L, h = self._native()
        st = _capi.YmOccmapInfo()
        _capi.check(L.ym_occmap_get_info(h, C.byref(st)))
        image = np.empty((max(st.height, 0), max(st.width, 0)), dtype=np.uint8)
        stats = _capi.YmDespeckleStats()
        _capi.check(L.ym_occmap_read(h, image.ctypes.data_as(C.POINTER(C.c_uint8)), image.size,
                                     None if opts is None else C.byref(opts), C.byref(stats)))
        g = OccupancyGrid(image, Pose2(st.offset_x, st.offset_y, 0.0), st.resolution)
        if opts is not None:
            g.stats = _stats_dict(stats)
        if counts:
            g.passes, g.hits = np.empty(image.shape, dtype=np.uint32), np.empty(image.shape, dtype=np.uint32)
            u32 = C.POINTER(C.c_uint32)
            _capi.check(L.ym_occmap_read_counts(h, g.passes.ctypes.data_as(u32), g.hits.ctypes.data_as(u32), image.size))
        return g

    def grid(self, counts=False):
        """what create_occupancy_grid returns, of the window as it stands; counts=True: with `.passes` and `.hits`"""
        return self._read(None, counts)

    def clean_grid(self, min_area=5, connectivity=8):
        """what create_clean_occupancy_grid returns (`.stats` included)"""
        return self._read(_filter_opts(0, 255, min_area, connectivity))

    def ros_map(self, **filter_opts):
        """what ros_map returns: the window cleaned (filter_opts: min_area, connectivity) with the codes of nav_msgs/OccupancyGrid"""
        g = self.clean_grid(**filter_opts)
        return RosMap(ros_codes(g.image), g.offset, g.resolution, g.stats)
