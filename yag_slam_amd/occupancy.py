"""Occupancy-grid rendering: drop-in for `karto_scanmatcher.create_occupancy_grid(scans, resolution, range_threshold)`
as yag-slam calls it (/root/reference/yag_slam/graph_slam.py:341-342, /root/reference/ros1/slam_node_ros1:187-202,
/root/reference/yag_slam/helpers.py:595-603).  The returned object has what those callers touch: `.image` (uint8,
[height][width], 0 occupied / 200 unknown / 255 free), `.width`, `.height`, `.offset` (`.x`, `.y`: world position of
cell (0, 0)).  Rendered on the device from the scans' resident twins (include/yagmatch.h, ym_occupancy_*).  The wheel's
algorithm is not in the reference tree: restated from open_karto's OccupancyGrid, parity unpinned.

The map the ROS node publishes (slam_node_ros1:187-212, `_make_map`) is that grid with its specks removed and its codes
rewritten: `despeckle`, `create_clean_occupancy_grid`, `ros_codes` and `ros_map` give it with nothing but this package
installed (the filter runs on the device, ym_image_despeckle / ym_occupancy_create_clean)."""
import ctypes as C

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
