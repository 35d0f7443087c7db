"""Virtual scans ray-traced from an occupancy map on the device: the scan loop of the ROS node's "start in a prior map" path
(`ingest_base_map` -> `map_to_graphslam` -> `map_to_graph`, /root/reference/ros1/slam_node_ros1:131-147,
/root/reference/yag_slam/splicing.py:82-107), whose rays the reference casts one pixel at a time in numba
(/root/reference/yag_slam/raytracing.py:63-92).  Here every (viewpoint, angle) pair of a call walks in one kernel launch
(include/yagmatch.h, ym_raymap_*), bit for bit the walk of `trace_ray`, and the scans' device twins are created in one call.

The segmentation (`segment_map`: SLIC from scikit-image, OpenCV morphology) and `create_edges` stay with the caller: they are
CPU image work.  Their output, the segment centroids, is what `virtual_scans` takes.

Frames.  `layout="reference"` reproduces `map_to_graph` exactly, quirks included: the image is the one the node passes
(`cv2.imread(...)[::-1, :, 0]`, slam_node_ros1:138, so row 0 is the lowest y), the pose is `pixel_to_meters` of the centroid
(`(x res + ox, (h - y) res + oy)`, heading 0), and reading i is the ray cast at `angles[::-1][i]` = 179.5 - 0.25 i degrees
while the scan's sensor says -180 + 0.25 i.  What holds (tests/test_raytrace_host.py checks it on the fixture's map):
the scans are those of the map MIRRORED about a horizontal line -- pose y = oy + (h - y) res is the mirror of the image
row's own y = oy + y res about y = oy + h res / 2, and the traced direction 179.5 - 0.25 i is the mirror of the sensor's
beam angle shifted by half a degree: in the mirrored map, reading i lies along -180 + 0.25 i + 0.5 degrees, so every scan
is a scan of the mirrored map taken at heading +0.5 degrees and filed at heading 0 (and, with cell centres at oy + y res,
placed one cell higher than the mirror of its centroid, whose row the mirrored image holds at h - 1 - y).  On the
fixture's map 99.9 % of the readings agree with that mirrored walk to 1.5 pixels; the float32 walk is not exactly
mirror-symmetric.  Each scan holds 1439 readings while its min / max / increment describe 1440.

`layout="world"` is for maps in this package's own frame (`occupancy.create_occupancy_grid`: image[row][col], row 0 the
lowest y, cell (0, 0) at `origin` = the grid's `.offset`).  Cell (col, row) is CENTRED at (ox + col res, oy + row res) --
Karto's world -> grid rounding (`world_to_grid`), so a world point (x, y) is pixel ((x - ox) / res, (y - oy) / res) and the
walk's rint finds its cell (ties, exactly half a cell off a centre, round to even where Karto rounds away from zero).
Viewpoints are (x, y, heading) in metres (`world_to_pixels`), reading i is cast along heading + min_angle + i increment
(every viewpoint its own directions, all viewpoints in one launch: `ym_raymap_trace_each`), range = length res.
A ray ends one step past the first occupied pixel it meets (the reference's rule), so a range overshoots the wall's cell
centre by about one cell; a ray that meets an unknown pixel jumps 1000 pixels and returns a range far beyond any range
threshold, i.e. no reading.
"""
import ctypes as C
from collections.abc import Mapping

import numpy as np

from . import _capi
from .models import LocalizedRangeScan, ScanBlock, native_many

# map_to_graph's angle list (splicing.py:86): -180 .. 179.5 degrees, 1439 values; its rays are cast in reversed order
REFERENCE_ANGLES = np.arange(-180, 180, 0.25)[:-1]
# its virtual sensor (splicing.py:102): min_angle, max_angle, angle_increment, min_range, max_range, range_threshold
REFERENCE_SENSOR = (-np.pi, np.pi - np.deg2rad(0.25), np.deg2rad(0.25), 0, 30, 20)
# ranges above this (metres) become REFERENCE_NO_HIT (splicing.py:93-95)
REFERENCE_MAX_RANGE, REFERENCE_NO_HIT = 20, 100


def pixel_to_meters(resolution, origin, h, x, y):
    """pixel (x = column, y = row) of an image of h rows -> metres, as the reference converts (splicing.py:29-30)"""
    return (x * resolution) + origin[0], ((h - y) * resolution) + origin[1]


def direction_table(angles_deg):
    """(cos, sin) per angle in degrees, computed as trace_ray does (np.deg2rad, then np.cos / np.sin in float64): [n][2]"""
    a = np.deg2rad(np.asarray(angles_deg, dtype=np.float64).reshape(-1))
    return np.ascontiguousarray(np.stack([np.cos(a), np.sin(a)], axis=1))


class RayMap(object):
    """An occupancy image (uint8, [rows][cols]; x = column, y = row) resident on one device, for many ray sweeps.
    `trace` is `run_raytracing_sweep(image, angles, sx, sy)` (raytracing.py:91-92) for many viewpoints in one launch."""

    def __init__(self, image, device=0):
        im = np.asarray(image)
        if im.ndim != 2 or im.dtype != np.uint8:
            raise ValueError("RayMap: a 2-D uint8 image, got %s %s" % (im.dtype, im.shape))
        if im.strides[1] != 1 or im.strides[0] < im.shape[1]:
            im = np.ascontiguousarray(im)
        self.height, self.width = im.shape
        self.device = int(device)
        self._h = None
        h = _capi.lib().ym_raymap_create(self.device, im.ctypes.data_as(C.POINTER(C.c_uint8)), self.width, self.height,
                                         int(im.strides[0]))
        if not h:
            raise _capi.YmError(-1, _capi.last_error())
        self._h = h
        self.capped = 0  # rays of the last trace that reached the iteration cap (0 on every valid input)

    def _trace(self, fn, st, dc, n_angles):
        if self._h is None:
            raise ValueError("RayMap is closed")
        ends = np.empty((st.shape[0], n_angles, 2), dtype=np.float32)
        lengths = np.empty((st.shape[0], n_angles), dtype=np.float64)
        capped = C.c_int64(0)
        dp = C.POINTER(C.c_double)
        _capi.check(fn(self._h, st.ctypes.data_as(dp), st.shape[0], dc.ctypes.data_as(dp), n_angles,
                       ends.ctypes.data_as(C.POINTER(C.c_float)), lengths.ctypes.data_as(dp), C.byref(capped)))
        self.capped = int(capped.value)
        return ends, lengths

    def trace_dirs(self, viewpoints_px, dir_cs):
        """viewpoints_px [n][2] (x, y) pixels, dir_cs [a][2] unit (cos, sin) -> (ends [n, a, 2] float32, lengths [n, a] float64)"""
        st = np.ascontiguousarray(viewpoints_px, dtype=np.float64).reshape(-1, 2)
        dc = np.ascontiguousarray(dir_cs, dtype=np.float64).reshape(-1, 2)
        return self._trace(_capi.lib().ym_raymap_trace, st, dc, dc.shape[0])

    def trace_each(self, viewpoints_px, dir_cs):
        """a direction table per viewpoint in one launch: dir_cs [n][a][2] -> (ends [n, a, 2], lengths [n, a])"""
        st = np.ascontiguousarray(viewpoints_px, dtype=np.float64).reshape(-1, 2)
        dc = np.ascontiguousarray(dir_cs, dtype=np.float64)
        if dc.ndim != 3 or dc.shape[0] != st.shape[0] or dc.shape[2] != 2:
            raise ValueError("trace_each: dir_cs [%d][angles][2], got %s" % (st.shape[0], dc.shape))
        return self._trace(_capi.lib().ym_raymap_trace_each, st, dc, dc.shape[1])

    def trace(self, viewpoints_px, angles_deg):
        """rays from every viewpoint at every angle (degrees, the reference's convention) -> (ends, lengths)"""
        return self.trace_dirs(viewpoints_px, direction_table(angles_deg))

    def close(self):
        if getattr(self, "_h", None) is not None:
            _capi.lib().ym_raymap_destroy(self._h)
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


def trace_rays(image, angles_deg, viewpoints_px, device=0):
    """run_raytracing_sweep(image, angles, sx, sy) for every (sx, sy) of viewpoints_px at once -> (ends, lengths)"""
    with RayMap(image, device) as rm:
        out = rm.trace(viewpoints_px, angles_deg)
        _check_capped(rm)
        return out


def _check_capped(rm):
    # the walk provably leaves the image within its step cap (ym_k_raytrace.hpp); a capped ray is a library fault
    if rm.capped:
        raise RuntimeError("%d rays reached the iteration cap of the walk" % rm.capped)


def _centroid_list(centroids):
    """determine_centroids' dict {index: (x, y)} (map_to_graph reads centroid_map[0 .. len - 1]) or a sequence of (x, y)"""
    if isinstance(centroids, Mapping):
        return [centroids[i] for i in range(len(centroids))]
    return [tuple(c) for c in centroids]


def _reference_ranges(map_image, resolution, centroids, device):
    pts = np.array([(float(c[0]), float(c[1])) for c in centroids], dtype=np.float64).reshape(-1, 2)
    _, lengths = trace_rays(map_image, REFERENCE_ANGLES[::-1], pts, device)  # (raises on a capped ray)
    ranges = lengths * resolution
    ranges[ranges > REFERENCE_MAX_RANGE] = REFERENCE_NO_HIT
    return pts, ranges


def world_to_pixels(resolution, origin, x, y):
    """metres -> the walk's pixel units in this package's frame: cell (col, row) is centred at (ox + col res, oy + row res)"""
    return (np.asarray(x, dtype=np.float64) - origin[0]) / resolution, (np.asarray(y, dtype=np.float64) - origin[1]) / resolution


def _world_ranges(map_image, resolution, origin, viewpoints, sensor, n_beams, device):
    vp = np.asarray(viewpoints, dtype=np.float64).reshape(-1, 3)
    pts = np.stack(world_to_pixels(resolution, origin, vp[:, 0], vp[:, 1]), axis=1)
    # every viewpoint its own beam directions (heading + min_angle + i increment), all in one launch
    a = vp[:, 2:3] + (sensor[0] + np.arange(n_beams) * sensor[2])[None, :]
    with RayMap(map_image, device) as rm:
        _, lengths = rm.trace_each(pts, np.stack([np.cos(a), np.sin(a)], axis=2))
        _check_capped(rm)
    return vp, lengths * resolution


def virtual_scans(map_image, resolution, origin, centroids, layout="reference", device=0, sensor=None, n_beams=1439):
    """Virtual LocalizedRangeScans of an occupancy image, their device twins created in one call.

    layout="reference": map_to_graph's scan loop (splicing.py:87-107) for the caller's centroids (determine_centroids'
        dict, or (x, y) pixel pairs): scan i at pixel_to_meters(centroid i), heading 0, readings = the reversed sweep's
        lengths x resolution with > 20 -> 100, the reference's sensor, num = i.  Bit for bit the reference's ranges up to
        its float32 length (see the module text for the frame it implies).
    layout="world": maps in this package's frame (module text); centroids = viewpoints (x, y, heading) in metres,
        sensor = (min_angle, max_angle, angle_increment, min_range, max_range, range_threshold) (default: the reference's
        virtual sensor), n_beams readings along heading + min_angle + i increment, range = length x resolution."""
    sensor = tuple(REFERENCE_SENSOR if sensor is None else sensor)
    im = np.asarray(map_image)
    if layout == "reference":
        pts, ranges = _reference_ranges(im, resolution, _centroid_list(centroids), device)
        scans = []
        for i, (p, r) in enumerate(zip(pts, ranges)):
            x, y = pixel_to_meters(resolution, origin, im.shape[0], p[0], p[1])
            s = LocalizedRangeScan(r, *REFERENCE_SENSOR, x, y, 0)
            s.num = i
            scans.append(s)
    elif layout == "world":
        vp, ranges = _world_ranges(im, resolution, origin, centroids, sensor, n_beams, device)
        scans = []
        for i, (p, r) in enumerate(zip(vp, ranges)):
            s = LocalizedRangeScan(r, *sensor, p[0], p[1], p[2])
            s.num = i
            scans.append(s)
    else:
        raise ValueError("layout: 'reference' or 'world', got %r" % (layout,))
    native_many(scans, device)
    return scans


def virtual_scan_block(map_image, resolution, origin, viewpoints, layout="reference", device=0, sensor=None, n_beams=1439):
    """The scans of `virtual_scans` as one ScanBlock (device twins from arrays, no Python object per scan): for thousands of
    pose hypotheses (layout="world": one launch whatever their headings, then one ym_scans_create).  Returns the block; its
    `.ranges` [n][beams] and `.poses` [n][3] are kept on it."""
    im = np.asarray(map_image)
    if layout == "reference":
        pts, ranges = _reference_ranges(im, resolution, _centroid_list(viewpoints), device)
        xy = [pixel_to_meters(resolution, origin, im.shape[0], p[0], p[1]) for p in pts]
        poses = np.array([(x, y, 0.0) for x, y in xy], dtype=np.float64).reshape(-1, 3)
        sensor = REFERENCE_SENSOR
    elif layout == "world":
        sensor = tuple(REFERENCE_SENSOR if sensor is None else sensor)
        poses, ranges = _world_ranges(im, resolution, origin, viewpoints, sensor, n_beams, device)
    else:
        raise ValueError("layout: 'reference' or 'world', got %r" % (layout,))
    block = ScanBlock(ranges, poses, sensor, device)
    block.ranges, block.poses = ranges, poses
    return block
