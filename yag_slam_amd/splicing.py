"""Virtual scans ray-traced from an occupancy map on the device: the scan loop of the ROS node's "start in a prior map" path
(`ingest_base_map` -> `map_to_graphslam` -> `map_to_graph`, /root/reference/ros1/slam_node_ros1:131-147,
/root/reference/yag_slam/splicing.py:82-107), whose rays the reference casts one pixel at a time in numba
(/root/reference/yag_slam/raytracing.py:63-92).  Here every (viewpoint, angle) pair of a call walks in one kernel launch
(include/yagmatch.h, ym_raymap_*), bit for bit the walk of `trace_ray`, and the scans' device twins are created in one call.

The segmentation (`segment_map`; the reference's is OpenCV morphology and SLIC from scikit-image) runs on the device too
(`free_space`, `SegmentMap.from_map`, ym_segments_from_map): the threshold and the grey closing are the reference's bit for
bit, the superpixel step is this package's own spatial k-means on the free pixels ("Map segmenter": not
scikit-image's SLIC; a free pixel in a fragment below the minimum size ends up in no segment).  `map_to_graph` takes a
caller's label image or, with `segments=None`, segments the map itself and goes on with the resident label image:
`segment_centroids` (the reference's `determine_centroids`) and `segment_edges` (its `create_edges`, `find_boundaries`
included) are one pass over the label image each on the device (ym_segments_*), and `map_to_graphslam` puts the scans and
edges into an empty `mapping.LoopClosingMapper`.

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


class SegmentError(_capi.YmError, ValueError):
    """the map segmenter refused its input (an image that yields no segment is a ValueError) or the library failed"""


class SegmentMap(object):
    """A label image ([rows][cols], any integer dtype; x = column, y = row; 0 = no segment, 1 .. K = segments) resident on
    one device.  It is converted once to int32 (a contiguous copy unless it already is int32 with unit column stride)."""

    def __init__(self, segments, device=0):
        seg = _label_image(segments)
        self.height, self.width = seg.shape
        self.device = int(device)
        self._h = None
        h = _capi.lib().ym_segments_create(self.device, seg.ctypes.data_as(C.POINTER(C.c_int32)), self.width, self.height,
                                           seg.strides[0] // 4)
        if not h:
            raise _capi.YmError(-1, _capi.last_error())
        self._h = h

    @classmethod
    def from_map(cls, map_image, density=1, device=0, n_segments=0, close_size=11, iterations=10, min_size_div=4, stage="final"):
        """The map segmenter ("Map segmenter"): the label image of an occupancy image (uint8; free = 254 / 255),
        computed and kept on the device.  n_segments=0: the reference's rule, int(sum of the closed image // 600000 * density).
        stage="assigned" keeps centre index + 1 of every pixel, the state before the components (a test hook).  `.info` holds
        sum, n_free, n_segments, step, seeds, segments, iterations_run, min_size, unlabelled.  Raises SegmentError (a
        ValueError) on an image that yields no segment."""
        im = _map_image(map_image)
        opts = _capi.YmSegmentOpts(int(n_segments), float(density), int(close_size), int(iterations), int(min_size_div),
                                   _capi.SEGMENT_STAGES[stage])
        info = _capi.YmSegmentInfo()
        h = _capi.lib().ym_segments_from_map(int(device), im.ctypes.data_as(C.POINTER(C.c_uint8)), im.shape[1], im.shape[0],
                                             int(im.strides[0]), C.byref(opts), C.byref(info))
        if not h:
            raise SegmentError(-1, _capi.last_error())
        self = cls.__new__(cls)
        self.height, self.width = im.shape
        self.device = int(device)
        self._h = h
        self.info = {name: int(getattr(info, name)) for name, _ in _capi.YmSegmentInfo._fields_}
        return self

    def _handle(self):
        if self._h is None:
            raise ValueError("SegmentMap is closed")
        return self._h

    def labels(self):
        """the resident label image as int32 [rows][cols]"""
        out = np.empty((self.height, self.width), dtype=np.int32)
        _capi.check(_capi.lib().ym_segments_labels(self._handle(), out.ctypes.data_as(C.POINTER(C.c_int32)), out.size))
        return out

    def label_range(self):
        """(smallest, largest) label of the image"""
        lo, hi = C.c_int32(0), C.c_int32(0)
        _capi.check(_capi.lib().ym_segments_label_range(self._handle(), C.byref(lo), C.byref(hi)))
        return int(lo.value), int(hi.value)

    def stats(self, n_labels):
        """(count, sum_x, sum_y), int64 [n_labels] indexed by label; every label must lie in [0, n_labels)"""
        out = [np.zeros(int(n_labels), dtype=np.int64) for _ in range(3)]
        lp = C.POINTER(C.c_int64)
        _capi.check(_capi.lib().ym_segments_stats(self._handle(), int(n_labels), *[o.ctypes.data_as(lp) for o in out]))
        return tuple(out)

    def boundaries(self):
        """skimage.segmentation.find_boundaries(segments) with its defaults, as a bool image"""
        mask = np.zeros((self.height, self.width), dtype=np.uint8)
        _capi.check(_capi.lib().ym_segments_boundaries(self._handle(), mask.ctypes.data_as(C.POINTER(C.c_uint8)), mask.size))
        return mask.astype(bool)

    def pairs(self, table_slots=0, cap=1 << 16):
        """create_edges' table: (pairs int32 [n][2] of (a - 1, b - 1), counts int32 [n], first_index int64 [n]) in the order
        the reference's dict holds them.  table_slots: the first size of the device hash table (0: the library's)."""
        ip = C.POINTER(C.c_int32)
        while True:
            pairs = np.zeros((cap, 2), dtype=np.int32)
            counts = np.zeros(cap, dtype=np.int32)
            first = np.zeros(cap, dtype=np.int64)
            n = C.c_int32(-1)
            rc = _capi.lib().ym_segments_pairs(self._handle(), int(table_slots), cap, pairs.ctypes.data_as(ip), counts.ctypes.data_as(ip),
                                               first.ctypes.data_as(C.POINTER(C.c_int64)), C.byref(n))
            if rc != _capi.YM_OK and n.value > cap:  # the arrays were too short: n says how long they must be
                cap = int(n.value)
                continue
            _capi.check(rc)
            return pairs[:n.value], counts[:n.value], first[:n.value]

    def close(self):
        if getattr(self, "_h", None) is not None:
            _capi.lib().ym_segments_destroy(self._h)
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


def _map_image(map_image):
    """the occupancy image as uint8 with unit column stride (a strided view is passed as it is, by its pitch)"""
    im = np.asarray(map_image)
    if im.ndim != 2 or im.dtype != np.uint8 or im.size == 0:
        raise ValueError("map_image: a non-empty 2-D uint8 image, got %s %s" % (im.dtype, im.shape))
    if im.strides[1] != 1 or im.strides[0] < im.shape[1]:
        im = np.ascontiguousarray(im)
    return im


def free_space(map_image, close_size=11, device=0):
    """The pre-processing of the reference's segment_map (splicing.py:33-44), bit for bit: pixels < 254 -> 0, then the grey
    closing of 255 - image with a close_size x close_size square, inverted back -> (closed uint8, its sum, its non-zero
    pixels).  Pixels outside the image take no part in a window (OpenCV's default border for morphology)."""
    im = _map_image(map_image)
    closed = np.empty(im.shape, dtype=np.uint8)
    total, n_free = C.c_int64(0), C.c_int64(0)
    bp = C.POINTER(C.c_uint8)
    _capi.check(_capi.lib().ym_map_free_space(int(device), im.ctypes.data_as(bp), im.shape[1], im.shape[0], int(im.strides[0]),
                                              int(close_size), closed.ctypes.data_as(bp), C.byref(total), C.byref(n_free)))
    return closed, int(total.value), int(n_free.value)


def segment_map(map_image, density=1, device=0, **opts):
    """The reference's segment_map (splicing.py:32-55) on the device -> int32 label image, 0 = no segment, 1 .. K.  The
    pre-processing is the reference's; the superpixels are `SegmentMap.from_map`'s (its keyword options pass through)."""
    with SegmentMap.from_map(map_image, density=density, device=device, **opts) as sm:
        return sm.labels()


def _label_image(segments):
    """the label image as int32 with unit column stride and a row stride of whole elements (one conversion at most)"""
    seg = np.asarray(segments)
    if seg.ndim != 2 or seg.dtype.kind not in "iu" or seg.size == 0:
        raise ValueError("segments: a non-empty 2-D integer label image, got %s %s" % (seg.dtype, seg.shape))
    if seg.shape[0] > 65536 or seg.shape[1] > 65536:
        raise ValueError("segments: %d x %d pixels, at most 65536 x 65536" % (seg.shape[1], seg.shape[0]))
    if seg.dtype == np.int32 and seg.strides[1] == 4 and seg.strides[0] >= 4 * seg.shape[1] and seg.strides[0] % 4 == 0:
        return seg
    if not np.can_cast(seg.dtype, np.int32) and (int(seg.max()) > np.iinfo(np.int32).max or int(seg.min()) < np.iinfo(np.int32).min):
        raise ValueError("segments: labels beyond int32")
    return np.ascontiguousarray(seg, dtype=np.int32)


def _checked_stats(sm):
    """the statistics of labels 0 .. K, after the checks the reference's indexing implies: determine_centroids drops the
    SMALLEST label present whatever it is (np.unique(...)[1:]) and map_to_graph reads centroid_map[0 .. K - 1], so label 0 must
    occur and 1 .. K must all be present.  Checked on the device's label range and counts."""
    lo, hi = sm.label_range()
    if lo < 0:
        raise ValueError("segments: a negative label (%d); labels are 0 (no segment) and 1 .. K" % lo)
    if hi > sm.width * sm.height - 1:
        raise ValueError("segments: a gap in the labels (largest label %d in an image of %d pixels)" % (hi, sm.width * sm.height))
    count, sum_x, sum_y = sm.stats(hi + 1)
    if count[0] == 0:
        raise ValueError("segments: no pixel holds label 0; the reference drops the smallest label present, which would be "
                         "segment %d" % lo)
    missing = np.flatnonzero(count[1:] == 0)
    if missing.size:
        raise ValueError("segments: a gap in the labels (label %d of 1 .. %d does not occur)" % (missing[0] + 1, hi))
    return count, sum_x, sum_y


def _checked_pairs(sm):
    lo, _ = sm.label_range()
    if lo < 0:
        raise ValueError("segments: a negative label (%d); labels are 0 (no segment) and 1 .. K" % lo)
    return sm.pairs()


def _centroids_of(stats):
    count, sum_x, sum_y = stats
    # one correctly rounded float64 division of exact integers: np.mean of the integer coordinate arrays, bit for bit
    cx, cy = sum_x[1:] / count[1:], sum_y[1:] / count[1:]
    return dict(enumerate(zip(cx.tolist(), cy.tolist())))


def _edges_of(table, min_count):
    pairs, counts, _ = table
    return list(map(tuple, pairs[counts > min_count].tolist()))


def segment_centroids(segments, device=0):
    """determine_centroids (splicing.py:57-65): {index: (x, y)}, index = label - 1, (x, y) the mean column and row of the
    label's pixels as np.mean gives them.  Raises ValueError when the labels are not 0 and every one of 1 .. K."""
    with SegmentMap(segments, device) as sm:
        return _centroids_of(_checked_stats(sm))


def segment_edges(segments, device=0, min_count=3):
    """create_edges (splicing.py:67-80): the (a, b) index pairs, a < b, whose segments share more than `min_count` boundary
    pixels with exactly the two of them in the 4 x 4 window, in the reference's order.  Raises ValueError on a negative label."""
    with SegmentMap(segments, device) as sm:
        return _edges_of(_checked_pairs(sm), min_count)


def map_to_graph(map_image, resolution, origin, segments=None, layout="reference", device=0, density=1):
    """The reference's map_to_graph (splicing.py:82-107): -> (scans, edges), scan i the virtual scan at the centroid of
    label i + 1 (`virtual_scans`), edges as `segment_edges`.  segments=None: the map is segmented on the device
    (`SegmentMap.from_map(map_image, density)`, the reference's `segment_map(map_image, density)` step) and centroids and
    edges run on the resident label image; otherwise `segments` is the caller's label image.
    layout="world": the viewpoint of centroid pixel (x, y) is (ox + x res, oy + y res, 0), the frame of the module text."""
    im = np.asarray(map_image)
    if layout not in ("reference", "world"):
        raise ValueError("layout: 'reference' or 'world', got %r" % (layout,))
    if segments is not None and np.shape(segments) != im.shape:
        raise ValueError("segments %s and map_image %s differ in shape" % (np.shape(segments), im.shape))
    with (SegmentMap.from_map(im, density=density, device=device) if segments is None else SegmentMap(segments, device)) as sm:
        centroids = _centroids_of(_checked_stats(sm))
        edges = _edges_of(_checked_pairs(sm), 3)
    if layout == "world":
        centroids = [(origin[0] + x * resolution, origin[1] + y * resolution, 0.0) for x, y in _centroid_list(centroids)]
    return virtual_scans(im, resolution, origin, centroids, layout=layout, device=device), edges


def map_to_graphslam(mapper, map_image, resolution, origin, segments=None, layout="reference", device=0, density=1, hold=False):
    """map_to_graphslam (splicing.py:109-126) into an EMPTY `mapping.LoopClosingMapper`: `add_vertex` for every scan of
    `map_to_graph` in order, `link_scans(scan[a], scan[b], identity * 1e-12)` for every edge; `running_scans` stays empty, so
    the first live scan goes through `mapper.splice_first_scan`.  All scans stay: the reference's "get rid of any nodes that
    did not have edges" assigns an attribute (`slam_fake.vertices`) that nothing reads, and its renumbering over
    `graph.vertices` is the identity -- no vertex is removed there, and none is here.  Returns the mapper.
    hold=True (not in the reference) holds every vertex added here through `mapper.hold_vertices`, after adding them: the
    prior map stays where it is and a later closure re-poses the robot's own scans only.  It needs a mapper whose optimizer
    has `hold` (`posegraph.PoseGraphOptimizer`); without one it raises ValueError before anything is added."""
    if mapper.scans or mapper.running_scans:
        raise ValueError("map_to_graphslam: the mapper already holds %d vertices and %d running scans; it must be empty"
                         % (len(mapper.scans), len(mapper.running_scans)))
    if hold and not hasattr(getattr(mapper, "opt", None), "hold"):
        raise ValueError("map_to_graphslam: hold=True needs a mapper with an optimizer that has hold()")
    more = {"density": density} if density != 1 else {}  # (the default is map_to_graph's own)
    scans, edges = map_to_graph(map_image, resolution, origin, segments, layout=layout, device=device, **more)
    for scan in scans:
        mapper.add_vertex(scan)
    for a, b in edges:
        mapper.link_scans(scans[a], scans[b], np.identity(3) * 1e-12)
    if hold:
        mapper.hold_vertices(scans)
    return mapper
