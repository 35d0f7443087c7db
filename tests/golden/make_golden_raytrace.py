#!/usr/bin/env python3
"""Ray casting of the reference's "start in a prior map" path, recorded on a synthetic occupancy image:
`run_raytracing_sweep` (/root/reference/yag_slam/raytracing.py:63-92) at hand-picked and full angle lists, and
`map_to_graph`'s scans (/root/reference/yag_slam/splicing.py:82-107) for the centroids its own `determine_centroids` finds.

Run where the reference is importable (tests/refstubs.py: its location and the stand-ins for what this image lacks):

    python tests/golden/make_golden_raytrace.py

raytracing.py and splicing.py are imported unmodified.  Stand-ins added here to those of tests/refstubs.py:
  numba.experimental.jitclass  the class itself, with every field its spec declares float32 rounded to np.float32 on every
                               assignment (what numba's jitclass storage does); `.class_type.instance_type` is the class
  numba.types.float32          the marker those specs name
  skimage.segmentation         slic / mark_boundaries / find_boundaries that raise (the segmentation is not recorded)
`splicing.segment_map` is replaced by a fixed label image and `splicing.create_edges` by an empty edge list
(`find_boundaries` is absent); `determine_centroids` is the reference's own.

The map (300 x 220 pixels): free (254) with a wall on the left and bottom borders, open top, an unknown (205) band on the
right border, interior walls (boxes, a diagonal), an unknown blob, 3 x 3 squares at each of the threshold values
179, 180, 181, 209, 210, 211 and a seeded speckle of them.  The centroids: segment means with ties at .5, pixels next to
the border, one on an occupied pixel, one on an unknown pixel, one on a 210 and one on a 180 pixel.

Output: tests/golden/raytrace.npz (a data file).
"""
import os
import sys
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
sys.dont_write_bytecode = True
sys.path.insert(0, REPO)

from tests import refstubs  # noqa: E402

W, H = 300, 220
# map_to_graph's part at 0.1 m per pixel: readings from 0.1 m to beyond 20 m, so the `rng > 20 -> 100` rule meets real
# lengths (a horizontal ray across the 300-pixel map is ~30 m), not only the 1000-pixel jump
RESOLUTION = 0.1
ORIGIN = (-3.25, 1.5)
SWEEP_ANGLES = np.array([0.0, 45.0, -45.0, 90.0, -90.0, -180.0, 179.5, 180.0, 0.25, 33.3, 135.0, -112.75])


def synthetic_map():
    rng = np.random.default_rng(31)
    im = np.full((H, W), 254, dtype=np.uint8)
    im[:, 0] = 0                      # left wall
    im[H - 2:, :] = 0                 # bottom wall (the last two rows)
    im[:111, W - 20:] = 205           # unknown band on the right border
    im[30:34, 170:240] = 0            # boxes
    im[120:180, 200:204] = 0
    im[90:95, 20:60] = 0
    for k in range(80):               # a diagonal wall
        im[60 + k, 40 + k] = 0
    im[150:200, 30:90] = 205          # an unknown blob
    for i, v in enumerate((179, 180, 181, 209, 210, 211)):
        im[100:103, 150 + 8 * i:153 + 8 * i] = v
        im[10:13, 60 + 8 * i:63 + 8 * i] = v
    speck = rng.random((H, W)) < 0.006
    speck[:, :2] = False
    im[speck] = rng.choice(np.array([179, 180, 181, 209, 210, 211], dtype=np.uint8), size=int(speck.sum()))
    im[200, 150] = 180                # a viewpoint on a 180 pixel (stops, no jump)
    im[70, 260] = 210                 # and one on a 210 pixel (free)
    return im


def segment_labels(im):
    """label image: 0 = no segment, 1 .. K = segments (np.unique(...)[1:] in determine_centroids)"""
    lab = np.zeros((H, W), dtype=np.int64)
    lab[40:60, 100:140] = 1           # centroid (119.5, 49.5): ties at .5
    lab[1, 1] = 2                     # next to the top-left border
    lab[70, 50] = 3                   # on the diagonal wall: an occupied start
    lab[160, 50] = 4                  # on the unknown blob: jumps at once
    lab[120:140, 100:103] = 5         # an L shape
    lab[137:140, 103:130] = 5
    lab[200, 150] = 6                 # on a 180 pixel
    lab[70, 260] = 7                  # on a 210 pixel
    lab[218, 298] = 8                 # the bottom-right corner, on the wall
    lab[0, 150] = 9                   # the top row (open): one step
    return lab


def main():
    if not refstubs.available():
        raise SystemExit("the reference is not importable here (tests/refstubs.py)")
    refstubs.install()
    float32 = type("float32", (), {"__repr__": lambda self: "float32"})()

    def jitclass(spec):
        f32 = frozenset(name for name, typ in spec if typ is float32)

        def wrap(cls):
            def __setattr__(self, name, value):
                object.__setattr__(self, name, np.float32(value) if name in f32 else value)
            ns = {k: v for k, v in vars(cls).items() if k not in ("__dict__", "__weakref__")}
            ns["__setattr__"] = __setattr__
            new = type(cls.__name__, cls.__bases__, ns)
            new.class_type = types.SimpleNamespace(instance_type=new)
            return new
        return wrap

    numba = sys.modules["numba"]
    numba.experimental = sys.modules["numba.experimental"] = types.ModuleType("numba.experimental")
    numba.experimental.jitclass = jitclass
    numba.types = sys.modules["numba.types"] = types.ModuleType("numba.types")
    numba.types.float32 = float32

    def absent(*a, **k):
        raise NotImplementedError("scikit-image is not part of the recording")
    sk = sys.modules["skimage"] = types.ModuleType("skimage")
    sk.segmentation = sys.modules["skimage.segmentation"] = types.ModuleType("skimage.segmentation")
    sk.segmentation.slic = sk.segmentation.mark_boundaries = sk.segmentation.find_boundaries = absent

    from yag_slam import raytracing, splicing  # the reference
    im = synthetic_map()
    labels = segment_labels(im)
    splicing.segment_map = lambda imin, verbose=False, density=1: labels
    splicing.create_edges = lambda segments: []

    centroid_map = splicing.determine_centroids(labels)
    cent = np.array([centroid_map[i] for i in range(len(centroid_map))], dtype=np.float64)

    sweep_vp = np.array([[150.3, 110.7], [1.0, 1.0], [0.4, 0.6], [299.4, 219.4], [119.5, 49.5], [50.0, 70.0], [50.0, 160.0],
                         [2.5, 217.5], [264.0, 100.2]], dtype=np.float64)
    sweep = [raytracing.run_raytracing_sweep(im, SWEEP_ANGLES, sx, sy) for sx, sy in sweep_vp]
    full_vp = np.array([151.25, 108.5])
    full_angles = np.arange(-180, 180, 0.25)[:-1]
    full = raytracing.run_raytracing_sweep(im, full_angles, full_vp[0], full_vp[1])

    scans, edges = splicing.map_to_graph(im, RESOLUTION, list(ORIGIN), density=5)
    assert edges == [] and len(scans) == len(cent)
    s0 = scans[0]
    out = dict(
        image=im, resolution=np.float64(RESOLUTION), origin=np.array(ORIGIN, dtype=np.float64), centroids=cent,
        sweep_viewpoints=sweep_vp, sweep_angles=SWEEP_ANGLES,
        sweep_ends=np.array([[r.end.val for r in rs] for rs in sweep], dtype=np.float32),
        sweep_lengths=np.array([[r.length for r in rs] for rs in sweep], dtype=np.float64),
        sweep_cs=np.array([[np.cos(np.deg2rad(a)), np.sin(np.deg2rad(a))] for a in SWEEP_ANGLES], dtype=np.float64),
        full_viewpoint=full_vp, full_angles=full_angles,
        full_ends=np.array([r.end.val for r in full], dtype=np.float32),
        full_lengths=np.array([r.length for r in full], dtype=np.float64),
        graph_ranges=np.array([s.ranges for s in scans], dtype=np.float64),
        graph_poses=np.array([(s.corrected_pose.x, s.corrected_pose.y, s.corrected_pose.euler[-1]) for s in scans], dtype=np.float64),
        graph_nums=np.array([s.num for s in scans], dtype=np.int64),
        graph_sensor=np.array([s0.min_angle, s0.max_angle, s0.angle_increment, s0.min_range, s0.max_range, s0.range_threshold],
                              dtype=np.float64),
    )
    path = os.path.join(HERE, "raytrace.npz")
    np.savez_compressed(path, **out)
    print("raytrace.npz: %d bytes, %d centroids, %d sweep viewpoints" % (os.path.getsize(path), len(cent), len(sweep_vp)))


if __name__ == "__main__":
    main()
