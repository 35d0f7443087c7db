#!/usr/bin/env python3
"""The segment graph of the reference's "start in a prior map" path, recorded on synthetic label images:
`determine_centroids` and `create_edges` (/root/reference/yag_slam/splicing.py:57-80), the two parts of `map_to_graph` that
tests/golden/make_golden_raytrace.py left out.

Run where the reference is importable (tests/refstubs.py: its location and the stand-ins for what this image lacks):

    python tests/golden/make_golden_segments.py

splicing.py is imported unmodified.  Stand-ins added here to those of tests/refstubs.py: the `numba.experimental` and
`numba.types` stand-ins of make_golden_raytrace.py (raytracing.py needs them at import), and
  skimage.segmentation.find_boundaries   scikit-image is not installed here.  The stand-in restates the library's documented
                                         behaviour for its defaults (connectivity=1, mode="thick"): a pixel is a boundary
                                         pixel when grey dilation and grey erosion of the label image over the cross-shaped
                                         footprint (the pixel and its 4 neighbours, neighbours outside the image ignored)
                                         differ.  Written with scipy.ndimage; label 0 takes part like any other value.
  skimage.segmentation.slic / mark_boundaries   raise (the segmentation is not recorded)

Recorded per label image (cases `names`): the labels, the stand-in's boundary mask, determine_centroids' dict as an array
[K][2], create_edges' list (the reference's own window loop), per-label count / sum_x / sum_y, and the full pair table
(pairs, counts, first raster index, in the order of the first index) from a loop of this script's own that states the window
rule of include/yagmatch.h (ym_segments_pairs); the script asserts that this table's pairs with count > 3 are create_edges'
list, order included.  On images of fewer than 4 rows or columns the reference's slice [y-2:y+2] with a negative start wraps
and is not empty; the 3 x 3 case is chosen so that both readings give the same (empty) edge list.

Output: tests/golden/segments.npz (a data file).
"""
import os
import sys
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
sys.dont_write_bytecode = True
sys.path.insert(0, REPO)
sys.path.insert(0, HERE)

from tests import refstubs  # noqa: E402


def find_boundaries(label_img, connectivity=1, mode="thick", background=0):
    from scipy import ndimage
    assert connectivity == 1 and mode == "thick"
    cross = ndimage.generate_binary_structure(label_img.ndim, 1)
    # mode="nearest" repeats the border pixel: a neighbour outside the image never changes the maximum or the minimum
    return ndimage.grey_dilation(label_img, footprint=cross, mode="nearest") != ndimage.grey_erosion(label_img, footprint=cross, mode="nearest")


def walled_partition(h, w, n_seeds, seed):
    """the nearest-seed partition cut by walls of zeros 1, 2 and 3 pixels wide (and one short of the border)"""
    from yag_slam_amd.synth import seeded_partition
    lab = seeded_partition(h, w, n_seeds, seed).astype(np.int64)
    lab[:, w // 4] = 0
    lab[h // 3:h // 3 + 2, :] = 0
    lab[: h - 7, (2 * w) // 3:(2 * w) // 3 + 3] = 0
    return lab


def pair_table(lab):
    """the window rule as include/yagmatch.h states it -> (pairs [n][2], counts [n], first [n]) by first index, and the number
    of windows with three or more labels"""
    h, w = lab.shape
    mask = find_boundaries(lab)
    table, crowded = {}, 0
    for y, x in zip(*np.where(mask)):
        if y < 2 or x < 2:
            continue
        u = [int(v) for v in np.unique(lab[y - 2:y + 2, x - 2:x + 2]) if v]
        crowded += len(u) >= 3
        if len(u) == 2:
            e = table.setdefault((u[0] - 1, u[1] - 1), [0, int(y) * w + int(x)])
            e[0] += 1
    keys = list(table)
    return (np.array(keys, dtype=np.int32).reshape(-1, 2), np.array([table[k][0] for k in keys], dtype=np.int32),
            np.array([table[k][1] for k in keys], dtype=np.int64), crowded)


def cases():
    import make_golden_raytrace
    out = {}
    out["walls"] = walled_partition(160, 200, 60, 11)                    # 200 x 160, 60 seeds
    out["small"] = walled_partition(64, 64, 5, 3)
    out["raytrace"] = make_golden_raytrace.segment_labels(None)         # single-pixel segments, one at (1, 1), ties at .5
    from yag_slam_amd.synth import seeded_partition
    b = seeded_partition(90, 130, 24, 8).astype(np.int64)                # segments touch every border; zeros inside
    b[30:50, 40:90] = 0
    out["borders"] = b
    out["one"] = np.zeros((1, 1), dtype=np.int64)                        # label 0 alone: no segments
    out["three"] = np.array([[1, 1, 2], [1, 1, 2], [0, 1, 2]], dtype=np.int64)
    return out


def reference_splicing():
    """the reference's splicing module, imported unmodified behind the stand-ins of the module text"""
    if not refstubs.available():
        raise SystemExit("the reference is not importable here (tests/refstubs.py)")
    refstubs.install()
    numba = sys.modules["numba"]
    numba.experimental = sys.modules["numba.experimental"] = types.ModuleType("numba.experimental")
    numba.experimental.jitclass = lambda spec: (lambda cls: setattr(cls, "class_type", types.SimpleNamespace(instance_type=cls)) or cls)
    numba.types = sys.modules["numba.types"] = types.ModuleType("numba.types")
    numba.types.float32 = object()

    def absent(*a, **k):
        raise NotImplementedError("the segmentation is not part of the recording")
    sk = sys.modules["skimage"] = types.ModuleType("skimage")
    sk.segmentation = sys.modules["skimage.segmentation"] = types.ModuleType("skimage.segmentation")
    sk.segmentation.slic = sk.segmentation.mark_boundaries = absent
    sk.segmentation.find_boundaries = find_boundaries
    from yag_slam import splicing  # the reference
    return splicing


def main():
    splicing = reference_splicing()
    out = {}
    names = []
    for name, lab in cases().items():
        names.append(name)
        centroid_map = splicing.determine_centroids(lab)
        assert sorted(int(k) for k in centroid_map) == list(range(len(centroid_map)))
        cent = np.array([centroid_map[i] for i in range(len(centroid_map))], dtype=np.float64).reshape(-1, 2)
        edges = np.array(splicing.create_edges(lab), dtype=np.int32).reshape(-1, 2)
        pairs, counts, first, crowded = pair_table(lab)
        assert np.array_equal(pairs[counts > 3], edges), name
        assert (np.diff(first) > 0).all()
        k = int(lab.max())
        mask = find_boundaries(lab)
        early = int(mask[:2, :].sum() + mask[2:, :2].sum())
        if name == "walls":
            assert {2, 3, 4} <= set(counts.tolist()), sorted(set(counts.tolist()))  # the `> 3` rule is met from both sides
            assert crowded == 652 and early == 57, (crowded, early)  # windows with >= 3 labels; boundary pixels in rows / columns 0-1
        print("%-9s %3d x %3d  K = %3d  pairs %3d  edges %3d  windows with >= 3 labels %4d  boundary pixels in rows / columns 0-1 %3d"
              % (name, lab.shape[1], lab.shape[0], k, len(pairs), len(edges), crowded, early), file=sys.stderr)
        out[name + "_labels"] = lab.astype(np.int32)
        out[name + "_mask"] = mask
        out[name + "_centroids"] = cent
        out[name + "_edges"] = edges
        out[name + "_count"] = np.bincount(lab.ravel(), minlength=k + 1).astype(np.int64)
        out[name + "_sum_x"] = np.bincount(lab.ravel(), weights=np.tile(np.arange(lab.shape[1]), lab.shape[0]), minlength=k + 1).astype(np.int64)
        out[name + "_sum_y"] = np.bincount(lab.ravel(), weights=np.repeat(np.arange(lab.shape[0]), lab.shape[1]), minlength=k + 1).astype(np.int64)
        out[name + "_pairs"], out[name + "_pair_counts"], out[name + "_pair_first"] = pairs, counts, first
    out["names"] = np.array(names)
    path = os.path.join(HERE, "segments.npz")
    np.savez_compressed(path, **out)
    print("segments.npz: %d bytes, %d label images" % (os.path.getsize(path), len(names)))


if __name__ == "__main__":
    main()
