"""Virtual scans from an occupancy map, host side (yag_slam_amd/splicing.py): the test's own vectorised numpy restatement of
the reference's pixel walk (/root/reference/yag_slam/raytracing.py:63-88) against the fixture the reference's code recorded
(tests/golden/make_golden_raytrace.py), the frame conversions and sensor of map_to_graph (splicing.py:82-107), and what
its scans describe.  CPU only: the walk here is the yardstick of tests/test_gpu_raytrace.py."""
import hashlib
import math
import os
import subprocess
import sys

import numpy as np
import pytest

from tests.util import GOLDEN


def walk(img, starts, dir_cs, max_steps=None):
    """trace_ray for every (start, direction) pair at once: float32 point, float64 arithmetic, np.round (half to even) on
    the float32 value.  img uint8 [h][w] (any row stride), starts [n][2] (x = column, y = row), dir_cs [a][2] (cos, sin).
    Returns (ends [n, a, 2] float32, lengths [n, a] float64 = |end - start| of the float32 points, steps [n, a])."""
    img = np.asarray(img)
    h, w = img.shape
    st = np.asarray(starts, dtype=np.float64).reshape(-1, 2)
    dc = np.asarray(dir_cs, dtype=np.float64).reshape(-1, 2)
    shape = (st.shape[0], dc.shape[0])
    x0 = np.broadcast_to(st[:, 0].astype(np.float32)[:, None], shape).ravel()
    y0 = np.broadcast_to(st[:, 1].astype(np.float32)[:, None], shape).ravel()
    c = np.broadcast_to(dc[None, :, 0], shape).ravel()
    s = np.broadcast_to(dc[None, :, 1], shape).ravel()
    x, y = x0.copy(), y0.copy()
    steps = np.zeros(x.shape, dtype=np.int64)
    act = np.arange(x.size)
    cap = max_steps or 2 * (w + h) + 4
    while act.size:
        ax, ay = x[act], y[act]
        val = img[np.rint(ay).astype(np.int64), np.rint(ax).astype(np.int64)]
        nx = (ax.astype(np.float64) + c[act]).astype(np.float32)
        ny = (ay.astype(np.float64) + s[act]).astype(np.float32)
        hit = val < 210
        jump = hit & (val > 180)
        nx[jump] = (nx[jump].astype(np.float64) + 1000 * c[act][jump]).astype(np.float32)
        ny[jump] = (ny[jump].astype(np.float64) + 1000 * s[act][jump]).astype(np.float32)
        rx, ry = np.rint(nx), np.rint(ny)
        out = (ry < 1) | (rx < 1) | (rx >= w - 1) | (ry >= h - 1)
        x[act], y[act] = nx, ny
        steps[act] += 1
        act = act[~(hit | out) & (steps[act] < cap)]
    dx, dy = (x - x0).astype(np.float64), (y - y0).astype(np.float64)
    ends = np.stack([x, y], axis=1).reshape(shape + (2,))
    return ends, np.sqrt(dx * dx + dy * dy).reshape(shape), steps.reshape(shape)


def reference_ranges(lengths, resolution):
    """map_to_graph's readings: length x resolution, > 20 -> 100 (splicing.py:92-95)"""
    r = lengths * resolution
    return np.where(r > 20, 100.0, r)


@pytest.fixture(scope="module")
def fx():
    return np.load(os.path.join(GOLDEN, "raytrace.npz"), allow_pickle=False)


def test_walk_reproduces_the_reference_sweeps_bit_for_bit(fx):
    from yag_slam_amd.splicing import direction_table
    im = fx["image"]
    ends, lengths, _ = walk(im, fx["sweep_viewpoints"], direction_table(fx["sweep_angles"]))
    assert np.array_equal(ends, fx["sweep_ends"])
    np.testing.assert_allclose(lengths, fx["sweep_lengths"], rtol=1e-6, atol=0)
    ends, lengths, _ = walk(im, fx["full_viewpoint"][None], direction_table(fx["full_angles"]))
    assert np.array_equal(ends[0], fx["full_ends"])
    np.testing.assert_allclose(lengths[0], fx["full_lengths"], rtol=1e-6, atol=0)


def test_walk_reproduces_map_to_graph_ranges(fx):
    from yag_slam_amd.splicing import REFERENCE_ANGLES, direction_table
    _, lengths, steps = walk(fx["image"], fx["centroids"], direction_table(REFERENCE_ANGLES[::-1]))
    want = fx["graph_ranges"]
    got = reference_ranges(lengths, float(fx["resolution"]))
    assert np.array_equal(got == 100, want == 100)
    np.testing.assert_allclose(got, want, rtol=1e-6, atol=0)
    # the edge cases the fixture's centroids stand for
    assert (steps[2] == 1).all() and np.allclose(got[2], float(fx["resolution"]), rtol=1e-5)  # on an occupied pixel: one step
    assert (got[3] == 100).all()                                            # on an unknown pixel: the jump
    assert (steps[5] == 1).all()                                            # on a 180 pixel: one step, no jump
    assert (steps[8] == 1).sum() > 700                                      # the open top row: one step upwards
    # the `> 20 -> 100` rule meets real lengths (not only the 1000-pixel jump), and readings just below 20 m stay
    real = lengths < 1000
    assert ((lengths * float(fx["resolution"]) > 20) & real).sum() > 100
    assert ((want > 19.5) & (want <= 20)).sum() > 10


def test_direction_table_is_the_references(fx):
    from yag_slam_amd.splicing import REFERENCE_ANGLES, direction_table
    assert np.array_equal(direction_table(fx["sweep_angles"]), fx["sweep_cs"])
    assert np.array_equal(REFERENCE_ANGLES, fx["full_angles"]) and REFERENCE_ANGLES.shape == (1439,)
    assert REFERENCE_ANGLES[0] == -180 and REFERENCE_ANGLES[-1] == 179.5
    # the table trace_ray evaluates angle by angle (np.deg2rad, np.cos / np.sin of a float64 scalar)
    tab = direction_table(REFERENCE_ANGLES[::-1])
    for i in range(0, 1439, 7):
        a = np.deg2rad(REFERENCE_ANGLES[::-1][i])
        assert tab[i, 0] == np.cos(a) and tab[i, 1] == np.sin(a)


def test_pixel_to_meters_and_sensor_are_the_references(fx):
    from yag_slam_amd.splicing import REFERENCE_SENSOR, pixel_to_meters
    res, origin, h = float(fx["resolution"]), tuple(fx["origin"]), fx["image"].shape[0]
    for (cx, cy), p in zip(fx["centroids"], fx["graph_poses"]):
        assert pixel_to_meters(res, origin, h, cx, cy) == (p[0], p[1]) and p[2] == 0
    assert np.array_equal(np.array(REFERENCE_SENSOR, dtype=np.float64), fx["graph_sensor"])
    assert np.array_equal(fx["graph_nums"], np.arange(len(fx["centroids"])))
    assert fx["graph_ranges"].shape == (len(fx["centroids"]), 1439)


def test_reference_scans_describe_the_mirrored_map(fx):
    """map_to_graph's frame (the splicing module text): reading i, cast at 179.5 - 0.25 i degrees and filed under the
    sensor's -180 + 0.25 i, is the reading of the map mirrored about a horizontal line along -180 + 0.25 i + 0.5 degrees,
    from the mirrored centroid.  The float32 walk is not exactly mirror-symmetric, so readings agree to a pixel."""
    from yag_slam_amd.splicing import REFERENCE_ANGLES, direction_table
    im, res = fx["image"], float(fx["resolution"])
    h = im.shape[0]
    cent = fx["centroids"][[0, 4]]  # the two centroids inside free space
    want = fx["graph_ranges"][[0, 4]]
    mirrored = cent.copy()
    mirrored[:, 1] = (h - 1) - cent[:, 1]
    _, lengths, _ = walk(im[::-1], mirrored, direction_table(REFERENCE_ANGLES + 0.5))
    got = reference_ranges(lengths, res)
    near = np.abs(got - want) <= 1.5 * res
    assert near.mean() > 0.97, near.mean()
    # ... while the sensor's own angles in the unmirrored map do not describe them
    _, lengths, _ = walk(im, cent, direction_table(REFERENCE_ANGLES))
    assert (np.abs(reference_ranges(lengths, res) - want) <= 1.5 * res).mean() < 0.5


def cell_centre_grid():
    """a 40 x 30 grid at 0.05 m, cell (0, 0) at world (-1.3, 0.7), one-cell walls at column 25, column 3 and row 22, and a
    viewpoint at the world centre of cell (11, 15): in this package's frame (cell (c, r) centred at (ox + c res, oy + r res))
    the +x, -x and +y rays read exactly (25 + 1 - 11), (11 - 3 + 1) and (22 + 1 - 15) cells -- the wall's cell and the
    reference's one step past it.  Under a corner convention (centre at ox + (c + 0.5) res) the start lies on a tie, rounds
    to cell 12 and the rays step past the one-cell walls."""
    res, origin = 0.05, (-1.3, 0.7)
    im = np.full((30, 40), 254, dtype=np.uint8)
    im[:, 25] = 0
    im[:, 3] = 0
    im[22, :] = 0
    view = (origin[0] + 11 * res, origin[1] + 15 * res)
    want = np.array([25 + 1 - 11, 22 + 1 - 15, 11 - 3 + 1]) * res  # beams at 0, 90 and 180 degrees
    return im, res, origin, view, want


def test_world_layout_cell_centres_exact():
    from yag_slam_amd.splicing import world_to_pixels
    im, res, origin, view, want = cell_centre_grid()
    cs = [[math.cos(a), math.sin(a)] for a in (0.0, math.pi / 2, math.pi)]
    px = np.array(world_to_pixels(res, origin, view[0], view[1]))
    _, lengths, _ = walk(im, px[None], cs)
    assert np.array_equal(lengths[0] * res, want)
    _, lengths, _ = walk(im, px[None] + 0.5, cs)  # the corner convention: a different reading
    assert not np.allclose(lengths[0] * res, want, rtol=0, atol=0.5 * res)


def test_raymap_rejects_what_the_walk_cannot_take():
    """argument checks that run before any device work (no GPU needed to reach them)"""
    from yag_slam_amd import splicing
    with pytest.raises(ValueError):
        splicing.RayMap(np.zeros((4, 4), dtype=np.float32))
    with pytest.raises(ValueError):
        splicing.virtual_scans(np.zeros((4, 4), dtype=np.uint8), 0.05, (0, 0), [], layout="pixels")


@pytest.mark.skipif(not (os.path.isdir("/root/reference") and os.environ.get("YM_REGENERATE_GOLDENS") == "1"),
                    reason="opt-in (YM_REGENERATE_GOLDENS=1) and only where the reference is: the build container")
def test_raytrace_golden_regenerates_bit_identically():
    path = os.path.join(GOLDEN, "raytrace.npz")
    before = hashlib.sha256(open(path, "rb").read()).hexdigest()
    subprocess.check_call([sys.executable, os.path.join(GOLDEN, "make_golden_raytrace.py")], stdout=subprocess.DEVNULL,
                          stderr=subprocess.DEVNULL)
    assert hashlib.sha256(open(path, "rb").read()).hexdigest() == before
