"""The component area filter on the device (yag_slam_amd/csrc/ym_k_despeckle.hpp; occupancy.despeckle,
create_clean_occupancy_grid, ros_map, LoopClosingMapper.make_ros_map) against the restatement tests/despeckle_ref.py: every
comparison is exact equality of the image and of the statistics.  The kernels' tiling is the segmenter's, 64 columns x 16
rows a block and 64 columns x 1 row a wave step, so the border cases sit on columns 63|64 and 127|128 and rows 15|16 and
31|32 of a 130 x 35 image, whose last tiles are partial.  tests/test_despeckle_host.py checks the restatement itself and
that the rendered fixtures hold specks to remove and walls to keep."""
import ctypes as C

import numpy as np
import pytest

from tests import despeckle_ref as D

pytestmark = pytest.mark.gpu


def _check(im, what="", **kw):
    """device == restatement: image and statistics; returns both"""
    from yag_slam_amd.occupancy import despeckle
    want, want_st = D.despeckle(np.ascontiguousarray(im), **kw)
    got, st = despeckle(im, stats=True, **kw)
    assert got.dtype == np.uint8 and got.shape == im.shape and got.flags.c_contiguous
    assert st == want_st, (what, kw, st, want_st)
    assert np.array_equal(got, want), (what, kw, int((got != want).sum()), np.argwhere(got != want)[:5].tolist())
    return got, st


def _blank(h, w, cells, value=255):
    im = np.full((h, w), value, np.uint8)
    for y, x in cells:
        assert 0 <= y < h and 0 <= x < w, (y, x)
        im[y, x] = 0
    return im


# ------------------------------------------------------------------------------------------------------ smallest shapes
def test_smallest_images():
    for v in (0, 255, 200):
        got, st = _check(np.full((1, 1), v, np.uint8), "1 x 1")
        # a lone occupied cell is a speck; a lone other cell is a background of 1 < 5 cells and becomes 255
        assert got[0, 0] == 255 and st["components"] == (v == 0) and st["background_filled"] == (v != 0)
    row = np.array([[0, 0, 255, 0, 200, 0, 0]], np.uint8)
    for conn in (4, 8):
        for area in (0, 1, 2, 3, 5):
            _check(row, "1 x 7", min_area=area, connectivity=conn)
            _check(np.ascontiguousarray(row.T), "7 x 1", min_area=area, connectivity=conn)
    five = _blank(5, 5, [(0, 0), (1, 1), (2, 2), (3, 3), (4, 4), (0, 4), (4, 0)])
    got8, st8 = _check(five, "5 x 5", connectivity=8)
    got4, st4 = _check(five, "5 x 5", connectivity=4)
    assert st8["components"] == 3 and st8["removed_components"] == 2 and (got8 == 0).sum() == 5
    assert st4["components"] == 7 and st4["removed_components"] == 7 and (got4 == 0).sum() == 0


# --------------------------------------------------------------------------------------------- the borders of the tiling
H, W = 35, 130


def _border_cases():
    """name -> (axis the border cuts, the first column or row beyond it, n -> the n cells)"""
    cases = {}
    for xb in (64, 128):  # (the image ends at column 129: the components at 127|128 start further left)
        def x0(n, xb=xb):
            return min(xb - 2, W - n)
        cases["row across columns %d|%d" % (xb - 1, xb)] = ("x", xb, lambda n, x0=x0: [(7, x0(n) + k) for k in range(n)])
        cases["diagonal down-right across columns %d|%d" % (xb - 1, xb)] = ("x", xb, lambda n, x0=x0: [(5 + k, x0(n) + k) for k in range(n)])
        cases["diagonal down-left across columns %d|%d" % (xb - 1, xb)] = ("x", xb, lambda n, x0=x0: [(5 + k, x0(n) + n - 1 - k) for k in range(n)])
    for yb in (16, 32):  # (the image ends at row 34)
        def y0(n, yb=yb):
            return min(yb - 2, H - n)
        cases["column across rows %d|%d" % (yb - 1, yb)] = ("y", yb, lambda n, y0=y0: [(y0(n) + k, 40) for k in range(n)])
        cases["diagonal down-right across rows %d|%d" % (yb - 1, yb)] = ("y", yb, lambda n, y0=y0: [(y0(n) + k, 30 + k) for k in range(n)])
        cases["diagonal down-left across rows %d|%d" % (yb - 1, yb)] = ("y", yb, lambda n, y0=y0: [(y0(n) + k, 40 - k) for k in range(n)])
    # where four tiles meet: (15, 63) | (15, 64) over (16, 63) | (16, 64)
    cases["corner, diagonal down-right"] = ("xy", None, lambda n: [(14 + k, 62 + k) for k in range(n)])
    cases["corner, diagonal down-left"] = ("xy", None, lambda n: [(14 + k, 65 - k) for k in range(n)])
    cases["corner, a square and a tail"] = ("xy", None, lambda n: [(15, 63), (15, 64), (16, 63), (16, 64), (17, 65)][:n])
    cases["corner, zigzag"] = ("xy", None, lambda n: [(15, 62), (16, 63), (15, 64), (16, 65), (15, 66)][:n])
    return cases


BORDER_CASES = _border_cases()


def _touch(a, b):
    return abs(a[0] - b[0]) <= 1 and abs(a[1] - b[1]) <= 1


@pytest.mark.parametrize("name", sorted(BORDER_CASES))
def test_components_of_4_and_5_cells_across_the_tile_borders(name):
    axis, border, make = BORDER_CASES[name]
    for n in (4, 5):
        cells = make(n)
        assert len(cells) == n and len(set(cells)) == n, (name, cells)
        xs, ys = [x for _, x in cells], [y for y, _ in cells]
        if axis == "x":
            assert min(xs) < border <= max(xs), (name, cells)  # the component does cross the border
        elif axis == "y":
            assert min(ys) < border <= max(ys), (name, cells)
        else:
            assert min(xs) < 64 <= max(xs) and min(ys) < 16 <= max(ys), (name, cells)
        edge_joined = all(abs(cells[k][0] - cells[k + 1][0]) + abs(cells[k][1] - cells[k + 1][1]) == 1 for k in range(n - 1))
        im = _blank(H, W, cells + [(1, x) for x in range(2, 8)])  # and a wall of 6 cells far away, which is always kept
        for conn in (8, 4):
            got, st = _check(im, name, connectivity=conn)
            if n == 5 and (conn == 8 or edge_joined):
                assert st["components"] == 2 and st["removed_components"] == 0 and np.array_equal(got, im), (name, n, conn, st)
            if n == 4:
                assert st["removed_components"] == st["components"] - 1 and (got == 0).sum() == 6, (name, n, conn, st)


def test_all_border_cases_in_one_image_under_every_area():
    """those of the 5-cell components that stay clear of one another, side by side, under areas on both sides of 4 and 5"""
    cells = []
    for name in sorted(BORDER_CASES):
        c = BORDER_CASES[name][2](5)
        if not any(_touch(p, q) for p in c for q in cells):
            cells += c
    im = _blank(H, W, cells)
    assert len(cells) >= 35
    for conn in (8, 4):
        for area in (1, 2, 4, 5, 6):
            _check(im, "all borders", min_area=area, connectivity=conn)


def test_checkerboard():
    yy, xx = np.mgrid[0:70, 0:70]
    im = np.where((yy + xx) % 2 == 0, 0, 255).astype(np.uint8)
    got, st = _check(im, "checkerboard", connectivity=8)
    assert st["components"] == 1 and st["removed_components"] == 0 and np.array_equal(got, im)
    got, st = _check(im, "checkerboard", connectivity=4)
    assert st["components"] == 2450 and st["removed_components"] == 2450 and (got == 255).all()


# ----------------------------------------------------------------------------------------------------------------- depth
def _spiral(n=200):
    """a one-cell-wide square spiral with one-cell gaps: a single 4-connected path from the corner to the middle"""
    im = np.full((n, n), 255, np.uint8)
    y, x, dy, dx = 0, 0, 0, 1
    im[0, 0] = 0
    while True:
        moved = 0
        while True:
            ny, nx = y + dy, x + dx
            ahead_y, ahead_x = ny + dy, nx + dx
            if not (0 <= ny < n and 0 <= nx < n) or im[ny, nx] == 0:
                break
            if 0 <= ahead_y < n and 0 <= ahead_x < n and im[ahead_y, ahead_x] == 0:
                break
            y, x = ny, nx
            im[y, x] = 0
            moved += 1
        if moved < 2:
            break
        dy, dx = dx, -dy
    return im


def _staircase(cells=199):
    pts, y, x = [], 0, 0
    for k in range(cells):
        pts.append((y, x))
        if k % 2 == 0:
            x += 1
        else:
            y += 1
    return _blank(y + 1, x + 1, pts)


def _comb(h=90, w=131):
    """teeth in every other column that join only in the last row: the lowest index of the one component is found last"""
    im = np.full((h, w), 255, np.uint8)
    im[:, ::2] = 0
    im[h - 1, :] = 0
    return im


@pytest.mark.parametrize("name", ["spiral", "staircase", "comb", "staircase mirrored", "comb upside down"])
def test_long_thin_components_are_one_component_with_an_exact_size(name):
    im = {"spiral": _spiral, "staircase": _staircase, "comb": _comb, "staircase mirrored": lambda: _staircase()[:, ::-1].copy(),
          "comb upside down": lambda: _comb()[::-1].copy()}[name]()
    cells = int((im == 0).sum())
    assert cells >= 199
    if name == "spiral":
        assert im.shape == (200, 200) and cells > 9000
    for conn in (4, 8):
        got, st = _check(im, name, min_area=cells, connectivity=conn)
        assert st["components"] == 1 and st["removed_components"] == 0 and np.array_equal(got, im), (name, conn, st)
        got, st = _check(im, name, min_area=cells + 1, connectivity=conn)
        assert st["removed_components"] == 1 and st["cleared_cells"] == cells and (got == 255).all(), (name, conn, st)


# ------------------------------------------------------------------------------------------------------- random images
@pytest.mark.parametrize("density", [0.05, 0.3, 0.41, 0.5, 0.7])
def test_random_images_on_both_sides_of_percolation(density):
    r = np.random.RandomState(int(density * 1000))
    im = np.where(r.rand(191, 257) < density, 0, r.choice([200, 255], size=(191, 257))).astype(np.uint8)
    assert im.shape == (191, 257)
    largest = {}
    for conn in (8, 4):
        for area in (1, 2, 5, 50, 10 ** 9):
            got, st = _check(im, "density %g" % density, min_area=area, connectivity=conn)
        largest[conn] = int((got == 0).sum()) == 0 and st["removed_components"] == st["components"]
    assert largest[8] and largest[4]  # at 10^9 everything goes
    if density == 0.05:
        assert D.despeckle(im, min_area=50)[1]["removed_components"] == D.despeckle(im, min_area=50)[1]["components"]
    if density == 0.7:
        assert D.despeckle(im, min_area=50)[1]["cleared_cells"] < 0.01 * (im == 0).sum()  # one giant component is kept


def test_rows_with_a_pitch_and_other_codes():
    from yag_slam_amd.occupancy import despeckle
    r = np.random.RandomState(5)
    big = np.where(r.rand(97, 300) < 0.3, 0, 255).astype(np.uint8)
    view = big[3:90, 11:208]
    assert view.strides[0] == 300 and not view.flags.c_contiguous
    before = big.copy()
    _check(view, "pitch > width")
    assert np.array_equal(big, before)  # the input is not written
    _check(big[::2, ::3], "a view whose columns are strided is copied first")
    many = r.randint(0, 12, size=(64, 150)).astype(np.uint8)
    got, st = _check(many, "foreground 7, fill 9", foreground=7, fill=9, min_area=3)
    assert st["removed_components"] > 50 and st["components"] > st["removed_components"]
    changed = got != many
    assert (many[changed] == 7).all() and (got[changed] == 9).all()
    # fill == foreground: the result is not examined again
    _check(many, "fill is the foreground", foreground=7, fill=7, min_area=3)
    assert despeckle(many, foreground=7, fill=9, min_area=3, stats=False).shape == many.shape


def test_background_rule_on_the_device():
    im = np.array([[0, 0, 0], [0, 255, 0], [0, 0, 200]], np.uint8)
    got, st = _check(im, "3 x 3, B = 2")
    assert st["background_filled"] == 1 and got[1, 1] == 255 and got[2, 2] == 255 and (got == 0).sum() == 7
    got, st = _check(im, "3 x 3, B = 2, area 2", min_area=2)
    assert st["background_filled"] == 0 and np.array_equal(got, im)
    got, st = _check(im, "3 x 3, B = 2, fill 9", fill=9)
    assert got[1, 1] == 9 and got[2, 2] == 9
    full = np.zeros((3, 3), np.uint8)
    got, st = _check(full, "3 x 3, B = 0")
    assert st["background_filled"] == 0 and st["background_cells"] == 0 and np.array_equal(got, full)
    # B = 4 spread over two waves and two blocks of a wider image
    wide = np.zeros((20, 70), np.uint8)
    wide[0, 0] = wide[0, 69] = wide[19, 63] = wide[19, 64] = 255
    got, st = _check(wide, "B = 4 in four tiles")
    assert st["background_filled"] == 1
    got, st = _check(wide, "B = 4 in four tiles, fill 3", fill=3)
    assert (got == 3).sum() == 4


def test_the_same_call_twice_gives_the_same_bytes():
    from yag_slam_amd.occupancy import despeckle
    r = np.random.RandomState(11)
    im = np.where(r.rand(191, 257) < 0.41, 0, 255).astype(np.uint8)
    a, sa = despeckle(im, stats=True)
    b, sb = despeckle(im, stats=True)
    assert a.tobytes() == b.tobytes() and sa == sb


def test_connectivity_6_raises():
    from yag_slam_amd import _capi
    from yag_slam_amd.occupancy import create_clean_occupancy_grid, despeckle
    im = np.zeros((4, 4), np.uint8)
    with pytest.raises(ValueError, match="connectivity 6"):
        despeckle(im, connectivity=6)
    with pytest.raises(ValueError, match="connectivity 6"):
        create_clean_occupancy_grid(D.loop_scans(2), 0.05, 12.0, connectivity=6)
    L = _capi.lib()
    u8 = C.POINTER(C.c_uint8)
    out = np.full((4, 4), 9, np.uint8)
    opts = _capi.YmDespeckleOpts(0, 255, 5, 6)
    assert L.ym_image_despeckle(0, im.ctypes.data_as(u8), 4, 4, 4, C.byref(opts), out.ctypes.data_as(u8), None) == -1
    assert "connectivity 6" in _capi.last_error() and (out == 9).all()


def test_no_device_memory_is_left_behind():
    from yag_slam_amd import _capi
    from yag_slam_amd.occupancy import create_clean_occupancy_grid, despeckle
    L = _capi.lib()

    def live():
        d, p = C.c_int64(), C.c_int64()
        _capi.check(L.ym_debug_live_bytes(C.byref(d), C.byref(p)))
        return d.value, p.value
    scans = D.loop_scans(4)
    for s in scans:
        s.native()
    im = np.where(np.random.RandomState(2).rand(100, 150) < 0.3, 0, 255).astype(np.uint8)
    despeckle(im)
    before = live()
    for k in range(5):
        despeckle(im, connectivity=4 + 4 * (k % 2), min_area=k)
        create_clean_occupancy_grid(scans, 0.05, 12.0)
    with pytest.raises(ValueError):
        despeckle(im, connectivity=6)
    assert live() == before


# ---------------------------------------------------------------------------------------------------- the render path
@pytest.fixture(scope="module")
def rendered():
    """per scan set: the scans, the plain grid, and the restatement's cleaning of it under 8 and under 4"""
    from yag_slam_amd.occupancy import create_occupancy_grid
    out = {}
    for name, (res, rt, dirty) in D.RENDER_SETS.items():
        scans = D.loop_scans(40, dirty)
        plain = create_occupancy_grid(scans, res, rt)
        out[name] = (scans, res, rt, plain, {conn: D.despeckle(plain.image, connectivity=conn) for conn in (8, 4)})
    return out


@pytest.mark.parametrize("name", sorted(D.RENDER_SETS))
def test_clean_grid_is_the_plain_grid_cleaned(rendered, name):
    from yag_slam_amd.occupancy import create_clean_occupancy_grid, create_occupancy_grid
    scans, res, rt, plain, want = rendered[name]
    for conn in (8, 4):
        g = create_clean_occupancy_grid(scans, res, rt, connectivity=conn)
        image, st = want[conn]
        assert (g.height, g.width) == (plain.height, plain.width) and g.offset == plain.offset and g.resolution == plain.resolution
        assert g.stats == st, (name, conn, g.stats, st)
        assert np.array_equal(g.image, image), (name, conn, int((g.image != image).sum()))
        assert st["removed_components"] >= 5 and st["components"] - st["removed_components"] >= 5  # (not vacuous)
    if name == "0.02_dirty":
        assert not np.array_equal(want[8][0], want[4][0])
    # other areas through the same path, and the plain entry as it was
    for area in (0, 2, 50):
        g = create_clean_occupancy_grid(scans, res, rt, min_area=area)
        image, st = D.despeckle(plain.image, min_area=area)
        assert np.array_equal(g.image, image) and g.stats == st
    again = create_occupancy_grid(scans, res, rt)
    assert np.array_equal(again.image, plain.image) and again.offset == plain.offset and not hasattr(again, "stats")


@pytest.mark.parametrize("name", sorted(D.RENDER_SETS))
def test_ros_map_is_the_nodes_arithmetic(rendered, name):
    from yag_slam_amd.occupancy import ros_map
    scans, res, rt, plain, want = rendered[name]
    m = ros_map(scans, res, rt)
    image, st = want[8]
    assert m.data.dtype == np.int8 and m.data.shape == (plain.height, plain.width)
    assert (m.height, m.width, m.resolution) == (plain.height, plain.width, res) and m.origin == plain.offset
    assert np.array_equal(m.data, D.ros_codes(image))
    assert m.data.ravel().tolist() == D.ros_codes(image).flatten().tolist()
    assert m.stats == st
    m4 = ros_map(scans, res, rt, connectivity=4, min_area=3)
    assert np.array_equal(m4.data, D.ros_codes(D.despeckle(plain.image, min_area=3, connectivity=4)[0]))


def test_stats_of_a_grid_made_without_the_filter_are_refused():
    from yag_slam_amd import _capi
    L = _capi.lib()
    scans = D.loop_scans(2)
    vp = C.c_void_p
    arr = (vp * 2)(*[s.native() for s in scans])
    st = _capi.YmDespeckleStats()
    st.components = 77
    for create in (L.ym_occupancy_create, L.ym_occupancy_create_counted):
        h = create(arr, 2, 0.05, 12.0)
        assert h
        try:
            assert L.ym_occupancy_get_despeckle_stats(h, C.byref(st)) == -1 and "without the filter" in _capi.last_error()
        finally:
            L.ym_occupancy_destroy(h)
    assert st.components == 77
    h = L.ym_occupancy_create_clean(arr, 2, 0.05, 12.0, None)  # null: the node's 0 / 255 / 5 / 8
    assert h
    try:
        assert L.ym_occupancy_get_despeckle_stats(h, C.byref(st)) == 0 and st.foreground_cells > 0
        info = _capi.YmOccupancyInfo()
        assert L.ym_occupancy_get_info(h, C.byref(info)) == 0
        img = np.empty((info.height, info.width), np.uint8)
        assert L.ym_occupancy_read(h, img.ctypes.data_as(C.POINTER(C.c_uint8)), img.size) == 0
    finally:
        L.ym_occupancy_destroy(h)
    from yag_slam_amd.occupancy import create_occupancy_grid
    want, want_st = D.despeckle(create_occupancy_grid(scans, 0.05, 12.0).image)
    assert np.array_equal(img, want) and st.components == want_st["components"] and st.cleared_cells == want_st["cleared_cells"]


def test_mapper_makes_the_map_the_node_publishes():
    """LoopClosingMapper.make_ros_map on the 30-scan trajectory of tests/test_gpu_occupancy.py's mapper test.  At the default
    0.05 m that trajectory's grid, at the poses the mapper arrives at, has 12 components of 25 .. 148 cells and no speck (measured;
    at the true poses it would have 30): there the map must simply be the node's arithmetic on the grid.  The same mapper's grid at
    0.02 m has specks (9 or 10 of 23 components at the true poses and at poses 1 cm off), so "fewer occupied cells" is asserted
    there, after the assertion that there is a speck to remove: no speck fails the test, it does not skip it."""
    from scipy import ndimage
    from yag_slam_amd import synth
    from yag_slam_amd.mapping import LoopClosingMapper
    from yag_slam_amd.scan_matching import ScanMatcher
    truth, scans = synth.trajectory_scans(30)
    mp = LoopClosingMapper(ScanMatcher(), None)
    for s in scans:
        mp.process_scan(s)
    g = mp.make_occupancy_grid(resolution=0.05, range_threshold=12)
    m = mp.make_ros_map()  # (resolution 0.05, range threshold 12)
    assert m.data.dtype == np.int8 and set(np.unique(m.data)) <= {-1, 0, 100}
    assert (m.height, m.width) == (g.height, g.width) and m.resolution == 0.05 and m.origin == g.offset
    assert np.array_equal(m.data, D.ros_codes(D.despeckle(g.image)[0]))
    assert (m.data == 100).sum() <= (g.image == 0).sum() and (m.data == 100).sum() > 200
    g = mp.make_occupancy_grid(resolution=0.02, range_threshold=12)
    labels, n = ndimage.label(g.image == 0, structure=np.ones((3, 3)))
    areas = np.bincount(labels.ravel())[1:]
    print("0.02 m: %d components, %d under 5 cells" % (n, int((areas < 5).sum())))
    assert n > 0 and (areas < 5).any(), "the uncleaned grid of this trajectory has no component under 5 cells: the test shows nothing"
    m = mp.make_ros_map(resolution=0.02, range_threshold=12)
    assert m.data.dtype == np.int8 and set(np.unique(m.data)) <= {-1, 0, 100}
    assert (m.height, m.width) == (g.height, g.width) and m.resolution == 0.02 and m.origin == g.offset
    assert (m.data == 100).sum() < (g.image == 0).sum()
    assert (m.data == 100).sum() == (g.image == 0).sum() - int(areas[areas < 5].sum())
    assert np.array_equal(m.data, D.ros_codes(D.despeckle(g.image)[0]))
