"""The finish stage alone, on response volumes chosen to exercise it, in all three of its forms.

ym_match_slice_begin scores into a caller-owned device volume; before ym_match_slice_finish (blockmax_kernel, then the
ordinary finish stage) the test overwrites that volume and the per-(x, y) maxima with its own.  Every case runs through
fine_kernel + final_kernel, finish_kernel<1024> and finish_kernel<256> (debug options 6 and 11), twice each:
  (a) the six results -- response, pose, covariance, fine sums -- must be the same bits (the project's own contract:
      a batch item is bit-identical to its single call whatever kernel finishes it), and
  (b) they must be what tests/finish_ref.py computes from the same volume and the device's own fine integer sums, at the
      tolerances of tests/test_gpu_parity.py (response 1e-12, pose 1e-9 absolute, covariance rtol 1e-9).
The planted values stand at least 0.1 above a seeded background in [0, 0.3]; the reference reports how far its closest
comparison was from its threshold and a case is compared only if that is at least 1e-9 (one explicit edge case, a
value exactly on the covariance's membership threshold, excepted)."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from tests import finish_ref as R  # noqa: E402

FORMS = ((0, 0), (2, 1024), (2, 256))  # (debug option 6, debug option 11): the per-angle pair, then the one-block kernel
BLOCK = 256                            # cells per score block (YM_SCORE_THREADS)
BEST = 0.75

# name -> configuration overrides; nx = search_size / (2 resolution) + 1, nt = 2 offset / angle resolution + 1
LATTICES = {
    "26x26x21": (dict(), (26, 26, 21)),                                                             # 63 blocks: the default
    "41x41x81": (dict(search_size=0.8, coarse_search_angle_offset=1.396), (41, 41, 81)),            # 567: the loop lattice after three expansions
    "41x41x161": (dict(search_size=0.8, coarse_search_angle_offset=2.792), (41, 41, 161)),          # 1127: above finish_kernel<256>'s 1024
    "47x47x21": (dict(search_size=0.92), (47, 47, 21)),                                             # 2209 cells: WIDE just over its threshold
    "91x91x256": (dict(search_size=1.8, coarse_search_angle_offset=2.55, coarse_angle_resolution=0.02), (91, 91, 256)),  # 8448 blocks
}

_rigs = {}
_backgrounds = {}


@pytest.fixture(scope="module", autouse=True)
def _release_rigs():
    yield
    for rig in _rigs.values():
        rig.m.set_stream(None)
    _rigs.clear()
    _backgrounds.clear()


class _Rig:
    """one matcher on a torch stream, with the device volume the sliced match scores into"""

    def __init__(self, lattice, expansion):
        import torch
        from oracle import oracle as orc
        from yag_slam_amd.scan_matching import ScanMatcher
        over, dims = LATTICES[lattice]
        over = dict(over) if expansion else dict(over, use_response_expansion=False)
        self.cfg = dict(orc.DEFAULT_CONFIG, **over)
        self.m = ScanMatcher(over or None)
        self.m.debug_option(12, 1)
        assert self.m.coarse_dims() == dims
        self.lc, self.lf = R.lattices(self.cfg)
        assert (self.lc["nx"], self.lc["ny"], self.lc["nt"]) == dims
        self.nx, self.ny, self.nt = dims
        torch.cuda.set_device(0)
        self.stream = torch.cuda.Stream()
        self.m.set_stream(self.stream.cuda_stream)
        with torch.cuda.stream(self.stream):
            self.resp = torch.empty(self.nx * self.ny * self.nt, dtype=torch.float64, device="cuda")
            self.probs = torch.empty(self.nx * self.ny, dtype=torch.float64, device="cuda")

    def run(self, vol, probs, query, base, refine, penalty):
        """the six results (three forms, twice each) as byte strings, and the fine sums of the first"""
        import torch
        with torch.cuda.stream(self.stream):
            vol_d = torch.from_numpy(np.ascontiguousarray(vol).ravel()).to("cuda")
            probs_d = torch.from_numpy(np.ascontiguousarray(probs).ravel()).to("cuda")
        out, fsums, first = [], None, None
        for form, threads in FORMS:
            for _ in range(2):
                self.m.debug_option(6, form)
                self.m.debug_option(11, threads)
                self.m.slice_begin(query, base, penalty, refine, 0, self.nt, self.resp.data_ptr(), self.probs.data_ptr())
                with torch.cuda.stream(self.stream):
                    self.resp.copy_(vol_d)
                    self.probs.copy_(probs_d)
                got = self.m.slice_finish()  # (raises on a status other than 0)
                bp = got.best_pose
                rec = np.array([got.response, bp.x, bp.y, bp.euler[-1]] + [v for row in got.covariance for v in row]).tobytes()
                if refine:
                    fs = self.m.debug_sums(1, dims=got.meta["fine_dims"])
                    assert tuple(got.meta["fine_dims"]) == (self.lf["nx"], self.lf["ny"], self.lf["nt"])
                    rec += fs.tobytes()
                    fsums = fs if fsums is None else fsums
                first = got if first is None else first
                out.append(rec)
        return out, first, fsums


def _rig(lattice, expansion=True):
    key = (lattice, expansion)
    if key not in _rigs:
        _rigs[key] = _Rig(lattice, expansion)
    return _rigs[key]


_scans = {}


def _inputs(heading=0.0):
    """the cfg2 query and base scans; the query's heading moved where a case asks for it (the grid only matters to the fine pass)"""
    from yag_slam_amd import synth
    if "base" not in _scans:
        _scans["q"], _scans["base"] = synth.single_match_scans()
    q = _scans["q"]
    if heading != 0.0 and heading not in _scans:
        _scans[heading] = synth.resident_scan(q.ranges, (3.0, 3.0, heading))
    return (q if heading == 0.0 else _scans[heading]), _scans["base"], (3.0, 3.0, heading)


def _background(lattice):
    """seeded values in [0, 0.3], [nt][ny][nx]; computed once per lattice and never written to (cases copy it)"""
    if lattice not in _backgrounds:
        nx, ny, nt = LATTICES[lattice][1]
        bg = np.random.default_rng(20240 + nx + nt).uniform(0.0, 0.3, size=(nt, ny, nx))
        bg.setflags(write=False)
        _backgrounds[lattice] = bg
    return _backgrounds[lattice].copy()


def _check(lattice, vol, heading=0.0, probs=None, refine=False, penalty=True, expansion=True, edge=False):
    """edge: an explicit edge case -- a value placed exactly on a threshold -- for which the margin rule cannot hold"""
    rig = _rig(lattice, expansion)
    query, base, pose = _inputs(heading)
    probs = vol.max(axis=0) if probs is None else probs
    recs, got, fsums = rig.run(vol, probs, query, base, refine, penalty)
    fine = None
    if refine:
        fine = dict(sums=fsums, nq=got.meta["n_query_points"], lat=rig.lf, penalize=penalty, pen=R.penalties(rig.cfg),
                    grid_off=R.grid_offset(rig.cfg, pose), scale=1.0 / rig.cfg["resolution"])
    ref = R.finish_ref(vol, rig.lc, pose, probs=probs, fine=fine)
    if edge:
        assert ref["margin"] == 0.0
    else:
        R.assert_margin(ref)
    # (a) one answer, bit for bit, from every form and every run
    names = ["%s run %d" % (("pair", "finish<1024>", "finish<256>")[i // 2], i % 2) for i in range(6)]
    differ = [n for n, r in zip(names, recs) if r != recs[0]]
    assert not differ, "results differ from the pair's first run in: %s (%d ties)" % (", ".join(differ), ref["n_ties"])
    # (b) and it is the reference's
    assert ref["status"] == 0
    bp = got.best_pose
    assert abs(got.response - ref["response"]) <= 1e-12
    np.testing.assert_allclose([bp.x, bp.y, bp.euler[-1]], ref["pose"], rtol=0, atol=1e-9)
    np.testing.assert_allclose(np.array(got.covariance), ref["cov"], rtol=1e-9, atol=1e-15)
    return ref, got


def _hyp_of_block(lattice, block, rng):
    """a seeded hypothesis (k, c) inside score block `block` = (angle k, block cb of 256 cells)"""
    nx, ny, nt = LATTICES[lattice][1]
    nxy = nx * ny
    ncb = (nxy + BLOCK - 1) // BLOCK
    k, cb = divmod(block, ncb)
    assert k < nt
    return k, cb * BLOCK + int(rng.integers(0, min(BLOCK, nxy - cb * BLOCK)))


def _n_blocks(lattice):
    nx, ny, nt = LATTICES[lattice][1]
    return (nx * ny + BLOCK - 1) // BLOCK * nt


def _plant(vol, kc, value):
    nt, ny, nx = vol.shape
    vol.reshape(nt, ny * nx)[kc[0], kc[1]] = value


# ------------------------------------------------------------------------------------------------ one maximum
def _single_places():
    out = []
    for lat in ("26x26x21", "41x41x81", "41x41x161"):
        out += [(lat, "h0"), (lat, "hlast"), (lat, "cell_last"), (lat, "cell256"), (lat, "k0"), (lat, "klast")]
    out += [("47x47x21", "hlast"), ("47x47x21", "cell_last"), ("47x47x21", "cell256")]
    out += [("91x91x256", "h0"), ("91x91x256", "hlast")]
    # score blocks around what each form keeps in registers (256, 512 and 1024 threads x 4, x 16 on a wide lattice), and the last
    out += [("91x91x256", b) for b in (1023, 1024, 2047, 2048, 4095, 4096, 8191, 8192, 8447)]
    return out


@pytest.mark.parametrize("lattice,where", _single_places())
def test_one_maximum(lattice, where):
    nx, ny, nt = LATTICES[lattice][1]
    nxy = nx * ny
    vol = _background(lattice)
    if isinstance(where, int):
        assert _n_blocks(lattice) == 8448
        kc = _hyp_of_block(lattice, where, np.random.default_rng(where))
    else:
        kc = {"h0": (0, 0), "hlast": (nt - 1, nxy - 1), "cell_last": (nt // 2, nxy - 1), "cell256": (1, 256), "k0": (0, 300),
              "klast": (nt - 1, 17)}[where]
    _plant(vol, kc, BEST)
    ref, got = _check(lattice, vol)
    assert ref["n_ties"] == 1 and got.response == BEST
    iy, ix = divmod(kc[1], nx)
    # a lone peak: the mean is its hypothesis, both variances clamp to 0.1 step^2 (times 1 / best)
    assert abs(got.best_pose.x - (3.0 - (nx - 1) * 0.01 + ix * 0.02)) < 1e-9
    assert got.covariance[0][0] == pytest.approx(0.1 * 0.02 * 0.02 / BEST, rel=1e-9)


# ------------------------------------------------------------------------------------------------ tie sets by block count
def _tie_counts():
    counts = (2, 255, 256, 257, 511, 512, 513, 1023, 1024, 1025)
    out = [("26x26x21", 2), ("26x26x21", 63)]
    out += [("41x41x81", n) for n in counts if n <= 567] + [("41x41x81", 567)]
    out += [("41x41x161", n) for n in counts]
    out += [("91x91x256", n) for n in (257, 513, 1025)]
    return out


@pytest.mark.parametrize("lattice,n_ties", _tie_counts())
def test_ties_one_per_block(lattice, n_ties):
    """the candidate-block list: one block, 2 to NT ranked blocks, more than NT (the full walk) -- NT is 512, 1024 and 256 in
    the three forms, so one tie set takes different paths in different forms"""
    rng = np.random.default_rng(1000 * n_ties + LATTICES[lattice][1][2])
    blocks = rng.choice(_n_blocks(lattice), size=n_ties, replace=False)
    vol = _background(lattice)
    places = [_hyp_of_block(lattice, int(b), rng) for b in blocks]
    for i in rng.permutation(n_ties):
        _plant(vol, places[i], BEST)
    ref, got = _check(lattice, vol)
    assert ref["n_ties"] == n_ties


@pytest.mark.parametrize("lattice", ["26x26x21", "41x41x161"])
def test_ties_several_in_one_block_and_others_elsewhere(lattice):
    rng = np.random.default_rng(77)
    vol = _background(lattice)
    nb = _n_blocks(lattice)
    inside = [_hyp_of_block(lattice, nb // 2, rng) for _ in range(9)]
    elsewhere = [_hyp_of_block(lattice, int(b), rng) for b in (0, 3, nb // 2 + 1, nb - 1)]
    for kc in inside + elsewhere:
        _plant(vol, kc, BEST)
    ref, got = _check(lattice, vol)
    assert ref["n_ties"] == len(set(inside)) + 4


@pytest.mark.parametrize("lattice", ["26x26x21", "41x41x161"])
def test_whole_angle_plane_tied(lattice):
    nx, ny, nt = LATTICES[lattice][1]
    vol = _background(lattice)
    vol[nt // 3] = BEST
    ref, got = _check(lattice, vol)
    assert ref["n_ties"] == nx * ny
    assert abs(got.best_pose.x - 3.0) < 1e-9 and abs(got.best_pose.y - 3.0) < 1e-9


@pytest.mark.parametrize("lattice", ["26x26x21", "41x41x81"])
def test_all_zero_volume(lattice):
    """a query that sees nothing: every hypothesis ties at zero (567 blocks on the loop lattice after three expansions: the
    pair's list overflows, finish_kernel<1024>'s does not)"""
    nx, ny, nt = LATTICES[lattice][1]
    ref, got = _check(lattice, np.zeros((nt, ny, nx)), expansion=False)
    assert ref["n_ties"] == nx * ny * nt and got.response == 0.0
    assert got.covariance[0][0] == 500.0 and got.covariance[1][1] == 500.0


@pytest.mark.parametrize("lattice", ["26x26x21", "41x41x161"])
def test_near_ties_at_the_edge_of_the_tolerance(lattice):
    """exact binary fractions: 0.5 - 2^-21 is DoubleEqual to 0.5 (1e-6), 0.5 - 2^-19 is not"""
    rng = np.random.default_rng(5)
    nb = _n_blocks(lattice)
    vol = _background(lattice)
    blocks = [int(b) for b in rng.choice(nb, size=8, replace=False)]
    best, member, outside = 0.5, 0.5 - 2.0 ** -21, 0.5 - 2.0 ** -19
    _plant(vol, _hyp_of_block(lattice, blocks[0], rng), best)
    _plant(vol, _hyp_of_block(lattice, blocks[1], rng), best)
    _plant(vol, _hyp_of_block(lattice, blocks[1], rng), outside)
    for b in blocks[2:5]:  # blocks whose maximum is a near tie and that hold no hypothesis equal to the best
        _plant(vol, _hyp_of_block(lattice, b, rng), member)
    _plant(vol, _hyp_of_block(lattice, blocks[4], rng), outside)
    for b in blocks[5:]:   # blocks whose maximum lies just outside
        _plant(vol, _hyp_of_block(lattice, b, rng), outside)
    ref, got = _check(lattice, vol)
    assert ref["n_ties"] == 5 and got.response == 0.5


@pytest.mark.parametrize("heading", [3.13, -3.13])
@pytest.mark.parametrize("ks", [(5, 15), (3, 12, 19), (0, 20, 20)])
def test_tied_headings_either_side_of_the_wrap(heading, ks):
    """the lattice's headings run from heading - 0.349 to heading + 0.349: across +-pi"""
    lattice = "26x26x21"
    rng = np.random.default_rng(31)
    vol = _background(lattice)
    cells = rng.choice(26 * 26, size=len(ks), replace=False)
    for k, c in zip(ks, cells):
        _plant(vol, (k, int(c)), BEST)
    ref, got = _check(lattice, vol, heading=heading)
    assert ref["n_ties"] == len(ks)
    lo, hi = heading - 0.349 + min(ks) * 0.0349, heading - 0.349 + max(ks) * 0.0349
    assert lo < np.pi < hi or lo < -np.pi < hi


# ------------------------------------------------------------------------------------------------ positional covariance
def _plateau(lattice, k, centre, radius, value, rim=None):
    """a disc of `value` around a peak of 0.5 in angle plane k; rim = (inside, outside): the last ring just above and the
    next just below the membership threshold"""
    nx, ny, nt = LATTICES[lattice][1]
    vol = _background(lattice)
    iy, ix = np.mgrid[0:ny, 0:nx]
    d = np.hypot(ix - centre[0], iy - centre[1])
    vol[k][d <= radius] = value
    if rim:
        vol[k][(d > radius - 1) & (d <= radius)] = rim[0]
        vol[k][(d > radius) & (d <= radius + 1)] = rim[1]
    vol[k, centre[1], centre[0]] = 0.5
    return vol


@pytest.mark.parametrize("inside", ["just_above", "exactly_at"])
def test_covariance_membership_at_its_edge(inside):
    """best - 0.1 +- 2^-20: the ring just above is a member, the ring just below is not.  And a ring exactly AT best - 0.1
    (the same IEEE subtraction on both sides, so the comparison is decided, not rounded: the one case compared with a
    margin of zero) is a member: the rule is >=."""
    edge = 0.5 - 0.1
    exact = inside == "exactly_at"
    vol = _plateau("26x26x21", 7, (15, 9), 5, 0.45, rim=(edge if exact else edge + 2.0 ** -20, edge - 2.0 ** -20))
    ref, got = _check("26x26x21", vol, edge=exact)
    probs = vol.max(axis=0)
    assert (probs >= edge).sum() == (np.hypot(*(np.mgrid[0:26, 0:26] - np.array([9, 15])[:, None, None])) <= 5).sum()
    assert got.covariance[0][0] > 2 * 0.1 * 0.02 * 0.02 / 0.5  # (well above the clamp)


def test_covariance_of_a_peak_in_a_corner():
    vol = _plateau("26x26x21", 20, (0, 0), 6, 0.45)
    vol[20, 3:6, 0] = 0.2  # (an asymmetric bite out of it)
    ref, got = _check("26x26x21", vol)
    assert abs(got.covariance[0][1]) > 1e-6 and got.covariance[0][1] == got.covariance[1][0]


def test_covariance_of_a_plateau_beyond_2048_cells():
    """47 x 47: the pair's covariance block walks with 32 loads in flight (WIDE), the one-block kernels with eight"""
    vol = _plateau("47x47x21", 4, (40, 3), 100, 0.45)
    ref, got = _check("47x47x21", vol)
    assert (vol.max(axis=0) >= 0.4).sum() == 2209


def test_covariance_from_maxima_that_are_not_the_volumes():
    """the search-space probabilities are an input of their own (a sliced match combines them across slices): members the
    volume does not show must count"""
    vol = _background("26x26x21")
    _plant(vol, (10, 13 * 26 + 13), BEST)
    probs = vol.max(axis=0)
    probs[2, 3] = probs[20, 24] = 0.7
    ref, got = _check("26x26x21", vol, probs=probs)
    assert got.covariance[0][0] > 10 * 0.1 * 0.02 * 0.02 / BEST


# ------------------------------------------------------------------------------------------------ the fine tail
def _fine_cases():
    near = 14 * 26 + 16  # the cell nearest the query's true offset (0.07, 0.04); angle 11 is nearest its true heading 0.05
    return {
        "peak_near_truth": [(11, near)],
        "peak_far": [(2, 3 * 26 + 22)],
        "peak_last": [(20, 26 * 26 - 1)],
        "two_ties": [(11, near), (11, near + 1)],
        "three_ties_off_lattice": [(11, near), (12, near + 1), (11, near + 26)],
        "three_ties_spread": [(10, near - 27), (11, near), (13, near + 2 * 26)],
    }


@pytest.mark.parametrize("penalty", [True, False])
@pytest.mark.parametrize("case", sorted(_fine_cases()))
def test_fine_tail_from_an_injected_coarse_mean(case, penalty):
    """refine: the injected coarse mean decides where the 3 x 3 fine lattice lands (three ties put it off the coarse
    lattice); the fine responses, best, tie mean and ComputeAngularCovariance are computed from the device's fine sums"""
    vol = _background("26x26x21")
    for kc in _fine_cases()[case]:
        _plant(vol, kc, BEST)
    ref, got = _check("26x26x21", vol, refine=True, penalty=penalty)
    assert ref["n_ties"] == len(_fine_cases()[case])
    if case != "peak_far" and case != "peak_last":
        assert got.response > 0.2  # (a real fine match: the lattice landed on the scene)


@pytest.mark.parametrize("heading", [3.13, -3.13])
def test_fine_tail_across_the_wrap(heading):
    vol = _background("26x26x21")
    for kc in [(9, 300), (12, 301), (12, 326)]:
        _plant(vol, kc, BEST)
    _check("26x26x21", vol, heading=heading, refine=True, penalty=True)


def _forced_regather_changes_nothing(vol, heading, penalty):
    """debug option 49: the angular covariance gathers the scan again at the mean pose's cell instead of reading that cell's
    column of the fine sums.  By the code's own argument the two are the same integers wherever that cell is one of the fine
    lattice's, so the three forms, each twice, forced and not, give the same bytes"""
    rig = _rig("26x26x21")
    query, base, _ = _inputs(heading)
    probs = vol.max(axis=0)
    plain = rig.run(vol, probs, query, base, True, penalty)[0]
    rig.m.debug_option(49, 1)
    try:
        forced = rig.run(vol, probs, query, base, True, penalty)[0]
    finally:
        rig.m.debug_option(49, 0)
    assert len(plain) == len(forced) == 6
    names = ["%s %s" % (f, w) for w in ("as is", "forced") for f in ("pair", "pair again", "finish<1024>", "finish<1024> again", "finish<256>", "finish<256> again")]
    differ = [n for n, r in zip(names, plain + forced) if r != plain[0]]
    assert not differ, "records differ from the pair's unforced one in: %s" % ", ".join(differ)


@pytest.mark.parametrize("penalty", [True, False])
@pytest.mark.parametrize("case", sorted(_fine_cases()))
def test_forced_regather_equals_the_fine_sums(case, penalty):
    vol = _background("26x26x21")
    for kc in _fine_cases()[case]:
        _plant(vol, kc, BEST)
    _check("26x26x21", vol, refine=True, penalty=penalty)  # (the unforced results are still the reference's)
    _forced_regather_changes_nothing(vol, 0.0, penalty)


@pytest.mark.parametrize("heading", [3.13, -3.13])
def test_forced_regather_equals_the_fine_sums_across_the_wrap(heading):
    vol = _background("26x26x21")
    for kc in [(9, 300), (12, 301), (12, 326)]:
        _plant(vol, kc, BEST)
    _check("26x26x21", vol, heading=heading, refine=True, penalty=True)
    _forced_regather_changes_nothing(vol, heading, True)


def test_status_of_a_volume_without_a_best_position_reaches_the_host():
    """every response NaN: no hypothesis is DoubleEqual to the best, the tie set is empty and the match has status -5,
    "unable to find best position", from every form (coarse only: there is no mean to refine around)"""
    import torch
    from yag_slam_amd import _capi
    rig = _rig("26x26x21")
    query, base, _ = _inputs()
    with torch.cuda.stream(rig.stream):
        vol_d = torch.full((21 * 26 * 26,), float("nan"), dtype=torch.float64, device="cuda")
    for form, threads in FORMS:
        rig.m.debug_option(6, form)
        rig.m.debug_option(11, threads)
        rig.m.slice_begin(query, base, True, False, 0, rig.nt, rig.resp.data_ptr(), rig.probs.data_ptr())
        with torch.cuda.stream(rig.stream):
            rig.resp.copy_(vol_d)
            rig.probs.copy_(vol_d[:26 * 26])
        with pytest.raises(_capi.YmError) as err:
            rig.m.slice_finish()
        assert err.value.code == -5, (form, threads)


def test_fine_tail_of_the_zero_volume():
    _check("26x26x21", np.zeros((21, 26, 26)), refine=True, penalty=True, expansion=False)
