"""The map segmenter's rules as tests/segmenter_ref.py restates them ("Map segmenter"), checked on the CPU: the
closing against a brute-force window, the invariants of the final labels, the share of free pixels that end up in no
segment, and the layouts of the C structs.  The device is compared with the same file in tests/test_gpu_segmenter.py."""
import ctypes as C
import os
import re

import numpy as np
import pytest
from scipy import ndimage

from tests import segmenter_ref as ref
from tests.util import REPO
from yag_slam_amd import _capi, splicing


@pytest.mark.parametrize("shape", [(7, 5), (23, 40), (67, 130)])
@pytest.mark.parametrize("close_size", [3, 11])
def test_closing_is_the_brute_force_window(shape, close_size):
    im = np.random.RandomState(shape[0]).choice(np.array([0, 100, 200, 254, 255], np.uint8), size=shape, p=[.1, .05, .05, .3, .5])
    closed, total, n_free = ref.free_space(im, close_size)
    want = ref.free_space_brute(im, close_size)
    assert closed.dtype == np.uint8 and np.array_equal(closed, want)
    assert set(np.unique(closed)) <= {0, 254, 255}
    assert total == int(want.astype(np.int64).sum()) and n_free == int((want != 0).sum())


FLOORPLANS = [((384, 512, 1), 83, 73), ((240, 320, 2), 33, 26), ((131, 197, 4), 11, 7)]


@pytest.fixture(scope="module")
def plans():
    return {args: ref.segment(ref.floorplan(*args)) for args, _, _ in FLOORPLANS}


@pytest.mark.parametrize("args,k,n", FLOORPLANS)
def test_final_labels_are_contiguous_connected_large_enough_and_in_raster_order(plans, args, k, n):
    labels, info = plans[args]
    assert labels.dtype == np.int32 and labels.shape == args[:2]
    assert info["segments"] == k and info["n_segments"] == n
    assert np.array_equal(np.unique(labels), np.arange(k + 1))  # 0 and exactly 1 .. K
    sizes = np.bincount(labels.reshape(-1))
    firsts = []
    for label in range(1, k + 1):
        assert ndimage.label(labels == label)[1] == 1, label  # one 4-connected component
        assert sizes[label] >= info["min_size"], label
        firsts.append(int(np.flatnonzero(labels.reshape(-1) == label)[0]))
    assert firsts == sorted(firsts)
    closed, _, n_free = ref.free_space(ref.floorplan(*args))
    assert not labels[closed == 0].any()  # only free pixels are labelled
    assert info["unlabelled"] == n_free - int(np.count_nonzero(labels))


@pytest.mark.parametrize("args,k,n", FLOORPLANS)
def test_few_free_pixels_end_up_in_no_segment(plans, args, k, n):
    _, info = plans[args]
    assert info["unlabelled"] / info["n_free"] <= 0.05, info


def test_a_pass_that_changes_nothing_ends_the_iterations():
    im = ref.walled_square(94)
    a, ia = ref.segment(im, n_segments=4, iterations=10, stage=ref.STAGE_ASSIGNED)
    b, ib = ref.segment(im, n_segments=4, iterations=ia["iterations_run"], stage=ref.STAGE_ASSIGNED)
    assert ia["iterations_run"] < 10 and np.array_equal(a, b)
    assert ia["step"] == 47 and list(np.bincount(a.reshape(-1))[1:]) == [2209] * 4


def test_struct_layouts_match_the_header():
    hdr = open(os.path.join(REPO, "include", "yagmatch.h")).read()
    assert re.search(r"typedef struct ym_segment_opts \{ int32_t n_segments[^;]*; double density; "
                     r"int32_t close_size, iterations, min_size_div, stage; \} ym_segment_opts;", hdr)
    assert re.search(r"typedef struct ym_segment_info \{ int64_t sum, n_free; int32_t n_segments, step, seeds, segments, "
                     r"iterations_run, min_size; int64_t unlabelled; \} ym_segment_info;", hdr)
    o, i = _capi.YmSegmentOpts, _capi.YmSegmentInfo
    assert [n for n, _ in o._fields_] == ["n_segments", "density", "close_size", "iterations", "min_size_div", "stage"]
    assert C.sizeof(o) == 32 and o.density.offset == 8 and o.close_size.offset == 16 and o.stage.offset == 28
    assert [n for n, _ in i._fields_] == ["sum", "n_free", "n_segments", "step", "seeds", "segments", "iterations_run", "min_size",
                                          "unlabelled"]
    assert C.sizeof(i) == 48 and i.n_segments.offset == 16 and i.min_size.offset == 36 and i.unlabelled.offset == 40
    assert _capi.SEGMENT_STAGES == {"final": ref.STAGE_FINAL, "assigned": ref.STAGE_ASSIGNED}
    assert "#define YM_SEGMENT_STAGE_FINAL 0" in hdr and "#define YM_SEGMENT_STAGE_ASSIGNED 1" in hdr
    assert callable(splicing.segment_map) and callable(splicing.free_space) and callable(splicing.SegmentMap.from_map)
