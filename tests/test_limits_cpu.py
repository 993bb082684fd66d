"""The frames of tests/limits_ref.py against the oracle and the numpy references: the demands that tests/test_gpu_limits.py sizes the device lists
by. They are pinned here, without a GPU, so that the GPU tests cannot drift with the frames.

Three figures differ from the ones the work was planned with, and the references decide:
* squares(12, 10, 24, 40, 20) keeps 120 borders and gives 120 quads in a plane, not 240: the hole border of a 24-pixel square has 76 points and
  fails the size filter (more than 83 points at 520 pixels). With three threshold planes the frame has 360 quads and still 120 candidates.
* checker(96, 128) has 5766 hole and 63 outer start candidates (checker(80, 112): 4158 and 55) once the one-pixel frame is cleared as the contour
  stage clears it (cand_ref.binary_of, as tests/test_gpu_start_candidates.py takes its reference); 5922 / 64 are the counts of the uncleared image.
* a one-pixel checkerboard has few outer starts whichever way round; dominoes() is the frame that fills the outer half of the start list.
"""
from collections import Counter

import numpy as np
import pytest

from tests import cand_ref, limits_ref as L, quad_ref

SQ10 = (12, 10, 24, 40, 20)
SQ8 = (12, 8, 24, 40, 20)
SQ_MANY = (16, 12, 28, 36, 20)


def kinds(borders):
    return Counter((c["hole"], len(c["pts"])) for c in borders)


@pytest.mark.parametrize("args, shape, n", [(SQ10, (440, 520), 120), (SQ8, (360, 520), 96)])
def test_squares_keep_one_border_and_give_one_candidate_a_square(args, shape, n):
    g = L.squares(*args)
    assert g.shape == shape
    kept = L.kept_borders(L.plane_of(g))
    assert kinds(kept) == {(0, 92): n}                      # the outer border; 92 points outlast the walkers' 64-step leash
    assert L.quad_demand(kept) == n
    assert len(L.oracle_candidates(g)) == n
    assert L.pool_bounds(kept) == (92 * n, 98 * n)
    sc = cand_ref.start_candidates(cand_ref.binary_of(L.plane_of(g)))
    assert (len(sc["outer"]), len(sc["hole"])) == (n, n)   # no false starts: at most n long walks of either kind


def test_larger_squares_keep_both_borders():
    """28-pixel squares at 520 pixels: outer (108 points) and hole border (88) both pass the filter on the 7-pixel planes - 240 borders and quads for
    120 candidates in one plane, hole and outer descriptors together"""
    g = L.squares(12, 10, 28, 40, 20)
    assert g.shape == (440, 520)
    kept = L.kept_borders(L.plane_of(g))
    assert kinds(kept) == {(0, 108): 120, (1, 88): 120}
    assert L.quad_demand(kept) == 240 and len(L.oracle_candidates(g)) == 120


def test_squares_on_three_planes():
    g = L.squares(*SQ10)
    assert quad_ref.plane_windows(7, 1) == [7, 7, 9]
    per_plane = [L.kept_borders(L.plane_of(g, p1=w)) for w in quad_ref.plane_windows(7, 1)]
    assert [len(k) for k in per_plane] == [120, 120, 120]
    assert sum(L.quad_demand(k) for k in per_plane) == 360
    assert len(L.oracle_candidates(g, thres_range=1)) == 120
    many = L.squares(*SQ_MANY)
    assert many.shape == (472, 616)
    assert sum(L.quad_demand(L.kept_borders(L.plane_of(many, p1=w))) for w in quad_ref.plane_windows(7, 1)) == 576   # above the hard 512 of a frame


@pytest.mark.parametrize("make, shape, outer, hole", [(L.checker, (96, 128), 63, 5766), (L.checker, (80, 112), 55, 4158),
                                                       (L.dominoes, (136, 256), 4191, 0)])
def test_start_list_frames(make, shape, outer, hole):
    th = L.plane_of(make(*shape), fixed=128)
    sc = cand_ref.start_candidates(cand_ref.binary_of(th))
    assert (len(sc["outer"]), len(sc["hole"])) == (outer, hole)
    assert max(outer, hole) > 4096                            # one half of the smallest start list (8192 entries) cannot hold them
    assert L.kept_borders(th) == []


def test_mixed_frame_has_two_late_borders():
    g = L.mixed()
    assert g.shape == (L.MIXED_H, L.MIXED_W)
    assert L.size_filter(L.MIXED_W, L.MIXED_H)[0] == 102
    kept = L.kept_borders(L.plane_of(g))
    assert kinds(kept) == {(0, 108): 70, (1, 1024): 1, (0, 1044): 1}   # every small square passes the filter
    assert sum(len(c["pts"]) > L.LATE_POINTS for c in kept) == 2
    assert len(L.oracle_candidates(g)) == 71 and L.quad_demand(kept) == 72
    assert L.pool_bounds(kept) == (9628, 10248)


@pytest.mark.parametrize("shape", [(440, 520), (360, 520), (480, 640), (96, 128), (136, 256), (472, 616)])
def test_marked_frames_hold_two_or_three_markers(shape):
    from oracle import orc

    for seed in (1, 2, 3):
        g = L.marked(seed, *shape)
        for params in ({}, {"thres_method": 0, "thres_p1": 128.0}, {"thres_range": 1}):
            o = orc.Oracle(**params)
            assert len(o.detect(g)) in (2, 3), (shape, seed, params)
    assert not np.array_equal(L.marked(1, *shape), L.marked(2, *shape))
