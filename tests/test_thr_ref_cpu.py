"""tests/thr_ref.py, the reference of the threshold edge tests (tests/test_gpu_thr_edges.py), held to the oracle on the CPU, and the inputs of
those tests held to the coverage condition: an input that has no pixel within one grey level of the decision cannot see an off-by-one in a
kernel's constants, so every adaptive case must have at least 8 such pixels on each side. The reference alone decides that."""
import numpy as np
import pytest

from tests import thr_ref


@pytest.fixture(scope="module")
def orc():
    from oracle import orc
    orc.lib()
    return orc


def _sample(nframes, most=8):
    return sorted(set(int(round(i * (nframes - 1) / max(most - 1, 1))) for i in range(min(most, nframes))))


def test_adaptive_equals_the_oracle_on_every_input_of_the_edge_tests(orc):
    """Every adaptive case, at most 8 of its frames (the first and the last among them)."""
    seen = set()
    for name, family, nf, H, W, seed, block, c in thr_ref.adaptive_cases():
        for f in _sample(nf):
            key = (family, f, H, W, seed, block, c)
            if key in seen:
                continue
            seen.add(key)
            g = thr_ref.frame_of(family, f, H, W, seed)
            got, exp = thr_ref.adaptive(g, block, c), orc.adaptive_threshold(g, block, c)
            assert np.array_equal(got, exp), (name, f, thr_ref.first_diff(got, exp))
    assert len(seen) > 1000


def test_fixed_equals_the_oracles_fixed_image(orc):
    o = orc.Oracle(thres_method=0)
    for W in thr_ref.BLOCK_WIDTHS:
        for thr in thr_ref.FIXED_THRS:
            o.set_params(thres_p1=thr)
            for f in range(3):
                g = thr_ref.frame_of("levels", f, thr_ref.BLOCK_H, W, 700 + W)
                # the oracle's FIXED image comes with a detection; its marker stage has nothing to say here
                o.detect(g, cap=512)
                got, exp = thr_ref.fixed(g, thr), o.thresholded()
                assert np.array_equal(got, exp), (W, thr, f, thr_ref.first_diff(got, exp))


def test_tiles_and_bitmap_of_a_hand_written_example():
    """17 x 9 pixels: 3 x 2 real tiles in a 4 x 4 tile array (tiles_x = max(4, 3 + 1), tiles_y = max(4, 2 + 1))."""
    t = np.zeros((9, 17), np.uint8)
    t[:, :] = 0
    t[0, :] = 255            # first row: cleared
    t[8, :] = 255            # last row: cleared (it is the only row of the second tile row)
    t[:, 0] = 255            # first column: cleared
    t[:, 16] = 255           # last column: cleared (the only column of the third tile column)
    t[1, 1] = 255            # tile (0, 0) bit 1 * 8 + 1
    t[7, 7] = 255            # tile (0, 0) bit 63
    t[3, 8] = 255            # tile (0, 1) bit 3 * 8 + 0
    t[7, 15] = 255           # tile (0, 1) bit 7 * 8 + 7
    tiles = thr_ref.tiles_of(t)
    exp = np.zeros((4, 4), np.uint64)
    exp[0, 0] = (1 << 9) | (1 << 63)
    exp[0, 1] = (1 << 24) | (1 << 63)
    assert tiles.dtype == np.uint64 and tiles.shape == (4, 4)
    assert np.array_equal(tiles, exp)
    bm = thr_ref.bitmap_of(tiles, 17)
    assert bm.shape == (4, 2) and bm.dtype == np.uint64
    assert np.array_equal(bm, np.array([[1, 1], [0, 0], [0, 0], [0, 0]], np.uint64))   # even word: tile 0, odd word: tile 1
    # a set pixel in the last real row and column that is not on the frame: 18 x 10
    t2 = np.zeros((10, 18), np.uint8)
    t2[8, 16] = 255
    tiles2 = thr_ref.tiles_of(t2)
    exp2 = np.zeros((4, 4), np.uint64)
    exp2[1, 2] = 1
    assert np.array_equal(tiles2, exp2)
    assert np.array_equal(thr_ref.bitmap_of(tiles2, 18), np.array([[0, 0], [2, 0], [0, 0], [0, 0]], np.uint64))   # tile 2 = even word, bit 1
    # two strips: tile 128 is bit 0 of the second strip's even word, tile 127 bit 63 of the first strip's odd word
    wide = np.zeros((4, 131), np.uint64)
    wide[0, 127] = 5
    wide[0, 128] = 1
    wide[0, 130] = 7                # the pad tile of a 1040-pixel row: beyond ceil(W / 8) = 130, no bit
    bm = thr_ref.bitmap_of(wide, 1040)
    assert np.array_equal(bm[0], np.array([0, 1 << 63, 1, 0], np.uint64)) and not bm[1:].any()


def test_stack_and_single_frame_forms_agree():
    g = thr_ref.batch("lines", 4, 19, 33, 5)
    a = thr_ref.adaptive(g, 5, -3.5)
    for f in range(4):
        assert np.array_equal(a[f], thr_ref.adaptive(g[f], 5, -3.5))
        assert np.array_equal(thr_ref.tiles_of(a)[f], thr_ref.tiles_of(a[f]))
    # the definition's other form: g - (S + n // 2) // n <= -floor(C)
    S = thr_ref.block_sums(g, 5)
    assert np.array_equal(a != 0, g.astype(np.int64) - (S + 12) // 25 <= 4)
    # no two frames of a batch are alike
    assert len({g[f].tobytes() for f in range(4)}) == 4


# Cases whose input cannot satisfy the coverage condition, with the reason: none. (|floor(C)| >= 256 is outside the condition: no pixel of an
# 8-bit image is that far from its neighbourhood's mean, so every pixel falls on one side whatever the input.)
NO_NEAR_TIES = {}


def test_every_adaptive_case_has_pixels_within_one_grey_level_of_the_decision():
    """The coverage condition: summed over all of a case's frames at least 8 pixels with 0 <= d < n and 8 with -n <= d < 0. Prints, per group
    of cases, the lowest, median and highest of the sums (the table of DESIGN.md, "Edge cases of the threshold stage")."""
    groups = {}
    for name, family, nf, H, W, seed, block, c in thr_ref.adaptive_cases():
        if abs(int(np.floor(c))) >= 256 or name in NO_NEAR_TIES:
            continue
        above = below = 0
        for f in range(nf):
            a, b = thr_ref.near_ties(thr_ref.frame_of(family, f, H, W, seed), block, c)
            above, below = above + a, below + b
        assert above >= 8 and below >= 8, (name, above, below)
        groups.setdefault(name.split("-")[0].rstrip("0123456789"), []).append((min(above, below), above, below, name))
    for g, v in groups.items():
        v.sort()
        print("near ties %-10s %3d cases: lowest %s, median %s, highest %s" % (g, len(v), v[0], v[len(v) // 2][:3], v[-1][:3]))
