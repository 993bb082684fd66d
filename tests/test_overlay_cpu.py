"""Overlay pass, the checks that need no GPU: the library's exports, and the rules of tests/overlay_ref.py (the restatement the GPU tests
compare bytes against) checked on their own - the line rule, the projection against the oracle, the centroid rule."""
import ctypes as C
import os
import subprocess

import numpy as np

from tests import overlay_ref as ovr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_library_exports_the_draw_calls_and_the_style_is_12_bytes():
    from aruco_amd import build_library, capi

    lib = build_library()
    names = subprocess.run(["nm", "-D", "--defined-only", lib], stdout=subprocess.PIPE, text=True, check=True).stdout.split()
    assert "arucohip_draw_markers_batch" in names and "arucohip_draw_boards_batch" in names
    assert "arucohip_draw_markers_batch" in capi.SYMBOLS and "arucohip_draw_boards_batch" in capi.SYMBOLS
    assert C.sizeof(capi.Overlay) == 12
    # the header itself, with a C compiler
    src = ('#include "arucohip.h"\n_Static_assert(sizeof(arucohip_overlay_t) == 12, "style");\n'
           "_Static_assert(ARUCOHIP_DRAW_OUTLINE == 1 && ARUCOHIP_DRAW_IDS == 2 && ARUCOHIP_DRAW_AXIS == 4 && ARUCOHIP_DRAW_CUBE == 8 && "
           'ARUCOHIP_DRAW_Y_PERPENDICULAR == 16, "flags");\n')
    subprocess.run(["gcc", "-std=c11", "-fsyntax-only", "-I", os.path.join(ROOT, "include"), "-x", "c", "-"], input=src, text=True, check=True)


def test_font_has_every_character_the_overlays_print():
    assert set("0123456789id=xyzXYZ-") <= set(ovr.FONT)
    for ch, rows in ovr.FONT.items():
        assert len(rows) == 7 and all(0 <= r < 32 for r in rows), ch
    assert len({tuple(r) for r in ovr.FONT.values()}) == len(ovr.FONT)   # no two glyphs alike


def test_width_one_lines_in_all_eight_octants():
    """n + 1 pixels, one per major step, 8-connected, both endpoints included; |dx| = |dy| steps along x."""
    ends = [(17, 5), (5, 17), (-5, 17), (-17, 5), (-17, -5), (-5, -17), (5, -17), (17, -5),   # one per octant
            (9, 9), (-9, 9), (9, -9), (-9, -9), (12, 0), (0, 12), (-12, 0), (0, -12), (0, 0), (1000, 1), (3, 1000)]
    for dx, dy in ends:
        a, b = (40, 31), (40 + dx, 31 + dy)
        px = ovr.line_pixels(a, b)
        n = max(abs(dx), abs(dy))
        assert len(px) == n + 1 and px[0] == a and px[-1] == b, (dx, dy)
        assert len(set(px)) == n + 1
        major = 0 if abs(dx) >= abs(dy) else 1
        for p, q in zip(px, px[1:]):
            assert abs(q[major] - p[major]) == 1 and abs(q[1 - major] - p[1 - major]) <= 1, (dx, dy)
        # painting it covers exactly those pixels
        img = np.zeros((80, 80, 1), np.uint8)
        ovr.paint(img, [("line", a, b, (255, 0, 0), 1)])
        inside = {(x, y) for x, y in px if 0 <= x < 80 and 0 <= y < 80}
        assert {(int(x), int(y)) for y, x in zip(*np.nonzero(img[:, :, 0]))} == inside


def test_wide_lines_stamp_a_square_whose_top_left_is_half_the_width_back():
    for w in range(1, 8):
        img = np.zeros((20, 20, 1), np.uint8)
        ovr.paint(img, [("line", (10, 10), (10, 10), (9, 0, 0), w)])
        ys, xs = np.nonzero(img[:, :, 0])
        o = (w - 1) // 2
        assert (xs.min(), ys.min(), xs.max(), ys.max()) == (10 - o, 10 - o, 10 - o + w - 1, 10 - o + w - 1) and len(xs) == w * w


def _oracle_project(pts, rvec, tvec, K, k8):
    from oracle import orc

    so = orc.build()
    lib = orc.lib()
    sym = [s for s in subprocess.run(["nm", "-D", "--defined-only", so], stdout=subprocess.PIPE, text=True, check=True).stdout.split()
           if "project_points" in s]
    assert len(sym) == 1
    fn = getattr(lib, sym[0])
    fn.restype = None
    fn.argtypes = [C.c_void_p, C.c_int] + [C.c_void_p] * 7
    P = np.ascontiguousarray(pts, np.float64)
    out = np.zeros((len(P), 2))
    a = [np.ascontiguousarray(v, np.float64) for v in (rvec, tvec, K, k8)]
    fn(P.ctypes.data, len(P), a[0].ctypes.data, a[1].ctypes.data, a[2].ctypes.data, a[3].ctypes.data, out.ctypes.data, None, None)
    return out


def test_cube_and_axis_endpoints_equal_the_oracles_projection():
    """oracle/orc.h project_points (the restated cv::projectPoints) on the restatement's object points, five distortion coefficients."""
    K = np.array([[520.5, 0, 317.25], [0, 518.75, 243.5], [0, 0, 1]], np.float32)
    dist = np.array([0.11, -0.23, 0.0013, -0.0021, 0.057], np.float32)
    rvec, tvec = np.array([0.41, -0.73, 0.29]), np.array([0.031, -0.052, 0.61])
    k8 = np.zeros(8)
    k8[:5] = dist.astype(np.float64)
    sets = [ovr.marker_axis_points(0.05), ovr.marker_cube_points(0.05, False), ovr.marker_cube_points(0.05, True), ovr.board_axis_points(0.04),
            ovr.board_cube_points(0.04, False), ovr.board_cube_points(0.04, True)]
    for pts in sets:
        got = ovr.project(pts, rvec, tvec, K, dist)
        ref = _oracle_project(pts.astype(np.float64), rvec, tvec, K.astype(np.float64).reshape(9), k8)
        assert np.max(np.abs(got - ref)) < 1e-9
    # the reference's cube: its base is the marker's square, its top one marker size up (y when setYperpendicular)
    c, cy = ovr.marker_cube_points(0.05, False), ovr.marker_cube_points(0.05, True)
    assert np.allclose(c[:4, 2], 0) and np.allclose(c[4:, 2], 0.05) and np.allclose(np.abs(c[:, :2]), 0.025)
    assert np.allclose(cy[:4, 1], 0) and np.allclose(cy[4:, 1], 0.05) and np.allclose(cy[:, [0, 2]], c[:, :2])
    b = ovr.board_cube_points(0.04, False)
    assert np.allclose(b[[2, 3, 6, 7], 2], -0.04) and np.allclose(b[[0, 1, 4, 5], 2], 0) and np.allclose(b[4:, 1], 0.02)


def test_centroid_truncates_after_every_addition():
    """Point cent(0,0); cent.x += corner.x four times, then cent.x /= 4. By hand, x: 0 + 10.7 -> 10; 10 + 20.6 = 30.6 -> 30;
    30 + 20.9 = 50.9 -> 50; 50 + 10.9 = 60.9 -> 60; 60 / 4 = 15 (the mean of the floats is 15.775). y: 5.5 -> 5; 5 + 5.75 -> 10;
    10 + 30.9 -> 40; 40 + 30.99 -> 70; 70 / 4 = 17.5 -> 17."""
    assert ovr.centroid([10.7, 5.5, 20.6, 5.75, 20.9, 30.9, 10.9, 30.99]) == (15, 17)
    # negative coordinates truncate toward zero: -0.5 -> 0, 0 - 3.5 -> -3, -3 - 3.75 = -6.75 -> -6, -6 - 0.5 -> -6; -6 / 4 = -1.5 -> -1
    assert ovr.centroid([-0.5, 0, -3.5, 0, -3.75, 0, -0.5, 0])[0] == -1


def test_dropped_and_rounded_endpoints():
    assert ovr.to_pixel(2.5, 3.5) == (2, 4) and ovr.to_pixel(-0.5, -1.5) == (0, -2)      # ties to even
    assert ovr.to_pixel(float("nan"), 0) is None and ovr.to_pixel(float("inf"), 0) is None
    assert ovr.to_pixel(2.0 ** 20, 0) == (2 ** 20, 0) and ovr.to_pixel(2.0 ** 20 + 1, 0) is None
    assert ovr.to_pixel(1e300, 0) is None                                                  # narrows to infinity
