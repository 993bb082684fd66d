"""Plane rectification without a GPU: the numpy restatement (tests/rectify_ref.py) against properties it must have on its own, the host
window helper against hand-computed boxes, and the round trip with the CPU oracle's detections in place of the device's."""
import ctypes as C

import numpy as np

from tests import fiducial_ref as fr
from tests import rectify_ref as rr

IDENTITY = np.eye(3).reshape(9)


def test_identity_map_returns_the_source():
    rng = np.random.default_rng(1)
    for cn in (1, 3):
        src = rng.integers(0, 256, (64, 96) if cn == 1 else (64, 96, 3), dtype=np.uint8)
        assert np.array_equal(rr.warp_plane(src, IDENTITY, 96, 64), src)
        # a window past the right and bottom edges: zeros outside
        out = rr.warp_plane(src, IDENTITY, 100, 70)
        assert np.array_equal(out[:64, :96], src) and not out[64:].any() and not out[:, 96:].any()


def test_against_an_unquantised_bilinear_sample():
    """An independent float64 bilinear sample at the exact position. The ramp 2x + y has neighbour differences <= 4 (2, 1 and 3 on the
    diagonal), and on a ramp a bilinear sample is the ramp's value at the position. The rule moves the position by at most 1/64 px per
    axis (5 fractional bits, rounded to nearest), which moves the value by at most 4/64 per axis, and rounds the result once: 0.5. So
    every pixel whose four taps lie inside differs by less than 0.625 from the exact value, at most 1 level from its rounding."""
    H, W = 64, 96
    y, x = np.mgrid[0:H, 0:W]
    src = (2 * x + y).astype(np.uint8)
    K = np.array([[85.5, 0, 47.25], [0, 84.25, 31.5], [0, 0, 1]], np.float32)
    dist = np.array([0.08, -0.12, 0.0011, -0.0017, 0.03], np.float32)
    M = np.array([[1 / 90.0, 0.0007, -0.41], [-0.0004, 1 / 88.0, -0.27], [0.0006, -0.0009, 1.0]]).reshape(9)
    for Kd in ((None, None), (K, dist)):
        Mx = M if Kd[0] is not None else np.array([[0.93, 0.04, 5.3], [-0.03, 1.05, 2.2], [0.0008, -0.0011, 1.0]]).reshape(9)
        qx, qy, ok = rr.positions(Mx, 70, 50, *Kd)
        got = rr.sample(src, qx, qy, ok).astype(np.float64)
        px, py = qx / 32, qy / 32
        inside = ok & (px >= 0.5) & (px <= W - 1.5) & (py >= 0.5) & (py <= H - 1.5)
        assert inside.sum() > 2000
        x0, y0 = np.floor(px[inside]).astype(int), np.floor(py[inside]).astype(int)
        ax, ay = px[inside] - x0, py[inside] - y0
        s = src.astype(np.float64)
        exact = (s[y0, x0] * (1 - ax) * (1 - ay) + s[y0, x0 + 1] * ax * (1 - ay) + s[y0 + 1, x0] * (1 - ax) * ay + s[y0 + 1, x0 + 1] * ax * ay)
        assert np.max(np.abs(got[inside] - exact)) < 0.625
        assert np.max(np.abs(got[inside] - np.rint(exact))) <= 1


def test_half_even_tie_and_outside_taps():
    src = np.arange(1, 13, dtype=np.uint8).reshape(3, 4) * 20
    # px * 32 = 32 u + 0.5: a tie, rounded to the even 32 u, so the offset (1/64, 0) samples the source itself
    M = np.array([1, 0, 1 / 64, 0, 1, 0, 0, 0, 1.0])
    assert np.array_equal(rr.warp_plane(src, M, 4, 3), src)
    # py * 32 = 32 v + 1.5 rounds to the even 32 v + 2: ay = 2
    M = np.array([1, 0, 0, 0, 1, 3 / 64, 0, 0, 1.0])
    want = (src[:2].astype(int) * 30 * 32 * 32 + src[1:].astype(int) * 2 * 32 * 32 + (1 << 14)) >> 15
    assert np.array_equal(rr.warp_plane(src, M, 4, 3)[:2], want)
    # a shift by half a pixel to the left: the first column mixes the source's first column with a tap outside (0)
    M = np.array([1, 0, -0.5, 0, 1, 0, 0, 0, 1.0])
    out = rr.warp_plane(src, M, 4, 3)
    assert np.array_equal(out[:, 0], (src[:, 0].astype(int) * 16 * 32 * 32 + (1 << 14)) >> 15)
    # W <= 0, NaN and a saturated position are 0
    assert not rr.warp_plane(src, np.array([1, 0, 0, 0, 1, 0, 0, 0, -1.0]), 4, 3).any()
    assert not rr.warp_plane(src, np.array([1, 0, 0, 0, np.nan, 0, 0, 0, 1.0]), 4, 3).any()
    assert not rr.warp_plane(src, np.array([1e12, 0, 1e12, 0, 1e12, 1e12, 0, 0, 1.0]), 4, 3).any()


def _window_of_library(obj, info_type, marker_size, ppu, margin, flip_y):
    from aruco_amd import capi

    w = capi.rectify_board_window(obj, info_type, marker_size, ppu, margin, flip_y)
    return {"out_width": w.out_width, "out_height": w.out_height, "x0": w.x0, "y0": w.y0, "ux": w.ux, "uy": w.uy, "vx": w.vx, "vy": w.vy}


def test_window_helper_against_hand_computed_boxes():
    from aruco_amd import capi

    # PIX: two markers of side 100 spanning x -150..150, y -50..50 board pixels; marker_size 0.5 -> 0.005 per pixel: -0.75..0.75 x -0.25..0.25
    pix = np.array([[[-150, -50, 0], [-50, -50, 0], [-50, 50, 0], [-150, 50, 0]], [[50, -50, 0], [150, -50, 0], [150, 50, 0], [50, 50, 0]]], np.float32)
    want = {"out_width": 300, "out_height": 100, "x0": -0.75 + 0.0025, "y0": -0.25 + 0.0025, "ux": 0.005, "uy": 0.0, "vx": 0.0, "vy": 0.005}
    # ... with a margin of 0.125 (25 pixels each side) and y up
    want_m = {"out_width": 350, "out_height": 150, "x0": -0.875 + 0.0025, "y0": 0.375 - 0.0025, "ux": 0.005, "uy": 0.0, "vx": 0.0, "vy": -0.005}
    # METERS: one marker 0.25..0.75 x 1.0..1.5 at 64 px per metre: 32 x 32, the first centre 1/128 in
    met = np.array([[[0.25, 1.0, 0], [0.75, 1.0, 0], [0.75, 1.5, 0], [0.25, 1.5, 0]]], np.float32)
    want_met = {"out_width": 32, "out_height": 32, "x0": 0.25 + 1 / 128, "y0": 1.0 + 1 / 128, "ux": 1 / 64, "uy": 0.0, "vx": 0.0, "vy": 1 / 64}
    cases = [((pix, capi.BOARD_PIX, 0.5, 200.0, 0.0, False), want), ((pix, capi.BOARD_PIX, 0.5, 200.0, 0.125, True), want_m),
             ((met, capi.BOARD_METERS, 0.5, 64.0, 0.0, False), want_met)]
    for args, w in cases:
        for got in (_window_of_library(*args), rr.board_window(*args)):
            assert (got["out_width"], got["out_height"]) == (w["out_width"], w["out_height"])
            for k in ("x0", "y0", "ux", "uy", "vx", "vy"):
                assert float(got[k]) == float(np.float32(w[k])), (k, got[k], w[k])
    # a part of a pixel is a pixel; what cannot be a window is refused
    assert _window_of_library(met, capi.BOARD_METERS, -1.0, 64.5, 0.0, False)["out_width"] == 33
    win = capi.Rectify()
    L = capi.load()
    for bad in ((None, 1, 1, 1.0, 64.0, 0.0), (met.ctypes.data, 0, 1, 1.0, 64.0, 0.0), (met.ctypes.data, 1, 1, 1.0, 0.0, 0.0),
                (met.ctypes.data, 1, 1, 1.0, float("nan"), 0.0), (met.ctypes.data, 1, 1, 1.0, 64.0, -0.25), (met.ctypes.data, 1, 1, 1.0, 1e6, 0.0)):
        assert L.arucohip_rectify_board_window(*bad, 0, C.byref(win)) == capi.E_INVALID, bad
    assert L.arucohip_rectify_board_window(met.ctypes.data, 1, 1, 1.0, 64.0, 0.0, 0, None) == capi.E_INVALID


def test_round_trip_with_the_oracles_detections():
    """Paint the board, render it into three frames, detect and pose with the CPU oracle, rectify with the reference at one output pixel
    per board pixel: every cell centre of every marker reads what was painted. Cells are 10 px wide, so a pose good to 1e-4 relative
    cannot move a centre across an edge. The device chain of tests/test_gpu_rectify.py must meet the same condition."""
    from oracle import orc

    board, ids, obj = fr.board_image(fr.PANEL, rr.RT_GRID[0], rr.RT_GRID[1], rr.RT_SIDE, rr.RT_DIST, rr.RT_IDS)
    assert board.shape == (154, 238)
    frames = rr.round_trip_frames(obj)
    win = rr.board_window(obj, 0, rr.RT_MARKER_M, rr.RT_SIDE / rr.RT_MARKER_M, 0.0)
    assert (win["out_width"], win["out_height"]) == (238, 154)
    det = orc.Oracle()
    for f in range(len(frames)):
        markers = det.detect(frames[f], K=rr.RT_K, dist=None, marker_size=rr.RT_MARKER_M)
        assert sorted(m["id"] for m in markers) == sorted(rr.RT_IDS)
        b = orc.board_detect(markers, ids, obj, 0, rr.RT_K, None, rr.RT_MARKER_M)
        assert b["has_pose"] == 1
        M, valid = rr.plane_map(b["rvec"], b["tvec"], 1, win)
        out = rr.warp_plane(frames[f], M, 238, 154, rr.RT_K, None, valid)
        assert rr.round_trip_mismatches(board, out) == []
