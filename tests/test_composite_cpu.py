"""Plane compositing without a GPU: what the library declares and exports, the numpy restatement (tests/composite_ref.py) against
properties it must have on its own, and the board replaced in three frames with the CPU oracle's detections in place of the device's."""
import ctypes as C
import os
import re
import subprocess
from unittest import mock

import numpy as np
import pytest

from tests import composite_ref as cr
from tests import fiducial_ref as fr
from tests import rectify_ref as rr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("arucohip_composite_plane_batch", "arucohip_board_composite_batch")
IDENTITY = np.eye(3).reshape(9)


def shifted(ds=0.0, dt=0.0):
    return np.array([1, 0, ds, 0, 1, dt, 0, 0, 1.0])


def test_new_symbols_are_declared_bound_and_exported(tmp_path):
    from aruco_amd import build_library, capi

    header = open(os.path.join(ROOT, "include", "arucohip.h")).read()
    names = set(subprocess.run(["nm", "-D", "--defined-only", build_library()], stdout=subprocess.PIPE, text=True, check=True).stdout.split())
    for s in NEW:
        assert re.search(r"\bint %s\(" % s, header), s
        assert s in capi.SYMBOLS and s in names, s
    src = tmp_path / "texture_size.c"
    src.write_text('#include "arucohip.h"\n_Static_assert(sizeof(arucohip_texture_t) == %d, "arucohip_texture_t");\n' % C.sizeof(capi.Texture))
    r = subprocess.run(["gcc", "-std=c11", "-fsyntax-only", "-I" + os.path.join(ROOT, "include"), str(src)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    assert C.sizeof(capi.Texture) == 48 and capi.Texture.opacity.offset == 40 and capi.Texture.row_stride.offset == 24


def test_shim_caller_compiles_against_the_mock():
    cpp = os.path.join(ROOT, "tests", "cpp")
    r = subprocess.run(["g++", "-std=c++17", "-Wall", "-DARUCOHIP_USE_OPENCV", "-I" + os.path.join(cpp, "mock_opencv"), "-I" + os.path.join(ROOT, "include"),
                        "-fsyntax-only", os.path.join(cpp, "shim_composite.cpp")], capture_output=True, text=True)
    assert r.returncode == 0 and "warning" not in r.stderr, r.stderr[-3000:]


def test_identity_map_copies_the_texture_to_the_origin():
    rng = np.random.default_rng(2)
    for cn in (1, 3):
        frame = rng.integers(0, 256, (64, 96) if cn == 1 else (64, 96, 3), dtype=np.uint8)
        tex = rng.integers(0, 256, (30, 40) if cn == 1 else (30, 40, 3), dtype=np.uint8)
        out, painted = cr.composite(frame, tex, IDENTITY)
        assert painted.sum() == 40 * 30 and painted[:30, :40].all()
        assert np.array_equal(out[:30, :40], tex)
        keep = np.ones((64, 96), bool)
        keep[:30, :40] = False
        assert np.array_equal(out[keep], frame[keep])
        # an invalid frame, an all-zero mask and opacity 0 leave every byte
        for kw in (dict(valid=False), dict(mask=np.zeros((64, 96), np.uint8)), dict(opacity=0)):
            same, none = cr.composite(frame, tex, IDENTITY, **kw)
            assert np.array_equal(same, frame) and not none.any()


def test_blend_values_by_hand():
    """w = (A opacity + 127) / 255, out = (C w + F (255 - w) + 127) / 255 with C = 200 on F = 50, worked out on paper:
    A 255, opacity 255: w 255 -> 200;  A 255, opacity 128: w = 32767 / 255 = 128 -> 32077 / 255 = 125;  A 100, opacity 255: w = 25627 / 255 = 100
    -> 27877 / 255 = 109;  A 100, opacity 128: w = 12927 / 255 = 50 -> 20377 / 255 = 79;  A 0 or opacity 0: w 0, untouched;  A 1 at opacity
    128: w = 255 / 255 = 1 -> (200 + 50 * 254 + 127) / 255 = 13027 / 255 = 51."""
    frame = np.full((3, 4), 50, np.uint8)
    want = {(255, 255): 200, (255, 128): 125, (100, 255): 109, (100, 128): 79, (0, 255): 50, (0, 128): 50, (255, 0): 50, (100, 0): 50, (1, 128): 51,
            (1, 127): 50}           # A 1 at 127: w = 254 / 255 = 0
    for (A, opacity), value in want.items():
        tex = np.zeros((3, 4, 2), np.uint8)
        tex[:, :, 0], tex[:, :, 1] = 200, A
        out, painted = cr.composite(frame, tex, IDENTITY, opacity=opacity)
        assert (out == value).all(), (A, opacity, out[0, 0])
        assert painted.all() == (value != 50) and painted.any() == (value != 50)
    # without an alpha channel A is 255; three channels blend alike
    out, _ = cr.composite(frame, np.full((3, 4), 200, np.uint8), IDENTITY, opacity=128)
    assert (out == 125).all()
    f3 = np.stack([frame, frame + 10, frame + 20], axis=2)
    t4 = np.zeros((3, 4, 4), np.uint8)
    t4[..., 0], t4[..., 1], t4[..., 2], t4[..., 3] = 200, 0, 255, 100
    out, _ = cr.composite(f3, t4, IDENTITY, opacity=255)
    assert out[1, 1].tolist() == [109, (60 * 155 + 127) // 255, (25500 + 70 * 155 + 127) // 255]


def test_half_texel_shift_lands_on_the_tie_and_resolves_to_even():
    tex = (np.arange(1, 13, dtype=np.uint8).reshape(3, 4) * 20)
    frame = np.zeros((3, 4), np.uint8)
    # s * 32 = 32 u + 0.5: a tie, rounded to the even 32 u, so the texture is copied as it is
    out, painted = cr.composite(frame, tex, shifted(ds=1 / 64))
    assert np.array_equal(out, tex) and painted.all()
    # t * 32 = 32 v + 1.5 rounds to the even 32 v + 2: ay = 2; the last row would sample past the box of texel centres and is not painted
    out, painted = cr.composite(frame, tex, shifted(dt=3 / 64))
    want = (tex[:2].astype(int) * 30 * 32 * 32 + tex[1:].astype(int) * 2 * 32 * 32 + (1 << 14)) >> 15
    assert np.array_equal(out[:2], want) and painted[:2].all() and not painted[2].any() and not out[2].any()


def test_painted_set_ends_at_the_box_of_texel_centres():
    tex = (np.arange(1, 13, dtype=np.uint8).reshape(3, 4) * 20)
    frame = np.full((3, 8), 7, np.uint8)
    # s = u / 32 + 3 - 2 / 32: is = u + 94 with the limit 32 (4 - 1) = 96, so u = 0, 1, 2 are painted and u = 3 is the first that is not
    N = np.array([1 / 32, 0, 3 - 2 / 32, 0, 1, 0, 0, 0, 1.0])
    out, painted = cr.composite(frame, tex, N)
    assert painted[:, :3].all() and not painted[:, 3:].any()
    assert np.array_equal(out[:, 2], tex[:, 3]) and (out[:, 3:] == 7).all()       # is = 96 is the last texel itself
    # s = (u - 1) / 32: is = -1 at u = 0 is out, is = 0 at u = 1 is in
    out, painted = cr.composite(frame, tex, np.array([1 / 32, 0, -1 / 32, 0, 1, 0, 0, 0, 1.0]))
    assert not painted[:, 0].any() and painted[:, 1:].all() and np.array_equal(out[:, 1], tex[:, 0])
    # a 1 x 1 texture paints exactly the pixels whose position rounds to its centre
    out, painted = cr.composite(frame, np.array([[99]], np.uint8), shifted(ds=-2, dt=-1))
    assert painted.sum() == 1 and out[1, 2] == 99
    # Q <= 0, NaN, Inf and a saturated position leave the frame alone
    for N in (np.array([1, 0, 0, 0, 1, 0, 0, 0, -1.0]), np.array([1, 0, 0, 0, np.nan, 0, 0, 0, 1.0]), np.array([1, 0, np.inf, 0, 1, 0, 0, 0, 1.0]),
              np.array([1e12, 0, 1e12, 0, 1e12, 1e12, 0, 0, 1.0])):
        out, painted = cr.composite(frame, tex, N)
        assert not painted.any() and (out == 7).all()


def forward(M, s, t, K, dist):
    """rectify_ref.positions at the window positions (s, t) instead of its integer grid: (px, py). positions() builds its grid with one
    np.meshgrid call and nothing else; handing it (t, s) there runs its own projection and lens code on them, unrestated."""
    with mock.patch.object(np, "meshgrid", return_value=(t, s)):
        qx, qy, ok = rr.positions(M, s.shape[1], s.shape[0], K, dist)
    assert ok.all()
    return qx / 32, qy / 32


@pytest.mark.parametrize("ndist", [0, 4, 5, 8])
def test_painted_positions_project_back_onto_their_pixels(ndist):
    """Consistency with rectification: for every pixel the reference paints, (s, t) pushed forward through rectify_ref.positions with the M
    its N came from returns (u, v): within 1e-9 px without distortion (the two are inverse projective maps in double) and 1e-6 px with
    (five fixed-point iterations of the inverse lens model leave about 1e-8 px at these coefficients)."""
    from tests.test_gpu_rectify import DIST8, K_SMALL, POSE_LIKE

    W, H, TW, TH = 96, 64, 70, 50
    dist = DIST8[:ndist] if ndist else None
    worst, total = 0.0, 0
    for M in POSE_LIKE:
        N, valid = cr.inverse_map(M)
        assert valid == 1
        qs, qt, ok = cr.positions(N, W, H, K_SMALL, dist)
        i_s, i_t = cr.fixed(qs, ok), cr.fixed(qt, ok)
        painted = ok & (i_s >= 0) & (i_s <= 32 * (TW - 1)) & (i_t >= 0) & (i_t <= 32 * (TH - 1))
        v, u = np.nonzero(painted)
        px, py = forward(M, (qs[painted] / 32)[None, :], (qt[painted] / 32)[None, :], K_SMALL, dist)
        worst = max(worst, np.max(np.abs(px[0] - u)), np.max(np.abs(py[0] - v)))
        total += len(u)
    print("ndist %d: %d painted pixels, largest error %.3g px" % (ndist, total, worst))
    assert total > 5 * 2000
    assert worst <= (1e-6 if ndist else 1e-9)


def test_inverse_map_is_signed_for_the_camera_side():
    """det < 0 (a window handed the other way, flip_y) negates N, so that Q > 0 still means in front of the camera; no pose and a
    singular M are invalid."""
    win = dict(x0=-0.07, y0=-0.05, ux=0.002, uy=0.0, vx=0.0, vy=0.002)
    flipped = dict(win, y0=0.05, vy=-0.002)
    for w in (win, flipped):
        N, valid, M = cr.board_map((0.2, -0.1, 0.05), (0.0, 0.0, 0.25), 1, w)
        assert valid == 1
        # the ray through the window's pixel (10, 20) maps back to (10, 20) with Q > 0
        P = M.reshape(3, 3) @ np.array([10.0, 20.0, 1.0])
        assert P[2] > 0
        S = N.reshape(3, 3) @ np.array([P[0] / P[2], P[1] / P[2], 1.0])
        assert S[2] > 0 and abs(S[0] / S[2] - 10) < 1e-9 and abs(S[1] / S[2] - 20) < 1e-9
    assert np.linalg.det(cr.board_map((0.2, -0.1, 0.05), (0.0, 0.0, 0.25), 1, flipped)[2].reshape(3, 3)) < 0
    assert cr.board_map((0.2, -0.1, 0.05), (0.0, 0.0, 0.25), 0, win)[:2][1] == 0
    assert cr.inverse_map(np.array([1, 2, 3, 2, 4, 6, 0, 0, 1.0]))[1] == 0 and not cr.inverse_map(np.zeros(9))[0].any()


NEW_IDS = [7, 300, 641, 88, 1001, 412]


def test_replace_the_board_with_the_oracles_detections():
    """Paint the 3 x 2 panel, render it into three 640 x 480 frames, detect and pose with the CPU oracle, composite a panel of the same
    layout with six other ids at one texel per board pixel and opacity 255, detect again: every frame yields exactly the six new ids and
    none of the old. Measured with the oracle: 73 725, 61 739 and 63 433 pixels painted (the largest and the smallest bound the assertion),
    and the markers' corners, new against old at the same place of the layout, moved by at most 1.37, 0.28 and 0.29 px (printed, not
    asserted). The device chain of tests/test_gpu_composite.py must meet the same condition."""
    from oracle import orc

    board, ids, obj = fr.board_image(fr.PANEL, rr.RT_GRID[0], rr.RT_GRID[1], rr.RT_SIDE, rr.RT_DIST, rr.RT_IDS)
    texture, new_ids, new_obj = fr.board_image(fr.PANEL, rr.RT_GRID[0], rr.RT_GRID[1], rr.RT_SIDE, rr.RT_DIST, NEW_IDS)
    assert texture.shape == board.shape == (154, 238) and np.array_equal(new_obj, obj) and not set(NEW_IDS) & set(rr.RT_IDS)
    frames = rr.round_trip_frames(obj)
    win = cr.board_window(obj, 0, rr.RT_MARKER_M, rr.RT_SIDE / rr.RT_MARKER_M, 0.0)
    assert (win["out_width"], win["out_height"]) == (238, 154)
    det = orc.Oracle()
    for f in range(len(frames)):
        before = det.detect(frames[f], K=rr.RT_K, dist=None, marker_size=rr.RT_MARKER_M)
        assert sorted(m["id"] for m in before) == sorted(rr.RT_IDS)
        b = orc.board_detect(before, ids, obj, 0, rr.RT_K, None, rr.RT_MARKER_M)
        assert b["has_pose"] == 1
        N, valid, _ = cr.board_map(b["rvec"], b["tvec"], 1, win)
        assert valid == 1
        out, painted = cr.composite(frames[f], texture, N, rr.RT_K, None)
        after = det.detect(out, K=rr.RT_K, dist=None, marker_size=rr.RT_MARKER_M)
        assert sorted(m["id"] for m in after) == sorted(NEW_IDS), f
        old = {list(ids).index(m["id"]): np.asarray(m["corners"]).reshape(4, 2) for m in before}
        new = {list(new_ids).index(m["id"]): np.asarray(m["corners"]).reshape(4, 2) for m in after}
        moved = max(np.max(np.linalg.norm(new[k] - old[k], axis=1)) for k in old)
        print("frame %d: %d pixels painted, corners moved by at most %.2f px" % (f, painted.sum(), moved))
        assert 61739 <= painted.sum() <= 73725
