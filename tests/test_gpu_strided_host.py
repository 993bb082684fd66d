"""Host frames with padded rows and gaps between the frames through the C ABI, where the Python wrappers only ever pass packed arrays:
arucohip_undistort, arucohip_fisheye_undistort, arucohip_draw_markers_batch, arucohip_charuco_corners_batch and ChromaticMask's batch
classification, whose own test file has no padded host frames either. Two 37 x 19 frames, rows
of width * channels + 5 bytes, frames either 11 bytes further apart than their rows need (one copy per image) or gap-free (one copy for
the batch), 0xA5 in every byte that is no pixel. Each call's image bytes are those of the stage's own reference on the same pixels
(the oracle's cv::undistort, fisheye_ref's remap, overlay_ref's painter, charuco_ref's interpolation), and no padding byte changes.
One frame with a frame_stride of 0 is accepted by every call but ChromaticMask's, which holds a single frame's frame_stride to the
rule of several.

37 x 19 pixels hold no marker, so the ChArUco and ChromaticMask calls are pinned here on their staging, their acceptance and the
empty results of frames without markers or a board pose; test_gpu_charuco.py pins corner values read from padded host rows."""
import ctypes as C
import json
import os

import numpy as np
import pytest

from tests import charuco_ref as cr
from tests import chromatic_ref
from tests import fisheye_ref as fr
from tests import overlay_ref as ovr

pytestmark = pytest.mark.gpu

W, H, PAD, GAP, FILL = 37, 19, 5, 11, 0xA5
# (nframes, bytes between the frames beyond H rows; None: a frame_stride of 0)
LAYOUTS = [(2, GAP), (2, 0), (1, None)]
K_PIN = np.array([[31.0, 0, 18.25], [0, 30.5, 9.5], [0, 0, 1]], np.float32)
DIST = [-0.21, 0.06, 1.1e-3, -7e-4, 0.01]
K_FISH = np.array([[14.0, 0, 18.0], [0, 14.0, 9.0], [0, 0, 1]])
K_NEW = np.array([[12.0, 0, 18.0], [0, 12.0, 9.0], [0, 0, 1]])
CHARUCO = (2, 2, 9, 7)


class Strided:
    """n frames of H rows of W * ch pixels bytes in one host array filled with 0xA5: rows W * ch + 5 bytes apart, frames `gap` bytes
    further apart than H rows."""

    def __init__(self, n, ch, gap, seed):
        self.n, self.ch, self.row = n, ch, W * ch + PAD
        self.frame = 0 if gap is None else H * self.row + gap
        self.buf = np.full(max(n * self.frame, H * self.row), FILL, np.uint8)
        self.images()[...] = np.random.RandomState(seed).randint(0, 256, (n, H, W * ch))

    def images(self):
        """the pixels as [n][H][W * ch], a view"""
        return np.lib.stride_tricks.as_strided(self.buf, (self.n, H, W * self.ch), (self.frame, self.row, 1))

    def ptr(self):
        return self.buf.ctypes.data_as(C.c_void_p)

    def assert_padding_kept(self):
        pixel = np.zeros(self.buf.size, bool)
        np.lib.stride_tricks.as_strided(pixel, (self.n, H, W * self.ch), (self.frame, self.row, 1))[...] = True
        assert np.all(self.buf[~pixel] == FILL)


def shaped(img, ch):
    return img.reshape(H, W) if ch == 1 else img.reshape(H, W, 3)


@pytest.fixture(scope="module")
def env():
    import torch  # noqa: F401  (torch's HIP runtime first, see aruco_amd/capi.py)
    from aruco_amd import capi
    from oracle import orc

    h = capi.Handle(64, 64, max_batch=2)
    yield {"capi": capi, "orc": orc, "h": h}
    h.close()


@pytest.mark.parametrize("n,gap", LAYOUTS)
@pytest.mark.parametrize("ch", [1, 3])
def test_undistort(env, ch, n, gap):
    h, orc = env["h"], env["orc"]
    src = Strided(n, ch, gap, 1)
    want = src.images().copy()
    dist = np.asarray(DIST, np.float32)
    out = np.zeros((n, H, W * ch), np.uint8)
    h._chk(h.L.arucohip_undistort(h.h, src.ptr(), n, W, H, src.row, src.frame, ch, 0, K_PIN.ctypes.data_as(C.c_void_p),
                                  dist.ctypes.data_as(C.c_void_p), dist.size, out.ctypes.data_as(C.c_void_p), 0))
    for f in range(n):
        assert np.array_equal(shaped(out[f], ch), orc.undistort(shaped(want[f], ch), K_PIN, DIST)), f
    assert np.array_equal(src.images(), want)
    src.assert_padding_kept()


@pytest.fixture(scope="module")
def fisheye_table():
    table = fr.build_map(W, H, K_FISH, fr.D, K_NEW, 1.0)
    assert table[2].any() and not table[2].all()   # some of the ideal frame lies beyond the lens
    return table


@pytest.mark.parametrize("n,gap", LAYOUTS)
@pytest.mark.parametrize("ch", [1, 3])
def test_fisheye_undistort(env, fisheye_table, ch, n, gap):
    h, capi = env["h"], env["capi"]
    src = Strided(n, ch, gap, 2)
    want = src.images().copy()
    out = np.zeros((n, H, W * ch), np.uint8)
    knew = K_NEW.astype(np.float32)
    h._chk(h.L.arucohip_fisheye_undistort(h.h, src.ptr(), n, W, H, src.row, src.frame, ch, 0, capi.fisheye_models((K_FISH, fr.D)),
                                          knew.ctypes.data_as(C.c_void_p), 1.0, out.ctypes.data_as(C.c_void_p), 0))
    u32, v32, beyond = fisheye_table
    for f in range(n):
        diff = (shaped(out[f], ch) != fr.remap(shaped(want[f], ch), u32, v32, beyond)).reshape(H, W, ch).any(axis=2)
        # 1e-8: about the double evaluation error of 32 u and 32 v (test_gpu_fisheye.py)
        assert not (diff & ~fr.near_rounding_boundary(u32, v32, 1e-8)).any(), f
    assert np.array_equal(src.images(), want)
    src.assert_padding_kept()


def overlay_markers(capi, n):
    """one turned quad with its id per frame, the corners off the pixel grid"""
    ms = np.zeros((n, 1), capi.MARKER_DTYPE)
    for f in range(n):
        a = 0.3 + 0.4 * f
        c, s = np.cos(a), np.sin(a)
        pts = np.array([[-6.0, -6.0], [6.0, -6.0], [6.0, 6.0], [-6.0, 6.0]]) @ np.array([[c, s], [-s, c]]) + [17.3 + 3 * f, 9.3]
        ms[f, 0]["id"], ms[f, 0]["corners"], ms[f, 0]["ssize"] = 7 + 100 * f, pts.astype(np.float32).reshape(8), 0.05
    return ms, np.ones(n, np.int32)


@pytest.mark.parametrize("n,gap", LAYOUTS)
@pytest.mark.parametrize("ch", [1, 3])
def test_draw_markers(env, ch, n, gap):
    h, capi = env["h"], env["capi"]
    frames = Strided(n, ch, gap, 3)
    before = frames.images().copy()
    markers, counts = overlay_markers(capi, n)
    exp = before.copy()
    coords = ovr.draw_markers(exp, W, ch, markers, counts, flags=ovr.OUTLINE | ovr.IDS, line_width=1, color=(30, 200, 90))
    assert ovr.half_integer_margin(coords) >= 1e-3
    assert not np.array_equal(exp, before)
    st = capi.Overlay(ovr.OUTLINE | ovr.IDS, 1, (C.c_uint8 * 4)(30, 200, 90, 0))
    h._chk(h.L.arucohip_draw_markers_batch(h.h, frames.ptr(), n, W, H, ch, frames.row, frames.frame, 0, markers.ctypes.data_as(C.c_void_p), 1,
                                           counts.ctypes.data_as(C.c_void_p), 0, None, None, 0, C.byref(st)))
    bad = np.argwhere(frames.images() != exp)
    assert bad.size == 0, "first differing byte (frame, row, byte): %s, %d differ" % (bad[0], len(bad))
    frames.assert_padding_kept()


@pytest.mark.parametrize("n,gap", LAYOUTS)
def test_charuco_corners(env, n, gap):
    h, capi = env["h"], env["capi"]
    frames = Strided(n, 1, gap, 4)
    packed = frames.images().copy()
    found = h.detect_batch_host(packed)
    layout = capi.charuco_layout(CHARUCO[:2], CHARUCO[2], CHARUCO[3])
    _, _, nm, nc = capi.charuco_board_size(layout)
    ids = np.arange(nm, dtype=np.int32)
    rec = np.zeros((n, nc), capi.CHARUCO_CORNER_DTYPE)
    rec.view(np.uint8)[...] = 0x5A
    nf = np.full(n, -1, np.int32)
    h._chk(h.L.arucohip_charuco_corners_batch(h.h, C.byref(layout), ids.ctypes.data_as(C.c_void_p), nm, frames.ptr(), n, W, H, frames.row,
                                              frames.frame, 0, None, rec.ctypes.data_as(C.c_void_p), nf.ctypes.data_as(C.c_void_p), 0))
    for f in range(n):
        markers = [(int(m["id"]), np.asarray(m["corners"], np.float32).reshape(4, 2)) for m in found[f]]
        ref = cr.interpolate(CHARUCO, list(ids), markers, W, H)
        assert len(ref) == nc
        for g, r in zip(rec[f], ref):
            assert not r["found"] and (int(g["markers"]), int(g["found"]), int(g["win"]), int(g["pad_"])) == (r["markers"], 0, r["win"], 0)
            assert (float(g["start_x"]), float(g["start_y"])) == tuple(float(v) for v in r["start32"])
            assert (g["x"], g["y"]) == (g["start_x"], g["start_y"])
        assert nf[f] == 0
    assert np.array_equal(frames.images(), packed)
    frames.assert_padding_kept()


@pytest.mark.parametrize("n,gap", LAYOUTS)
def test_chromatic_classify_batch(env, n, gap):
    """No frame has a board pose, and a frame without one gets an empty mask (test_gpu_chromatic.py holds the batch call to that too)."""
    h, capi = env["h"], env["capi"]
    frames = Strided(n, 1, gap, 5)
    packed = frames.images().copy()
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    bc = json.load(open(os.path.join(root, "tests", "golden", "board.json")))["board_conf"]
    h.detect_batch_host(packed)
    boards = h.board_detect_batch(n, bc["ids"], bc["obj"], bc["info_type"], K=K_PIN, marker_size=0.039)
    assert not any(b["has_pose"] for b in boards)
    dev = h.chromatic(6, 6, 1e-4, K_PIN, None, W, H, chromatic_ref.board_corners(bc["obj"], bc["info_type"], 0.039))
    try:
        masks = np.full((n, H, W), 0x5A, np.uint8)
        npix = np.full(n, -1, np.int32)
        rc = h.L.arucohip_chromatic_classify_batch(dev.m, h.h, frames.ptr(), n, W, H, frames.row, frames.frame, 0, 2, 0.0,
                                                   masks.ctypes.data_as(C.c_void_p), 0, npix.ctypes.data_as(C.c_void_p))
        if gap is None:   # a frame_stride of 0: refused even for one frame, nothing written
            assert rc == capi.E_INVALID and (masks == 0x5A).all() and (npix == -1).all()
        else:
            assert rc == capi.OK and not masks.any() and not npix.any()
    finally:
        dev.close()
    assert np.array_equal(frames.images(), packed)
    frames.assert_padding_kept()
