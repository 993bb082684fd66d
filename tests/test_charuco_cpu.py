"""The chessboard-corner (ChArUco) reference on the CPU: the header's symbols, the layout arithmetic of the library against charuco_ref on
every limit, the interpolation's start on exact projections, what the refinement gains on the GPU test's frames, and the share of those
frames' corners whose judgement is fragile."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from tests import charuco_ref as cr
from tests import pixref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ["arucohip_default_charuco", "arucohip_charuco_board_size", "arucohip_charuco_board_image", "arucohip_charuco_corners_batch",
       "arucohip_charuco_calibrate_batch", "arucohip_charuco_pose_batch"]


def test_new_symbols_are_declared_bound_and_exported():
    from aruco_amd import build_library, capi

    header = open(os.path.join(ROOT, "include", "arucohip.h")).read()
    names = set(subprocess.run(["nm", "-D", "--defined-only", build_library()], stdout=subprocess.PIPE, text=True, check=True).stdout.split())
    for s in NEW:
        assert re.search(r"\b%s\(" % s, header), s
        assert s in capi.SYMBOLS and s in names, s
    for t in ("arucohip_charuco_t", "arucohip_charuco_corner_t", "arucohip_charuco_opt_t"):
        assert t in header
    assert C.sizeof(capi.Charuco) == 16 and C.sizeof(capi.CharucoOpt) == 8 and capi.CHARUCO_CORNER_DTYPE.itemsize == 32


def _sweep():
    """layouts on and one past every limit of the header"""
    out = [(5, 4, 100, 70), (2, 2, 9, 7), (3, 3, 9, 7), (64, 2, 9, 7), (2, 64, 9, 7), (1, 4, 9, 7), (65, 2, 9, 7), (4, 1, 9, 7), (2, 65, 9, 7),
           (3, 3, 9, 6), (3, 3, 8, 7), (3, 3, 10, 8), (3, 3, 9, 8), (3, 3, 7, 7), (3, 3, 20, 19), (3, 3, 100, 7), (0, 0, 0, 0), (3, 3, -5, -9)]
    out += [(28, 20, 9, 7), (28, 21, 9, 7), (20, 28, 9, 7), (33, 17, 9, 7), (34, 17, 9, 7)]          # 513, 540, 513, 512, 528 inner corners
    out += [(64, 9, 9, 7), (64, 10, 9, 7), (58, 10, 9, 7)]                                          # 504, 567 and 513 corners (1024 markers never fit within 512 corners)
    out += [(2, 2, 8191, 7), (2, 2, 8192, 7), (3, 2, 5461, 5459), (3, 2, 5462, 7), (2, 3, 5461, 7), (2, 3, 5462, 5000)]   # 16382, 16384, 16383, 16386 a side
    out += [(2, 2, 16383, 7), (2, 2, 1 << 30, 7), (64, 64, 1 << 26, 7)]
    return out


def test_board_size_equals_the_reference_on_every_limit():
    from aruco_amd import capi

    seen = {True: 0, False: 0}
    for L in _sweep():
        want = cr.board_size(L)
        lay = capi.charuco_layout(L[:2], L[2], L[3])
        if want is None:
            with pytest.raises(capi.ArucoHipError) as e:
                capi.charuco_board_size(lay)
            assert e.value.code == capi.E_INVALID, L
        else:
            assert capi.charuco_board_size(lay) == want, L
        seen[want is not None] += 1
    assert seen[True] >= 10 and seen[False] >= 15
    # the limits themselves
    assert cr.board_size((64, 2, 9, 7)) and not cr.board_size((65, 2, 9, 7)) and cr.board_size((3, 3, 9, 7)) and not cr.board_size((3, 3, 9, 6))
    assert cr.board_size((3, 3, 9, 7)) and not cr.board_size((3, 3, 8, 7)) and cr.board_size((33, 17, 9, 7))[3] == 512 and not cr.board_size((28, 20, 9, 7))
    assert cr.board_size((3, 2, 5461, 7))[0] == 16383 and not cr.board_size((2, 2, 8192, 7))


def test_layout_numbering():
    L = cr.LAYOUT
    assert cr.board_size(L) == (500, 400, 10, 12)
    assert cr.white_squares(L)[:3] == [(1, 0), (3, 0), (0, 1)]
    assert [k for k, _ in cr.neighbours(L, 0)] == [0, 2] and [k for k, _ in cr.neighbours(L, 1)] == [0, 3] and cr.corner_xy(L, 5) == (200, 200)
    img = cr.board_image(L, cr.IDS)
    assert img[0, 0] == 0 and img[0, 100] == 255 and img[14, 114] == 255 and img[15, 115] == 0 and img[100, 100] == 0 and img[99, 99] == 0
    obj, cobj = cr.objects(L, centered=True)
    assert obj[0].tolist() == [[-135, -185, 0], [-65, -185, 0], [-65, -115, 0], [-135, -115, 0]] and cobj[0].tolist() == [-150, -100, 0]


def test_start_is_exact_for_exact_projections():
    """marker corners that are exact projections of one homography (float64, not rounded): the start is the corner's projection to 1e-9 px"""
    L = (7, 5, 60, 44)
    ids = list(range(100, 100 + cr.board_size(L)[2]))
    Hm = np.array([[1.1, 0.12, 40.0], [-0.07, 0.95, 25.0], [1.5e-4, -0.8e-4, 1.0]])

    def proj(p):
        p = np.asarray(p, np.float64).reshape(-1, 2)
        q = np.concatenate([p, np.ones((len(p), 1))], axis=1) @ Hm.T
        return q[:, :2] / q[:, 2:3]

    worst = 0.0
    for c in range(cr.board_size(L)[3]):
        X, Y = cr.corner_xy(L, c)
        ps = []
        for k, s in cr.neighbours(L, c):
            h = cr.homography4(cr.marker_quad(L, s), proj(cr.marker_quad(L, s)))
            w = h[6] * X + h[7] * Y + 1.0
            ps.append(((h[0] * X + h[1] * Y + h[2]) / w, (h[3] * X + h[4] * Y + h[5]) / w))
        start = np.mean(np.array(ps), axis=0)
        worst = max(worst, float(np.max(np.abs(start - proj([[X, Y]])[0]))))
    assert worst < 1e-9, worst
    # and through interpolate(), whose marker corners are float32: the start moves by no more than the rounding of the corners allows
    markers = [(ids[k], proj(cr.marker_quad(L, s)).astype(np.float32)) for k, s in enumerate(cr.white_squares(L))]
    rec = cr.interpolate(L, ids, markers, 2000, 2000)
    for c, r in enumerate(rec):
        assert r["markers"] == 2 and r["found"] and r["win"] == 5
        assert np.max(np.abs(r["start"] - proj([cr.corner_xy(L, c)])[0])) < 1e-3


@pytest.fixture(scope="module")
def judged():
    """Every corner of the GPU test's rendered frames that the reference finds from the marker quads a detector gives (the CPU oracle's
    detection of the frame): (scene, corner, start, win, true position, pixref's reference)."""
    from oracle import orc

    o = orc.Oracle()
    out = []
    for name in cr.BATCH:
        frame, truth, _ = cr.frame(name)
        if truth is None:
            continue
        markers = [(m["id"], np.asarray(m["corners"], np.float32).reshape(4, 2)) for m in o.detect(frame)]
        for c, r in enumerate(cr.interpolate(cr.LAYOUT, cr.IDS, markers, cr.W, cr.H)):
            if r["found"]:
                out.append((name, c, r, truth[c], pixref.reference_on(frame, "subpix", r["start32"], r["win"])))
    return out


def test_refined_corners_are_closer_to_the_truth_than_the_starts(judged):
    """The reason for the refinement, as a condition without a tolerance: over the GPU test's frames the refined corners are on average closer
    to the true corners than the starts the markers give. The marker quads are the CPU oracle's detections of those frames: with the TRUE
    quads the start is the true corner to the float32 rounding of the quads (1e-5 px here, test_start_is_exact_for_exact_projections) and
    nothing can come closer; both figures are printed. The worst refined distance is printed for charuco_ref.REFINED_WORST_PX."""
    start = np.array([np.linalg.norm(r["start32"].astype(np.float64) - t) for _, _, r, t, _ in judged])
    refined = np.array([np.linalg.norm(ref["exact"] - t) for _, _, _, t, ref in judged])
    exact_start, exact_refined = [], []
    for name in cr.BATCH:
        frame, truth, _ = cr.frame(name)
        if truth is None:
            continue
        tm = cr.true_markers(name, cover=(cr.COVERED,) if name == "covered" else ())
        for c, r in enumerate(cr.interpolate(cr.LAYOUT, cr.IDS, tm, cr.W, cr.H)):
            if r["found"]:
                exact_start.append(np.linalg.norm(r["start32"].astype(np.float64) - truth[c]))
                exact_refined.append(np.linalg.norm(pixref.subpix(frame, tuple(r["start32"]), r["win"])["pt"] - truth[c]))
    print("corners %d: detected quads: start mean %.4f px, refined mean %.4f px, refined worst %.4f px; true quads: start mean %.2e px, "
          "refined mean %.4f px, refined worst %.4f px" % (len(judged), start.mean(), refined.mean(), refined.max(), np.mean(exact_start),
                                                           np.mean(exact_refined), np.max(exact_refined)))
    assert len(judged) >= 40
    assert refined.mean() < start.mean()
    print("charuco_ref.REFINED_WORST_PX = %.3f (recorded), %.3f (now)" % (cr.REFINED_WORST_PX, np.max(exact_refined)))


def test_fragile_share_is_capped(judged):
    """window-fragile corners and pixref's fragile kinds together stay within pixref.FRAGILE_CAP of the judged corners"""
    fragile = [(n, c) for n, c, r, _, ref in judged if r["fragile"] or ref["fragile"]]
    print("fragile %d of %d: %s" % (len(fragile), len(judged), fragile))
    assert len(fragile) <= pixref.FRAGILE_CAP * len(judged)
    # the corners the reference does not find are window-fragile no more often
    for name in cr.BATCH:
        frame, truth, _ = cr.frame(name)
        if truth is not None:
            tm = cr.true_markers(name, cover=(cr.COVERED,) if name == "covered" else ())
            assert sum(r["fragile"] for r in cr.interpolate(cr.LAYOUT, cr.IDS, tm, cr.W, cr.H)) == 0, name
