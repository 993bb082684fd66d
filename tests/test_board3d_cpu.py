"""Boards out of a plane, the reference side (runs without a GPU): tests/board3d_ref.py's restatement of solvePnP's general start recovers
generating poses, its fixtures stay clear of the planar / non-planar switch, every case the device tests rely on passes the judging gate,
arucohip_board_place equals numpy and the CPU oracle sees every marker of the rendered fold frames."""
import numpy as np
import pytest

from tests import board3d_ref as b3
from tests import pose_ref
from tests.planar_ref import rodrigues


def _fixtures():
    out = {"fold %g/%d" % (a, nm): b3.fold(nm, a) for a in b3.FOLD_ANGLES for nm in b3.FOLD_SIZES}
    out["fold 90/12"] = b3.fold(12, 90.0)
    out["fold 90/24"] = b3.fold(24, 90.0)
    for nm in (1, 16, 17):
        out["lifted %d" % nm] = b3.lifted(pose_ref.board(nm))
    ids, obj, panel = b3.fold(16, 90.0)
    out["one panel"] = (ids[panel == 1], obj[panel == 1])
    ids, obj = pose_ref.board(16)
    out["z = 0.25"] = (ids, obj + np.float32([0, 0, 0.25]))
    out["cube"] = b3.cube_faces()
    return out


def test_no_fixture_sits_near_the_switch():
    """w2 / w1 of every fixture is outside [1e-5, 1e-2]: two decades either side of the 1e-3 switch, so float32 rounding of a board file or
    another eigen-solver cannot change the branch."""
    for name, board in _fixtures().items():
        r = b3.spread_ratio(board[1])
        print("%-14s w2/w1 = %.3g" % (name, r))
        assert not (1e-5 <= r <= 1e-2), (name, r)
        planar = name.startswith(("lifted", "one panel", "z ="))
        assert (r < 1e-5) == planar, (name, r)


@pytest.mark.parametrize("name", ["fold 90/2", "fold 45/17", "fold 10/128", "cube", "lifted 1", "lifted 17", "one panel", "z = 0.25"])
def test_restatement_recovers_the_generating_pose(name):
    """Exact projections rounded to float32: the polished pose is the generating one to float32's rounding of the corners, and the start
    is already close (the linear start is exact on exact data)."""
    board = _fixtures()[name]
    for pose in b3.FOLD_POSES:
        v = b3.view(board, pose, 0.0, pose_ref.K_MAIN, seed=4100 + len(board[0]))
        ref = b3.solve(v["obj"].reshape(-1, 3), v["corners"].reshape(-1, 2), v["K"], v["dist"])
        assert ref is not None
        assert ref["branch"] == ("c" if name.startswith(("lifted", "one panel", "z =")) else "d")
        d_start = max(pose_ref.pose_dev(ref["start_rvec"], ref["start_tvec"], v["R"], v["t"]))
        d = max(pose_ref.pose_dev(ref["rvec"], ref["tvec"], v["R"], v["t"]))
        print("%-12s %-5s start %.3g final %.3g" % (name, pose, d_start, d))
        assert d < pose_ref.POSE_TOL and d_start < 0.1


def test_too_few_points_and_bad_numbers_give_no_pose():
    ids, obj, _ = b3.fold(2, 90.0)
    v = b3.view((ids, obj), "mild", 0.0, pose_ref.K_MAIN, seed=1)
    pts, px = obj.reshape(-1, 3), v["corners"].reshape(-1, 2)
    assert b3.start_pose(pts[[0, 1, 2, 4]], px[[0, 1, 2, 4]], v["K"], None) is None      # non-planar with n = 4
    bad = px.copy()
    bad[3, 0] = np.nan
    assert b3.start_pose(pts, bad, v["K"], None) is None


def test_every_case_asked_for_is_judged():
    """The gate is a condition, not a measurement: all noise-free cases and all 0.3 px cases at 90 degrees must pass it; 45 degrees with
    noise is judged where it passes."""
    cases = b3.judged_cases()
    worst = {}
    n45 = [0, 0]
    for c in cases:
        g = c["gate"]
        key = (c["angle"], c["noise"] > 0)
        w = worst.setdefault(key, [0.0, 0.0])
        if g["judged"]:
            w[0], w[1] = max(w[0], g["start_dev"]), max(w[1], g["final_dev"])
        if c["noise"] == 0 or c["angle"] == 90.0:
            assert g["judged"], (c["angle"], c["nm"], c["pose"], c["noise"], g["start_dev"], g["final_dev"])
        elif c["angle"] == 45.0:
            n45[0] += g["judged"]
            n45[1] += 1
    for (angle, noisy), (s, f) in sorted(worst.items()):
        print("fold %2g deg, %s: judged cases' worst start deviation %.3g, final %.3g" % (angle, "0.3 px" if noisy else "noise-free", s, f))
    print("45 degrees with 0.3 px: %d of %d cases judged" % tuple(n45))
    assert len([c for c in cases if c["noise"] == 0]) == 3 * 7 * 2


def test_board_place_equals_numpy():
    from aruco_amd import capi

    ids, obj = pose_ref.board(17)
    rng = np.random.default_rng(5)
    for rvec, tvec in ((b3.LIFT[0], b3.LIFT[1]), (np.zeros(3), np.array([1.0, -2.0, 3.0])), (rng.normal(size=3) * 2, rng.normal(size=3))):
        exp = (obj.reshape(-1, 3).astype(np.float64) @ rodrigues(rvec).T + tvec).astype(np.float32).reshape(-1, 4, 3)
        got = capi.board_place(obj, rvec, tvec)
        assert got.dtype == np.float32 and got.shape == obj.shape
        assert np.max(np.abs(got.astype(np.float64) - exp)) <= 1.2e-7 * np.max(np.abs(exp))   # one float32 rounding of a value equal to 1e-16
    assert np.array_equal(capi.board_place(obj, b3.LIFT[0], b3.LIFT[1]), b3.lifted((ids, obj))[1])
    L = capi.load()
    r, t = np.zeros(3), np.zeros(3)
    inplace = np.ascontiguousarray(obj).copy()
    assert L.arucohip_board_place(capi._ptr(inplace), 17, capi._ptr(b3.LIFT[0].copy()), capi._ptr(b3.LIFT[1].copy()), capi._ptr(inplace)) == capi.OK
    assert np.array_equal(inplace, b3.lifted((ids, obj))[1])
    assert L.arucohip_board_place(None, 1, capi._ptr(r), capi._ptr(t), capi._ptr(inplace)) == capi.E_INVALID
    assert L.arucohip_board_place(capi._ptr(inplace), 1, None, capi._ptr(t), capi._ptr(inplace)) == capi.E_INVALID
    assert L.arucohip_board_place(capi._ptr(inplace), -1, capi._ptr(r), capi._ptr(t), capi._ptr(inplace)) == capi.E_INVALID
    assert L.arucohip_board_place(capi._ptr(inplace), 0, capi._ptr(r), capi._ptr(t), capi._ptr(inplace)) == capi.OK


def test_oracle_detects_every_marker_of_the_rendered_fold():
    """The frames of the batch test: the CPU oracle finds all the markers each is meant to show, with the fold's ids."""
    from oracle import orc

    board, frames, shown = b3.batch_frames()
    o = orc.Oracle()
    for f, (gray, n) in enumerate(zip(frames, shown)):
        got = sorted(int(m["id"]) for m in o.detect(gray, K=b3.K_FRAME.reshape(-1), dist=None, marker_size=b3.MARKER_SIZE))
        exp = sorted(int(i) for i, p in zip(board[0], board[2]) if n == 12 or (n == 6 and p == 1))
        print("frame %d: %d markers" % (f, len(got)))
        assert got == exp, (f, got)
