"""Marker mapping on the device (arucohip_board_map / arucohip_board_map_batch): exact and noisy synthetic scenes against the truth and
against the scipy solve of tests/map_ref.py, the smallest shapes, which observations count, the limits and errors, determinism,
board_detect on the returned object points, and a rendered stream left on the device."""
import numpy as np
import pytest

from tests import map_ref as mr
from tests import pose_ref

pytestmark = pytest.mark.gpu

TOL = pose_ref.POSE_TOL * mr.SIZE   # metres on a corner position
# the device's error against the truth over the scipy solve's, in the noisy test: measured 1.000001, 0.999779 and 1.000001 on the three seeds
# (DESIGN.md "Marker mapping"), twice that allowed
TRUTH_RATIO = 2.0


@pytest.fixture(scope="module")
def handle():
    import torch  # noqa: F401
    from aruco_amd import capi

    h = capi.Handle(mr.W, mr.H, max_batch=1)
    yield h
    h.close()


def run_case(handle, c):
    sc = c["scene"]
    return handle.board_map(*c["obs"], c["nframes"], sc["ids"], sc["K"], sc["dist"], mr.SIZE)


def run_scene(handle, sc, obs, board_ids=None, nframes=None):
    return handle.board_map(*obs, len(sc["frames"]) if nframes is None else nframes, sc["ids"] if board_ids is None else board_ids, sc["K"],
                            sc["dist"], mr.SIZE)


def same_bits(a, b, nframes=None):
    for k in ("obj", "marker_rvecs", "marker_tvecs", "mapped", "marker_rms"):
        assert a[k].tobytes() == b[k].tobytes(), k
    for k in ("used", "frame_rvecs", "frame_tvecs"):
        assert a[k][:nframes].tobytes() == b[k][:nframes].tobytes(), k
    assert a["rms"] == b["rms"] and a["iterations"] == b["iterations"]


def test_exact_observations(handle):
    c = mr.case("cube", 0.0, 0)
    r = run_case(handle, c)
    dev = mr.obj_dev(r["obj"], mr.truth_obj(c["scene"]))
    print("exact cube: corner error %.3g m, rms %.3g px, %d steps" % (dev, r["rms"], r["iterations"]))
    assert r["mapped"].all() and np.array_equal(r["used"], c["ref"]["used"])
    assert dev < TOL and r["rms"] < 1e-3
    assert r["obj"].dtype == np.float32 and r["obj"].shape == (6, 4, 3)
    assert np.all(r["marker_rvecs"][0] == 0) and np.all(r["marker_tvecs"][0] == 0)
    assert np.all(r["marker_rms"] < 1e-3) and r["iterations"] >= 1


@pytest.mark.parametrize("seed", [1, 2, 3])
def test_noisy_observations_equal_scipy(handle, seed):
    c = mr.case("cube", pose_ref.NOISE, seed)
    ref = c["ref"]
    r = run_case(handle, c)
    truth = mr.truth_obj(c["scene"])
    dev, rel = mr.obj_dev(r["obj"], ref["obj"]), abs(r["rms"] - ref["rms"]) / ref["rms"]
    e_dev, e_ref = mr.obj_dev(r["obj"], truth), mr.obj_dev(ref["obj"], truth)
    print("noisy cube %d: against scipy %.3g m, rms %.9g / %.9g (rel %.3g), against the truth %.6g m (scipy %.6g m, ratio %.6f), %d steps"
          % (seed, dev, r["rms"], ref["rms"], rel, e_dev, e_ref, e_dev / e_ref, r["iterations"]))
    assert r["mapped"].all() and np.array_equal(r["used"], ref["used"])
    assert dev < TOL
    assert rel < 1e-6
    assert e_dev <= TRUTH_RATIO * e_ref
    assert np.max(np.abs(r["marker_rms"] - ref["marker_rms"])) < 1e-5
    for f in np.nonzero(r["used"])[0]:
        assert max(pose_ref.pose_dev(r["frame_rvecs"][f], r["frame_tvecs"][f], ref["frame_rvecs"][f], ref["frame_tvecs"][f])) < pose_ref.POSE_TOL


@pytest.mark.parametrize("name", ["pair", "pair180", "chain"])
def test_smallest_shapes(handle, name):
    """two markers in two frames (the 6 x 6 reduced system), the second marker turned 180 degrees about x, and the chain of four whose
    first and last panels are never seen together"""
    c = mr.case(name)
    r = run_case(handle, c)
    dev = mr.obj_dev(r["obj"], mr.truth_obj(c["scene"]))
    print("%s: corner error %.3g m, against scipy %.3g m, rms %.3g px, %d steps" % (name, dev, mr.obj_dev(r["obj"], c["ref"]["obj"]), r["rms"], r["iterations"]))
    assert r["mapped"].all() and r["used"].all()
    assert dev < TOL and r["rms"] < 1e-3
    assert mr.obj_dev(r["obj"], c["ref"]["obj"]) < TOL


def test_frames_that_do_not_count_change_nothing(handle):
    c = mr.case("cube", pose_ref.NOISE, 1)
    sc = c["scene"]
    fr, ids, cs = c["obs"]
    n = c["nframes"]
    base = run_case(handle, c)
    # frame n: one listed marker; frame n + 1: unlisted ids only; frame 0: an unlisted id and a repeat of its first id with other corners
    extra_f = np.array([0, 0, n, n + 1, n + 1], np.int32)
    extra_i = np.array([999, ids[0], sc["ids"][0], 998, 999], np.int32)
    extra_c = np.stack([cs[0], cs[0] + 5.0, cs[0], cs[0], cs[1]]).astype(np.float32)
    order = np.argsort(np.concatenate([fr, extra_f]), kind="stable")
    obs2 = tuple(np.concatenate([a, b])[order] for a, b in ((fr, extra_f), (ids, extra_i), (cs, extra_c)))
    more = run_scene(handle, sc, obs2, nframes=n + 2)
    assert not more["used"][n] and not more["used"][n + 1]
    assert np.all(more["frame_rvecs"][n:] == 0) and np.all(more["frame_tvecs"][n:] == 0)
    same_bits(base, more, nframes=n)


def test_seventeen_markers_in_a_frame(handle):
    sc = mr.grid(17)
    obs = mr.observe(sc)
    per_frame, used = mr.select(obs, len(sc["frames"]), sc["ids"], sc["K"], sc["dist"])
    sv = mr.start_values(per_frame, used, 17)
    r = run_scene(handle, sc, obs)
    assert int(r["used"].sum()) == int(sv["used"].sum()) == len(sc["frames"])
    assert np.array_equal(r["mapped"], sv["mapped"]) and r["mapped"].all()
    assert mr.obj_dev(r["obj"], mr.truth_obj(sc)) < TOL and r["rms"] < 1e-3


def test_sixty_four_markers_and_one_more(handle):
    from aruco_amd import capi

    sc = mr.grid(64, windows=True)
    obs = mr.observe(sc)
    r = run_scene(handle, sc, obs)
    print("64 markers: corner error %.3g m, rms %.3g px, %d steps" % (mr.obj_dev(r["obj"], mr.truth_obj(sc)), r["rms"], r["iterations"]))
    assert r["mapped"].all() and r["used"].all()
    assert mr.obj_dev(r["obj"], mr.truth_obj(sc)) < TOL and r["rms"] < 1e-3
    with pytest.raises(capi.ArucoHipError) as e:
        run_scene(handle, sc, obs, board_ids=np.arange(65, dtype=np.int32) + 200)
    assert e.value.code == capi.E_CAPACITY


def test_errors_and_unconnected_markers(handle):
    from aruco_amd import capi

    c = mr.case("chain")
    sc = c["scene"]
    fr, ids, cs = c["obs"]
    board = sc["ids"]
    # the reference marker is never seen
    hide = ids != board[0]
    with pytest.raises(capi.ArucoHipError) as e:
        run_scene(handle, sc, (fr[hide], ids[hide], cs[hide]))
    assert e.value.code == capi.E_INVALID
    # the last panel only in frames of its own: not mapped, zeros, and the others as if it were not listed
    with3 = [f for f, s in enumerate(sc["show"]) if 3 in s]
    keep = ~((ids == board[2]) & np.isin(fr, with3))
    obs = (fr[keep], ids[keep], cs[keep])
    r = run_scene(handle, sc, obs)
    three = run_scene(handle, sc, obs, board_ids=board[:3])
    assert r["mapped"].tolist() == [True, True, True, False]
    assert np.all(r["obj"][3] == 0) and np.all(r["marker_rvecs"][3] == 0) and np.all(r["marker_tvecs"][3] == 0) and r["marker_rms"][3] == 0
    assert not r["used"][with3].any()
    assert np.max(np.abs(r["obj"][:3].astype(np.float64) - three["obj"])) < 1e-9 and abs(r["rms"] - three["rms"]) < 1e-12
    assert mr.obj_dev(r["obj"][:3], mr.truth_obj(sc)[:3]) < TOL
    # only the reference marker is connected: fewer than two mapped
    only0 = np.isin(fr, with3) | (ids == board[0])
    with pytest.raises(capi.ArucoHipError) as e:
        run_scene(handle, sc, (fr[only0], ids[only0], cs[only0]))
    assert e.value.code == capi.E_INVALID
    for kw in (dict(board_ids=board[:1]), dict(K=None), dict(dist=np.zeros(8)), dict(size=0.0)):
        with pytest.raises(capi.ArucoHipError) as e:
            handle.board_map(fr, ids, cs, c["nframes"], kw.get("board_ids", board), kw.get("K", sc["K"]), kw.get("dist", sc["dist"]), kw.get("size", mr.SIZE))
        assert e.value.code == capi.E_INVALID, kw
    # the handle still maps
    assert run_case(handle, c)["mapped"].all()


def test_island_of_two_markers(handle):
    """panels 2 and 3 of the chain see each other but never panels 0 and 1: their frames show two listed markers, yet neither marker is
    mapped and the frames are not used; the two connected panels come out as if the island were not listed"""
    c = mr.case("chain")
    sc = c["scene"]
    obs, frames = mr.island(c)
    ref = mr.reference(obs, c["nframes"], sc["ids"], sc["K"], sc["dist"])
    r = run_scene(handle, sc, obs)
    two = run_scene(handle, sc, obs, board_ids=sc["ids"][:2])
    assert r["mapped"].tolist() == ref["mapped"].tolist() == [True, True, False, False]
    assert np.array_equal(r["used"], ref["used"]) and not r["used"][frames].any()
    assert np.all(r["obj"][2:] == 0) and np.all(r["marker_rvecs"][2:] == 0) and np.all(r["marker_tvecs"][2:] == 0) and np.all(r["marker_rms"][2:] == 0)
    assert np.all(r["frame_rvecs"][frames] == 0) and np.all(r["frame_tvecs"][frames] == 0)
    assert np.max(np.abs(r["obj"][:2].astype(np.float64) - two["obj"])) < 1e-9 and abs(r["rms"] - two["rms"]) < 1e-12
    assert mr.obj_dev(r["obj"][:2], mr.truth_obj(sc)[:2]) < TOL and mr.obj_dev(r["obj"][:2], ref["obj"][:2]) < TOL


def test_bit_reproducible_and_device_input(handle):
    import torch

    c = mr.case("cube", pose_ref.NOISE, 2)
    sc = c["scene"]
    a, b = run_case(handle, c), run_case(handle, c)
    same_bits(a, b)
    fr, ids, cs = (torch.from_numpy(x).cuda() for x in c["obs"])
    d = handle.board_map_device(fr.data_ptr(), ids.data_ptr(), cs.data_ptr(), len(c["obs"][0]), c["nframes"], sc["ids"], sc["K"], sc["dist"], mr.SIZE)
    same_bits(a, d)


def test_board_detect_takes_the_map(handle):
    from aruco_amd import capi

    c = mr.case("cube", pose_ref.NOISE, 1)
    sc = c["scene"]
    fr, ids, cs = c["obs"]
    r = run_case(handle, c)
    f = int(np.nonzero(np.bincount(fr, minlength=c["nframes"]) == 3)[0][0])
    m = np.zeros(3, capi.MARKER_DTYPE)
    m["id"], m["corners"] = ids[fr == f], cs[fr == f]
    b = handle.board_detect(m, sc["ids"], r["obj"], capi.BOARD_METERS, K=sc["K"], dist=sc["dist"], marker_size=mr.SIZE)
    d = pose_ref.pose_dev(b["rvec"], b["tvec"], r["frame_rvecs"][f], r["frame_tvecs"][f])
    print("board_detect on the mapped cube against the frame pose of the map: %.3g" % max(d))
    assert b["has_pose"] == 1 and len(b["markers"]) == 3
    assert max(d) < pose_ref.POSE_TOL


@pytest.mark.parametrize("streams", [1, 2], ids=["one_chunk", "two_chunks"])
def test_rendered_stream(monkeypatch, streams):
    """the folded board of tests/board3d_ref.py rendered at five poses (one frame shows one panel, one is empty): detect_batch, then the map
    from the device-resident markers against the scipy solve on the same detected corners; a single-frame detect() before and after"""
    import torch  # noqa: F401
    from aruco_amd import capi
    from tests import board3d_ref as b3

    board, frames, _ = b3.batch_frames()
    ids = board[0]
    KF = b3.K_FRAME.astype(np.float32)
    monkeypatch.setenv("ARUCOHIP_STREAMS", str(streams))
    h = capi.Handle(b3.W, b3.H, max_batch=5)
    monkeypatch.delenv("ARUCOHIP_STREAMS")
    try:
        before = [h.detect(frames[0]) for _ in range(3)]   # the third replays the captured single-frame graph
        markers = h.detect_batch_host(frames)
        if streams > 1:
            assert h.batch_chunks()[0] == 2
        r = h.board_map_batch(5, ids, KF, None, mr.SIZE)
        again = h.board_map_batch(5, ids, KF, None, mr.SIZE)
        seven = h.board_map_batch(5, ids, KF, None, mr.SIZE, min_markers=7)   # frame 2 shows six markers
        after = h.detect(frames[0])
    finally:
        h.close()
    obs = (np.concatenate([np.full(len(m), f, np.int32) for f, m in enumerate(markers)]), np.concatenate([m["id"] for m in markers]).astype(np.int32),
           np.concatenate([m["corners"] for m in markers]).astype(np.float32).reshape(-1, 8))
    ref = mr.reference(obs, 5, ids, b3.K_FRAME, None)
    dev, rel = mr.obj_dev(r["obj"], ref["obj"]), abs(r["rms"] - ref["rms"]) / ref["rms"]
    print("rendered fold: against scipy %.3g m, rms %.6g px (rel %.3g), against the drawing %.3g m, %d steps"
          % (dev, r["rms"], rel, mr.obj_dev(r["obj"], mr.truth_obj({"T": mr.relative_to_first(_placements(board[1]))})), r["iterations"]))
    assert r["mapped"].all() and r["used"].tolist() == ref["used"].tolist() == [True, True, True, False, True]
    assert dev < TOL and rel < 1e-6
    same_bits(r, again)
    assert seven["used"].tolist() == [True, True, False, False, True] and seven["mapped"].all()
    assert len(after) > 0
    for b in before:
        assert np.asarray(b).tobytes() == np.asarray(after).tobytes()


def _placements(obj):
    """(R, t) of markers given by their corners [n][4][3] in the order of Marker::getObjectPoints."""
    out = []
    for q in np.asarray(obj, np.float64):
        x, y = q[3] - q[0], q[1] - q[0]
        x, y = x / np.linalg.norm(x), y / np.linalg.norm(y)
        out.append((np.stack([x, y, np.cross(x, y)], axis=1), q.mean(axis=0)))
    return out
