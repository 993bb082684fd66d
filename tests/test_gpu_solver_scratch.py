"""What the calibration-family solvers share on a handle: their scratch, laid out and bound per call (camera calibration, marker mapping,
camera rigs, fisheye calibration), and the one pinned solver state. A handle that has grown, has run another solver, or holds a batch
in two chunks must give the bits of a fresh handle. The scenes are the host models' own (tests/*_ref.py), without their scipy solves."""
import numpy as np
import pytest

from tests import calib_ref as cr
from tests import fisheye_ref as fr
from tests import map_ref as mr
from tests import pose_ref
from tests import rig_ref as rr

pytestmark = pytest.mark.gpu


def new_handle(W=640, H=480, max_batch=1):
    import torch  # noqa: F401
    from aruco_amd import capi

    return capi.Handle(W, H, max_batch=max_batch)


def bits(r):
    """a result with every array as its bytes; the rig's camera records repeat rvecs / tvecs / calibrated"""
    if isinstance(r, list):
        return [bits(x) for x in r]
    if isinstance(r, dict):
        return {k: bits(v) for k, v in r.items() if k != "cams"}
    a = np.asarray(r)
    return (str(a.dtype), a.shape, a.tobytes())


def on_fresh_handle(call):
    h = new_handle()
    try:
        return bits(call(h))
    finally:
        h.close()


# ---- the calls: the smallest valid shape of every solver and one several times larger
def calib_call(nviews, seed):
    objs, imgs = cr.make_views(nviews, noise=0.2, seed=seed)
    return lambda h: h.calibrate_camera(objs, imgs, cr.SIZE)


def fisheye_call():
    objs, imgs = fr.make_views(12, noise=0.3)
    return lambda h: h.fisheye_calibrate(objs, imgs, (fr.W, fr.H))


def map_call(scene, noise, seed):
    obs = mr.observe(scene, noise, seed)
    return lambda h: h.board_map(*obs, len(scene["frames"]), scene["ids"], scene["K"], scene["dist"], mr.SIZE)


def rig_scene(name, noise=0.0, seed=0):
    c = rr.case(name, noise, seed, solve=False)
    return c["scene"], c["obs"]


def rig_call(name, noise=0.0, seed=0):
    from aruco_amd import capi

    sc, obs = rig_scene(name, noise, seed)
    return lambda h: h.rig_calibrate(*obs, sc["ninstants"], rr.cam_dicts(sc), sc["ids"], sc["obj"], capi.BOARD_METERS)


def rig_pose_call(name, noise=0.0, seed=0):
    from aruco_amd import capi

    sc, obs = rig_scene(name, noise, seed)
    return lambda h: h.rig_pose(*obs, sc["ninstants"], rr.cam_dicts(sc, truth=True), sc["ids"], sc["obj"], capi.BOARD_METERS)


def small_and_large(solver):
    if solver == "calib":   # 3 views of 96 points, then 20
        return calib_call(3, 7), calib_call(20, 11)
    if solver == "map":     # two markers in two frames, then the cube's six in 24 frames
        return map_call(mr.pair(), 0.0, 1000), map_call(mr.cube(102), pose_ref.NOISE, 1002)
    return rig_call("pair1"), rig_call("three", pose_ref.NOISE, 2)   # two cameras at one instant, then three at eight


@pytest.mark.parametrize("solver", ["calib", "map", "rig"])
def test_growth_and_reuse(solver):
    """small, then a shape whose scratch no longer fits (the memory is replaced and every pointer bound again), then small again in the
    larger memory: each as on a fresh handle"""
    small, large = small_and_large(solver)
    want_small, want_large = on_fresh_handle(small), on_fresh_handle(large)
    h = new_handle()
    try:
        got = [bits(call(h)) for call in (small, large, small)]
    finally:
        h.close()
    assert got[0] == want_small
    assert got[1] == want_large
    assert got[2] == want_small


def test_interleaved_solvers_share_one_handle():
    """every solver's state goes through the handle's one pinned buffer, and each has its own scratch: a call after another solver's
    gives the bits of a fresh handle"""
    calls = [("calibrate", calib_call(3, 7)), ("map", map_call(mr.pair(), 0.0, 1000)), ("rig calibrate", rig_call("pair2")),
             ("rig pose", rig_pose_call("pair2")), ("fisheye calibrate", fisheye_call()), ("calibrate again", calib_call(3, 7))]
    want = [on_fresh_handle(call) for _, call in calls]
    h = new_handle()
    try:
        got = [bits(call(h)) for _, call in calls]
    finally:
        h.close()
    for (name, _), g, w in zip(calls, got, want):
        assert g == w, name


# ---- batch owner: the scratch is that of the first chunk's worker
STREAM_W, STREAM_H, STREAM_FRAMES, STREAM_MIN_MARKERS = 960, 540, 4, 8


def _stream_results(monkeypatch, streams, host, bc, K):
    from aruco_amd import capi

    monkeypatch.setenv("ARUCOHIP_STREAMS", str(streams))
    h = capi.Handle(STREAM_W, STREAM_H, max_batch=STREAM_FRAMES)
    monkeypatch.delenv("ARUCOHIP_STREAMS")
    try:
        markers = h.detect_batch_host(host)
        if streams > 1:
            assert h.batch_chunks()[0] == streams
        board = [sum(int(m["id"]) in set(bc["ids"]) for m in ms) for ms in markers]
        assert min(board) >= STREAM_MIN_MARKERS, board
        calib = h.calibrate_board_batch(STREAM_FRAMES, bc["ids"], bc["obj"], bc["info_type"], (STREAM_W, STREAM_H), marker_size=0.039,
                                        min_markers=STREAM_MIN_MARKERS)
        mapped = h.board_map_batch(STREAM_FRAMES, bc["ids"], K, None, 0.039)
    finally:
        h.close()
    assert calib["used"].all() and mapped["used"].all()
    return bits(calib), bits(mapped)


def test_batch_forms_in_two_chunks_equal_one_chunk(monkeypatch):
    """the board stream of tests/test_gpu_calib.py at half its size, four frames: calibrate_board_batch and board_map_batch on a batch
    held by two workers (the solve runs in the first one's scratch) against the same batch in one chunk.
    rig_calibrate_batch: tests/test_gpu_rig.py::test_batch_forms_on_rendered_frames asserts the same."""
    import torch
    from aruco_amd import synth
    from tests.util import load_case

    _, doc = load_case("board")
    bc = doc["board_conf"]
    K = np.array([[850.0, 0, 477.5], [0, 845.0, 272.5], [0, 0, 1]], np.float32)
    frames, _ = synth.make_board_stream(STREAM_FRAMES, bc["ids"], bc["obj"], K.reshape(-1), width=STREAM_W, height=STREAM_H, seed=77, device="cuda")
    torch.cuda.synchronize()
    host = frames.cpu().numpy()
    one = _stream_results(monkeypatch, 1, host, bc, K)
    two = _stream_results(monkeypatch, 2, host, bc, K)
    assert one[0] == two[0], "calibrate_board_batch"
    assert one[1] == two[1], "board_map_batch"
