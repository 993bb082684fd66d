"""The call-scratch arena of a handle (arucohip_handle::scratch): different entry points carve the same memory one after the other, so
the one new way to go wrong is two of them aliasing each other. Every case runs a chain of different entry points on one handle and
asks for the bytes each call gives alone on a fresh handle.

The scene is 160 x 120 views of a board of four markers, cap 8, the cube mesh and a window of 22 x 22 pixels. The ChArUco cases need
that board's frames and take charuco_ref's 640 x 480 ones."""
import ctypes as C

import numpy as np
import pytest

from tests import charuco_ref as cr
from tests import recover_ref as rr

pytestmark = pytest.mark.gpu

W, H, CAP = 160, 120, 8
K = np.array([[150.0, 0, 80.0], [0, 150.0, 60.0], [0, 0, 1.0]])
KF = K.astype(np.float32)
MS = rr.MARKER_SIZE
POSES = (((0.1, -0.15, 0.03), (0.0, 0.0, 0.2)), ((-0.12, 0.1, -0.05), (0.003, -0.002, 0.21)))


def board4():
    """Two columns x two rows of tests/golden's board, centred: ids [4], obj [4][4][3] in board units."""
    ids, obj = rr.board12()
    pick = [0, 1, 4, 5]
    obj = obj[pick]
    ctr = (obj.reshape(-1, 3).min(axis=0) + obj.reshape(-1, 3).max(axis=0)) / 2
    return [ids[i] for i in pick], obj - ctr


def view(ids, obj, pose, seed):
    """synth.render_board of the board at a pose"""
    from aruco_amd import synth

    return synth.render_board(ids, obj, K, np.array(pose[0]), np.array(pose[1]), W, H, np.random.RandomState(seed), unit=rr.UNIT, pad=30.0)[0].numpy()


@pytest.fixture(scope="module")
def scene():
    import torch  # noqa: F401  (torch's HIP runtime first, see aruco_amd/capi.py)
    from aruco_amd import capi

    ids, obj = board4()
    clean = np.stack([view(ids, obj, POSES[f % 2], 5 + f) for f in range(4)])
    frames = clean[:2].copy()
    h = capi.Handle(W, H, max_batch=2)
    try:
        found = h.detect_batch_host(frames, K=KF, marker_size=MS, cap=CAP)
        boards = capi.Handle._board_records(h.board_detect_batch(2, ids, obj, rr.PIX, K=KF, marker_size=MS))
    finally:
        h.close()
    assert [len(m) for m in found] == [4, 4] and boards["has_pose"].all()
    markers = np.zeros((2, CAP), capi.MARKER_DTYPE)
    for f, m in enumerate(found):
        markers[f, :len(m)] = m
    win = capi.rectify_board_window(obj, rr.PIX, MS, 250.0, 0.0)
    assert (win.out_width, win.out_height) == (22, 22)
    tex = np.random.RandomState(3).randint(0, 256, (win.out_height, win.out_width)).astype(np.uint8)
    return {"ids": ids, "obj": obj, "frames": frames, "clean": clean, "markers": markers, "counts": np.array([4, 4], np.int32), "boards": boards,
            "win": win, "tex": tex, "mesh": capi.cube_mesh()}


def detected(sc, frames=None, max_batch=2):
    """a fresh handle that holds the detection of the scene's frames"""
    from aruco_amd import capi

    h = capi.Handle(W, H, max_batch=max_batch)
    h.detect_batch_host(sc["frames"] if frames is None else frames, K=KF, marker_size=MS, cap=CAP)
    return h


# ---------------------------------------------------------------------------------------------------------------------------------
# a chain of different entry points on one handle. Everything on the device: none of the first four synchronises (planar_poses_batch,
# the last, always does), and the arena's need goes 768 bytes of maps (rectify), the primitive lists (draw), 18 KiB of records
# (render), 768 bytes again (composite). Everything on the host: each call stages its frames and arguments in the arena as well.
# ---------------------------------------------------------------------------------------------------------------------------------
CHAIN = ("rectify", "draw", "render", "composite", "planar")


def run_device(h, sc, names):
    """the named calls back to back on device memory, one synchronisation at the end; name -> the bytes the call left"""
    import torch
    from aruco_amd import capi

    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1)).cuda()   # noqa: E731
    win = sc["win"]
    frames, markers, counts, boards = dev(sc["frames"]), dev(sc["markers"]), torch.from_numpy(sc["counts"]).cuda(), dev(sc["boards"])
    v, t = sc["mesh"]
    msh = capi.mesh(torch.from_numpy(v).cuda(), torch.from_numpy(t).cuda())
    tex = capi.texture(torch.from_numpy(sc["tex"]).cuda())
    out = {"rectify": torch.full((2 * win.out_height * win.out_width,), 0xA5, dtype=torch.uint8, device="cuda"),
           "planar": torch.full((2 * CAP * C.sizeof(capi.PlanarPoses),), 0xA5, dtype=torch.uint8, device="cuda")}
    for name in ("draw", "render", "composite"):
        out[name] = frames.clone().reshape(2, H, W)
    torch.cuda.synchronize()   # the tensors are made on torch's stream, the calls run on the handle's
    calls = {
        "rectify": lambda: h.board_rectify_device(frames.data_ptr(), 2, W, H, 1, boards, KF, win, out["rectify"].data_ptr()),
        "draw": lambda: h.draw_markers(out["draw"], markers, counts, K=KF, flags=capi.DRAW_OUTLINE | capi.DRAW_IDS | capi.DRAW_CUBE),
        "render": lambda: h.render_markers(out["render"], markers, counts, KF, msh),
        "composite": lambda: h.board_composite_device(out["composite"].data_ptr(), 2, W, H, 1, boards, KF, win, tex),
        "planar": lambda: h.planar_poses_batch_device(2, C.c_void_p(out["planar"].data_ptr()), CAP, KF, None, MS),
    }
    for name in names:
        calls[name]()
    h.synchronize()
    return {name: out[name].cpu().numpy().tobytes() for name in names}


def run_host(h, sc, names):
    """the same calls on host memory (each synchronises)"""
    from aruco_amd import capi

    v, t = sc["mesh"]
    calls = {
        "rectify": lambda: h.board_rectify(sc["frames"], sc["boards"], KF, sc["win"])[0],
        "draw": lambda: h.draw_markers(sc["frames"].copy(), sc["markers"], sc["counts"], K=KF, flags=capi.DRAW_OUTLINE | capi.DRAW_IDS | capi.DRAW_CUBE),
        "render": lambda: h.render_markers(sc["frames"].copy(), sc["markers"], sc["counts"], KF, capi.mesh(v, t)),
        "composite": lambda: h.board_composite(sc["frames"], sc["boards"], KF, sc["win"], sc["tex"])[0],
        "planar": lambda: h.planar_poses_batch(2, KF, None, MS, cap=CAP, fill=0xA5),
    }
    return {name: bytes(calls[name]()) if name == "planar" else calls[name]().tobytes() for name in names}


def test_chain_equals_every_call_alone(scene):
    """Device memory without a synchronisation between the calls, then host memory on the same handle; each call alone on a fresh
    handle gives the reference. Two fresh handles must agree first, or byte equality proves nothing."""
    alone = {}
    for name in CHAIN:
        for run in (run_device, run_host):
            got = []
            for _ in range(2):
                h = detected(scene)
                try:
                    got.append(run(h, scene, (name,))[name])
                finally:
                    h.close()
            assert got[0] == got[1], "two fresh handles disagree on %s (%s)" % (name, run.__name__)
            alone[name, run.__name__] = got[0]
    for name in ("draw", "render", "composite"):
        assert alone[name, "run_host"] != scene["frames"].tobytes(), name + " painted nothing"
    assert any(alone["rectify", "run_host"]) and alone["planar", "run_host"] != bytes([0xA5]) * len(alone["planar", "run_host"])
    h = detected(scene)
    try:
        for run in (run_device, run_host, run_device):
            got = run(h, scene, CHAIN)
            for name in CHAIN:
                assert got[name] == alone[name, run.__name__], "%s in the chain (%s) differs from the call alone" % (name, run.__name__)
    finally:
        h.close()


# ---------------------------------------------------------------------------------------------------------------------------------
# memory that outlives a call is not in the arena
# ---------------------------------------------------------------------------------------------------------------------------------
def test_resident_charuco_corners_survive_a_growing_arena():
    """charuco_corners_batch leaves its corners on the device; a host-frame rectify of the nine frames (2.7 MB staged) grows the arena
    before the two consumers read them. charuco_calibrate_batch gathers its views outside the arena and calls calibrate_camera, which
    carves it."""
    import torch  # noqa: F401
    from aruco_amd import capi

    L, ids = cr.CALIB_LAYOUT, cr.CALIB_IDS
    frames = np.stack([v[0] for v in cr.calib_frames()])
    n = len(frames)
    boards = np.zeros(n, capi.BOARD_DTYPE)
    boards["has_pose"], boards["tvec"] = 1, (0.0, 0.0, 0.5)
    win = capi.rectify_board_window(board4()[1], rr.PIX, MS, 2500.0, 0.0)

    def consumers(between):
        h = capi.Handle(cr.W, cr.H, max_batch=n)
        try:
            h.detect_batch_host(frames)
            rec, nf = h.charuco_corners_batch(capi.charuco_layout(L[:2], L[2], L[3]), ids, frames)
            if between:
                assert h.board_rectify(frames, boards, cr.K.astype(np.float32), win)[0].any()
            cal = h.charuco_calibrate_batch((cr.W, cr.H), square_size=0.08, min_corners=10)
            pose = h.charuco_pose_batch(n, cr.K.astype(np.float32), square_size=0.08)
            return rec.tobytes(), nf.tobytes(), [cal[k].tobytes() for k in ("K", "dist", "rvecs", "tvecs", "used")], cal["rms"], pose.tobytes()
        finally:
            h.close()

    want, got = consumers(False), consumers(True)
    assert np.frombuffer(want[1], np.int32).min() >= 4 and np.isfinite(want[3])
    assert got == want


def test_resident_board_poses_survive_a_growing_arena(scene):
    """board_detect_batch leaves its poses on the device for ChromaticMask's classify_batch, the one call that reads them there (no
    entry point hands their address out, so render_boards cannot be given them). A host-frame render_markers grows the arena in between."""
    from aruco_amd import capi

    v, t = scene["mesh"]

    def masks(between):
        h = detected(scene)
        try:
            b = h.board_detect_batch(2, scene["ids"], scene["obj"], rr.PIX, K=KF, marker_size=MS)
            m = h.chromatic(6, 6, 1e-4, KF, None, W, H, capi.chromatic_board_corners(scene["obj"], rr.PIX, MS))
            try:
                m.train(scene["frames"][0], b[0]["rvec"], b[0]["tvec"])
                if between:
                    h.render_markers(scene["frames"].copy(), scene["markers"], scene["counts"], KF, capi.mesh(v, t))
                got, npix = m.classify_batch(h, scene["frames"])
                geom = [np.concatenate([a.ravel() for a in m.debug_geometry(f)]).tobytes() for f in range(2)]
                return got.tobytes(), npix.tobytes(), geom
            finally:
                m.close()
        finally:
            h.close()

    want, got = masks(False), masks(True)
    assert any(want[2][0]) and want[2][0] != want[2][1]   # the two frames' board corners and homographies, from the resident poses
    assert got == want


# ---------------------------------------------------------------------------------------------------------------------------------
# chunk workers have an arena each
# ---------------------------------------------------------------------------------------------------------------------------------
def test_workers_carve_their_own_arenas(scene, monkeypatch):
    """Four clean frames on two chunk workers: planar poses into host memory (each worker stages its frames' results in its arena),
    marker recovery (a larger layout in the same arenas; it adopts nothing here, so the lists stay), planar poses again."""
    from aruco_amd import capi

    ids, obj = scene["ids"], scene["obj"]
    recover = lambda h: h.board_recover_batch(4, ids, obj, rr.PIX, KF, marker_size=MS, cap=CAP)   # noqa: E731

    def flat(r):
        out, n, rec, boards = r
        return [m.tobytes() for m in out], n.tobytes(), rec.tobytes(), [(b["n_markers"], b["has_pose"], b["rvec"].tobytes(), b["tvec"].tobytes()) for b in boards]

    monkeypatch.setenv("ARUCOHIP_STREAMS", "2")
    h, ref = capi.Handle(W, H, max_batch=4), capi.Handle(W, H, max_batch=4)
    monkeypatch.delenv("ARUCOHIP_STREAMS")
    try:
        for x in (h, ref):
            assert [len(m) for m in x.detect_batch_host(scene["clean"], K=KF, marker_size=MS, cap=CAP)] == [4] * 4
            assert x.batch_chunks() == (2, 2)
        first = bytes(h.planar_poses_batch(4, KF, None, MS, cap=CAP, fill=0xA5))
        rec = flat(recover(h))
        third = bytes(h.planar_poses_batch(4, KF, None, MS, cap=CAP, fill=0xA5))
        assert first == third and first != bytes([0xA5]) * len(first)
        assert rec == flat(recover(ref)) and rec[2] == np.zeros(4, np.int32).tobytes() and all(b[1] for b in rec[3])
    finally:
        h.close(), ref.close()


# ---------------------------------------------------------------------------------------------------------------------------------
# a handle's arena is used only on that handle's stream
# ---------------------------------------------------------------------------------------------------------------------------------
def test_charuco_after_a_waited_ticket_leaves_a_queued_draw_alone():
    """After a waited ticket the last batch lives on a pipeline lane with a stream of its own, and charuco_corners_batch uploads host
    frames on that stream: into the lane's arena, not into the caller's handle's, where a device draw_markers queued on the handle's
    stream and not waited for still reads its primitive lists. The corners are taken twice, so the second call finds every buffer grown."""
    import torch
    from aruco_amd import capi

    frames = np.stack([cr.frame("frontal")[0], cr.frame("tilted")[0]])
    L, cap = capi.charuco_layout(cr.LAYOUT[:2], cr.LAYOUT[2], cr.LAYOUT[3]), 16
    kf = cr.K.astype(np.float32)
    plain, h = capi.Handle(cr.W, cr.H, max_batch=2), capi.Handle(cr.W, cr.H, max_batch=2)
    try:
        found = plain.detect_batch_host(frames, K=kf, marker_size=0.07, cap=cap)
        want_rec, want_nf = plain.charuco_corners_batch(L, cr.IDS, frames)
        assert min(len(m) for m in found) >= 2 and want_nf.min() >= 4
        out, n = np.zeros((2, cap), capi.MARKER_DTYPE), np.zeros(2, np.int32)
        h.set_pipeline_depth(2)
        h.wait(h.submit_host(frames, out, n, K=kf, marker_size=0.07))
        assert [out[f, :n[f]].tobytes() for f in range(2)] == [m.tobytes() for m in found]
        dm, dn = torch.from_numpy(out.view(np.uint8).reshape(-1)).cuda(), torch.from_numpy(n).cuda()
        drawn, alone = torch.from_numpy(frames).cuda(), torch.from_numpy(frames).cuda()
        torch.cuda.synchronize()
        flags = capi.DRAW_OUTLINE | capi.DRAW_IDS | capi.DRAW_CUBE
        plain.draw_markers(alone, dm, dn, K=kf, flags=flags)
        plain.synchronize()
        h.draw_markers(drawn, dm, dn, K=kf, flags=flags)
        for _ in range(2):
            rec, nf = h.charuco_corners_batch(L, cr.IDS, frames)
            assert rec.tobytes() == want_rec.tobytes() and nf.tobytes() == want_nf.tobytes()
        h.synchronize()
        assert not torch.equal(alone.cpu(), torch.from_numpy(frames)) and torch.equal(drawn, alone)
    finally:
        plain.close(), h.close()


# ---------------------------------------------------------------------------------------------------------------------------------
# the one-frame graph reads nothing in the arena
# ---------------------------------------------------------------------------------------------------------------------------------
def test_single_frame_graph_survives_arena_calls(scene, monkeypatch):
    """Eager handle (ARUCOHIP_GRAPH=0 at creation) against the default handle, the same calls on both: detect x3 (eager, capture +
    launch, replay), a host-frame render_markers and a host-frame convert (both stage in the arena and grow it), detect x2 - identical
    bytes at every step."""
    from aruco_amd import capi

    v, t = scene["mesh"]
    a = scene["frames"][0]
    nv12 = np.concatenate([scene["frames"], np.full((2, H // 2, W), 128, np.uint8)], axis=1)
    kw = dict(K=KF, marker_size=MS)
    monkeypatch.setenv("ARUCOHIP_GRAPH", "0")
    eager = capi.Handle(W, H, max_batch=4)
    monkeypatch.delenv("ARUCOHIP_GRAPH")
    graphed = capi.Handle(W, H, max_batch=4)

    def same(call):
        want, got = call(eager), call(graphed)
        assert got.tobytes() == want.tobytes()
        return want

    try:
        assert len(same(lambda h: h.detect(a, **kw))) == 4
        for _ in range(2):
            same(lambda h: h.detect(a, **kw))
        assert same(lambda h: h.render_markers(scene["frames"].copy(), scene["markers"], scene["counts"], KF, capi.mesh(v, t))).tobytes() != scene["frames"].tobytes()
        assert same(lambda h: h.convert(nv12, capi.nv12(), 1)).shape == scene["frames"].shape
        for _ in range(2):
            assert len(same(lambda h: h.detect(a, **kw))) == 4
    finally:
        eager.close(), graphed.close()
