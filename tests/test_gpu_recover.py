"""arucohip_board_recover_batch on the device against the float64 restatement (tests/recover_ref.py).

Every generated input first passes the restatement's gate: no considered pair's distance within 5 % of max_corner_dist, no mismatch
count at the limit other than a painted one. Under that gate the device's decisions equal the restatement's exactly: the same
(board entry, candidate, rotation) triples, the same ids, the same recovered[f]. Frames are 640 x 480 views of the 12-marker board."""
import ctypes as C

import numpy as np
import pytest

from tests import recover_ref as rr

pytestmark = pytest.mark.gpu

CORNER_REL_TOL = 1e-4   # LINES corners against the oracle, relative to the coordinate's magnitude: the parity tests' tolerance (test_gpu_parity.py)
POSE_TOL = 1e-4         # the project's pose tolerance (test_gpu_fullsize.py)
OBSERVED = 0.0          # largest relative deviation of boards[f] from arucohip_board_detect on the returned markers, first MI355X run: the
                        # two solve the same correspondences with the same wave solver and agreed to the bit
TOL = 10 * OBSERVED
assert TOL <= POSE_TOL

DMG = {1: [(3, 3)], 6: [(2, 2), (4, 3)], 10: [(1, 1), (1, 4), (2, 3), (3, 2), (4, 5), (5, 3)]}   # 1, 2 and 6 repainted cells
DMG2 = {0: [(2, 4)], 7: [(3, 1), (5, 5)]}
ONE_LEFT = {k: [(3, 3)] for k in range(12) if k != 4}
KF = rr.K.astype(np.float32)
DIST = [-0.10, 0.02, 1e-3, -5e-4, 0]


@pytest.fixture(scope="module")
def scene():
    import torch  # noqa: F401  (torch's HIP runtime first, see aruco_amd/capi.py)

    ids, obj = rr.board12()
    fr = {"dmg": rr.build_frame(ids, obj, DMG)[0],
          "blot": rr.build_frame(ids, obj, {9: [(3, 3)]}, corner_blots=[4], seed=6)[0],
          "single": rr.build_frame(ids, obj, ONE_LEFT, seed=7)[0],
          "clean": rr.build_frame(ids, obj, seed=8)[0],
          "dmg2": rr.build_frame(ids, obj, DMG2, rvec=np.array([-0.1, 0.15, -0.04]), tvec=np.array([0.01, -0.005, 0.45]), seed=9)[0]}
    return {"ids": ids, "obj": obj, "frames": fr, "order": ["dmg", "blot", "single", "clean", "dmg2"]}


def make_handle(max_batch=1, params=None, limits=None):
    from aruco_amd import capi

    return capi.Handle(rr.W, rr.H, max_batch=max_batch, params=params, limits=limits)


def opt_of(**kw):
    from aruco_amd import capi

    o = capi.default_recover()
    for k, v in kw.items():
        setattr(o, k, v)
    return o


def as_dicts(ms):
    return [{"id": int(m["id"]), "corners": np.array(m["corners"], np.float32).reshape(4, 2)} for m in ms]


def expect(h, frames, markers, ids, obj, opt=None, painted=(), dist=None, cells=None):
    """The restatement on the device's own lists of every frame (before the call), gated."""
    out = []
    for f, gray in enumerate(frames):
        quads, cids, _ = h.debug_candidates(f)
        if cells:
            med, thr = h.debug_cells(f), h.debug_otsu(f)
            votes = lambda ci, med=med, thr=thr: rr.votes_from_cells(med[ci], thr[ci])   # noqa: E731
        else:
            votes = lambda ci, gray=gray, quads=quads: rr.votes_from_frame(gray, quads[ci])   # noqa: E731
        res = rr.recover_frame(as_dicts(markers[f]), quads, cids, votes, ids, obj, rr.PIX, rr.K, dist=dist, opt=opt,
                               rect=rr.border_rect(rr.W, rr.H))
        rr.gate(res, opt, painted)
        res["before"] = (quads, cids)
        out.append(res)
    return out


def decisions(h, f, before, ids):
    """(board entry, candidate, rotation) of the candidates the call adopted in frame f, in board order."""
    quads, cids, nrot = h.debug_candidates(f)
    assert np.array_equal(quads, before[0])
    got = [(ids.index(int(cids[ci])), ci, int(nrot[ci])) for ci in range(len(cids)) if before[1][ci] == -1 and cids[ci] >= 0]
    assert all(before[1][ci] == cids[ci] for ci in range(len(cids)) if before[1][ci] != -1)
    return sorted(got)


def check_batch(h, frames, markers, scene, opt=None, painted=(), cells=None, **kw):
    ids, obj = scene["ids"], scene["obj"]
    exp = expect(h, frames, markers, ids, obj, opt=opt, painted=painted, cells=cells)
    o = None if opt is None else opt_of(**opt)
    out, n, rec, boards = h.board_recover_batch(len(frames), ids, obj, rr.PIX, KF, marker_size=rr.MARKER_SIZE, opt=o, **kw)
    for f in range(len(frames)):
        assert decisions(h, f, exp[f]["before"], ids) == exp[f]["adopted"], f
        assert rec[f] == len(exp[f]["adopted"]) and n[f] == len(markers[f]) + rec[f]
        want = sorted([int(m["id"]) for m in markers[f]] + [ids[a[0]] for a in exp[f]["adopted"]])
        assert [int(m["id"]) for m in out[f]] == want
        if rec[f] == 0:
            assert out[f].tobytes() == np.asarray(markers[f]).tobytes()
        assert boards[f]["n_markers"] == sum(int(m["id"]) in ids for m in out[f])
    return exp, out, n, rec, boards


def frames_of(scene, n):
    return [scene["frames"][k] for k in scene["order"][:n]]


def check_story(exp, rec, n):
    """What the frames were built for: 1 and 2 wrong cells come back at the default limit and 6 do not; a marker without a quad stays
    missing; a frame with a single member is left alone; a clean frame recovers nothing."""
    assert [a[0] for a in exp[0]["adopted"]] == [1, 6] and rec[0] == 2
    if n > 1:
        assert [a[0] for a in exp[1]["adopted"]] == [9] and rec[1] == 1
    if n > 2:
        assert rec[2] == 0
    if n > 3:
        assert rec[3] == 0
    if n > 4:
        assert [a[0] for a in exp[4]["adopted"]] == [0, 7] and rec[4] == 2


def test_one_frame_path_stored_patches(scene):
    h = make_handle(1)
    try:
        gray = scene["frames"]["dmg"]
        for _ in range(3):   # eager, capture, replay of the single-frame graph
            m = h.detect(gray, K=KF, marker_size=rr.MARKER_SIZE)
        exp, out, n, rec, boards = check_batch(h, [gray], [m], scene)
        check_story(exp, rec, 1)
        # the graph stays valid: the next frame detects as before
        again = h.detect(gray, K=KF, marker_size=rr.MARKER_SIZE)
        assert again.tobytes() == m.tobytes()
    finally:
        h.close()


@pytest.mark.parametrize("n", [2, 3, 5])
def test_batch_sizes(scene, n):
    h = make_handle(n)
    try:
        frames = frames_of(scene, n)
        markers = h.detect_batch_host(np.stack(frames), K=KF, marker_size=rr.MARKER_SIZE)
        assert [len(m) for m in markers] == [9, 10, 1, 12, 10][:n]
        exp, out, n_out, rec, boards = check_batch(h, frames, markers, scene, cells=n >= 3)
        check_story(exp, rec, n)
    finally:
        h.close()


def test_two_spans(scene, monkeypatch):
    monkeypatch.setenv("ARUCOHIP_STREAMS", "2")
    h = make_handle(4)
    monkeypatch.delenv("ARUCOHIP_STREAMS")
    try:
        frames = [scene["frames"][k] for k in ("clean", "dmg", "blot", "dmg2")]
        markers = h.detect_batch_host(np.stack(frames), K=KF, marker_size=rr.MARKER_SIZE)
        assert h.batch_chunks() == (2, 2)
        exp, out, n, rec, boards = check_batch(h, frames, markers, scene)
        assert list(rec) == [0, 2, 1, 2]
    finally:
        h.close()


def test_ticket_of_a_pipeline(scene):
    from aruco_amd import capi

    h = make_handle(3)
    try:
        h.set_pipeline_depth(2)
        frames = np.stack(frames_of(scene, 3))
        out = np.zeros((3, 64), capi.MARKER_DTYPE)
        n = np.zeros(3, np.int32)
        other = np.stack([scene["frames"]["clean"]] * 3)
        out2, n2 = out.copy(), n.copy()
        t = h.submit_host(frames, out, n, K=KF, marker_size=rr.MARKER_SIZE)
        t2 = h.submit_host(other, out2, n2, K=KF, marker_size=rr.MARKER_SIZE)
        h.wait(t2)
        h.wait(t)   # the last batch is the first ticket's
        markers = [out[f, :n[f]].copy() for f in range(3)]
        exp, _, _, rec, _ = check_batch(h, list(frames), markers, scene, cells=True)
        check_story(exp, rec, 3)
    finally:
        h.close()


def test_six_errors_need_limit_six(scene):
    h = make_handle(3)
    try:
        frames = [scene["frames"]["dmg"]] * 3
        markers = h.detect_batch_host(np.stack(frames), K=KF, marker_size=rr.MARKER_SIZE)
        exp, out, n, rec, boards = check_batch(h, frames, markers, scene, opt={"max_cell_errors": 6}, painted=(6,), cells=True)
        assert [a[0] for a in exp[0]["adopted"]] == [1, 6, 10] and list(rec) == [3, 3, 3]
        assert [c[4] for c in exp[0]["considered"] if c[4] is not None] == [1, 2, 6]
    finally:
        h.close()


@pytest.mark.parametrize("turns", [1, 2, 3])
def test_in_plane_rotation(scene, turns):
    """Boards turned near 90, 180 and 270 degrees: corner i of every recovered marker lies within max_corner_dist of projected corner i."""
    ids = scene["ids"]
    obj = rr.turned(scene["obj"], turns)
    rvec = np.array([0.12, -0.1, 0.03])
    gray, _ = rr.build_frame(ids, obj, {2: [(2, 3)], 9: [(4, 2), (1, 5)]}, rvec=rvec, seed=20 + turns)
    h = make_handle(1)
    try:
        m = h.detect(gray, K=KF, marker_size=rr.MARKER_SIZE)
        s2 = dict(scene, obj=obj)
        exp, out, n, rec, boards = check_batch(h, [gray], [m], s2)
        assert rec[0] == 2 and [a[0] for a in exp[0]["adopted"]] == [2, 9]
        for j in (2, 9):
            got = [x for x in out[0] if int(x["id"]) == ids[j]][0]
            proj = rr.project(rr.K, rvec, rr.TVEC, obj[j] * rr.UNIT)
            assert np.max(np.linalg.norm(np.array(got["corners"]).reshape(4, 2) - proj, axis=1)) < 10.0
    finally:
        h.close()


def test_more_than_64_rejected_candidates(scene):
    ids, obj = scene["ids"], scene["obj"]
    _, quads = rr.build_frame(ids, obj)
    gray, _ = rr.build_frame(ids, obj, {1: [(3, 3)]}, squares=rr.background_squares(quads))
    # the flat candidate list of a handle holds 96 entries per frame of its batch: the frame shares a batch with two plain ones
    frames = [scene["frames"]["clean"], gray, scene["frames"]["clean"]]
    h = make_handle(3)
    try:
        markers = h.detect_batch_host(np.stack(frames), K=KF, marker_size=rr.MARKER_SIZE)
        exp = expect(h, frames, markers, ids, obj, cells=True)
        assert len(exp[1]["adopted"]) == 1 and exp[1]["adopted"][0][1] >= 64 and len(exp[1]["before"][1]) > 128
        _, _, _, rec, _ = check_batch(h, frames, markers, scene, cells=True)
        assert list(rec) == [0, 1, 0]
    finally:
        h.close()


def test_a_frame_the_batch_gave_up_stays_given_up(scene):
    """A handle of 96 candidates a frame (a one-frame handle's flat list held no more, whatever its limits said, until a single frame could fill
    its own candidate list): the frame with the squares, more than 128 candidates, overflows it and comes back with n = -1."""
    from aruco_amd import capi

    ids, obj = scene["ids"], scene["obj"]
    _, quads = rr.build_frame(ids, obj)
    gray, _ = rr.build_frame(ids, obj, {1: [(3, 3)]}, squares=rr.background_squares(quads))
    lim = capi.Limits()
    capi.load().arucohip_default_limits(C.byref(lim), rr.W, rr.H, 1)
    lim.candidates_per_frame = 96
    h = make_handle(1, limits=lim)
    try:
        markers, _, first = h.detect_batch_host_tolerant(gray[None], K=KF, marker_size=rr.MARKER_SIZE, retry=False)
        assert markers[0] is None and first[0] == -1
        before = [a.tobytes() for a in h.debug_candidates(0)]
        out, n, rec, boards = h.board_recover_batch(1, ids, obj, rr.PIX, KF, marker_size=rr.MARKER_SIZE)
        assert n[0] == -1 and rec[0] == 0 and len(out[0]) == 0 and boards[0]["n_markers"] == 0 and boards[0]["has_pose"] == 0
        assert [a.tobytes() for a in h.debug_candidates(0)] == before
    finally:
        h.close()


def oracle_lines(gray, quad0, nrot, K=None, dist=None):
    """orc.refine_lines on the oracle's own candidate with this integer quad, turned to canonical order."""
    from oracle import orc

    o = orc.Oracle()
    o.detect(gray)
    match = [c for c in o.candidates(with_contour=True) if np.array_equal(np.asarray(c["quad0"], np.float32), np.asarray(quad0, np.float32))]
    assert len(match) == 1
    c = orc.refine_lines(match[0]["contour"], match[0]["quad0"], K, dist)
    return np.array([c[(i + 4 - nrot) % 4] for i in range(4)], np.float32)


@pytest.mark.parametrize("dist", [None, DIST], ids=["no_dist", "dist"])
def test_lines_corners_against_the_oracle(scene, dist):
    ids, obj = scene["ids"], scene["obj"]
    gray = scene["frames"]["dmg"]
    h = make_handle(1)
    try:
        m = h.detect(gray, K=KF, dist=dist, marker_size=rr.MARKER_SIZE)
        exp = expect(h, [gray], [m], ids, obj, dist=dist)
        out, n, rec, _ = h.board_recover_batch(1, ids, obj, rr.PIX, KF, dist=dist, marker_size=rr.MARKER_SIZE)
        assert rec[0] == 2 and decisions(h, 0, exp[0]["before"], ids) == exp[0]["adopted"]
        for j, ci, rot in exp[0]["adopted"]:
            got = np.array([x for x in out[0] if int(x["id"]) == ids[j]][0]["corners"], np.float32).reshape(4, 2)
            ref = oracle_lines(gray, exp[0]["before"][0][ci], rot, KF if dist is not None else None, dist)
            err = np.max(np.abs(got - ref) / np.maximum(np.abs(ref), 1.0))
            print("LINES corner deviation", j, err)
            assert err < CORNER_REL_TOL
    finally:
        h.close()


def test_none_corners_are_the_rotated_integer_quad(scene):
    from aruco_amd import capi

    ids = scene["ids"]
    obj = rr.turned(scene["obj"], 1)
    gray, _ = rr.build_frame(ids, obj, {2: [(2, 3)]}, seed=21)
    p = capi.default_params()
    p.corner_method = capi.CORNER_NONE
    h = make_handle(1, params=p)
    try:
        m = h.detect(gray, K=KF, marker_size=rr.MARKER_SIZE)
        exp, out, n, rec, _ = check_batch(h, [gray], [m], dict(scene, obj=obj))
        (j, ci, rot), = exp[0]["adopted"]
        q = exp[0]["before"][0][ci]
        got = np.array([x for x in out[0] if int(x["id"]) == ids[j]][0]["corners"], np.float32).reshape(4, 2)
        assert got.tobytes() == np.array([q[(i + 4 - rot) % 4] for i in range(4)], np.float32).tobytes()
    finally:
        h.close()


def test_board_pose_equals_board_detect_on_the_returned_markers(scene):
    ids, obj = scene["ids"], scene["obj"]
    h = make_handle(3)
    try:
        frames = frames_of(scene, 3)
        h.detect_batch_host(np.stack(frames), K=KF, marker_size=rr.MARKER_SIZE)
        worst = 0.0
        for y_perp in (False, True):
            out, n, rec, boards = h.board_recover_batch(3, ids, obj, rr.PIX, KF, marker_size=rr.MARKER_SIZE, repj_err_thres=2.0, y_perp=y_perp)
            for f in range(3):
                ref = h.board_detect(out[f], ids, obj, rr.PIX, K=KF, marker_size=rr.MARKER_SIZE, repj_err_thres=2.0, y_perp=y_perp)
                rb = ref
                assert boards[f]["has_pose"] == rb["has_pose"] == 1 and abs(boards[f]["prob"] - rb["prob"]) == 0
                for k in ("rvec", "tvec"):
                    worst = max(worst, float(np.max(np.abs(boards[f][k] - rb[k])) / np.max(np.abs(rb[k]))))
        print("board pose deviation", worst)
        assert worst <= TOL
    finally:
        h.close()


def test_side_effects(scene):
    from aruco_amd import capi

    ids, obj = scene["ids"], scene["obj"]
    h = make_handle(3)
    try:
        frames = frames_of(scene, 3)
        markers = h.detect_batch_host(np.stack(frames), K=KF, marker_size=rr.MARKER_SIZE)
        rejected = [len(h.candidates(f)) for f in range(3)]
        before = h.board_detect_batch(3, ids, obj, rr.PIX, K=KF, marker_size=rr.MARKER_SIZE)
        out, n, rec, boards = h.board_recover_batch(3, ids, obj, rr.PIX, KF, marker_size=rr.MARKER_SIZE, opt=opt_of(pose_markers=1))
        assert list(rec) == [2, 1, 0]
        after = h.board_detect_batch(3, ids, obj, rr.PIX, K=KF, marker_size=rr.MARKER_SIZE)
        fresh = []
        for f in range(3):
            assert after[f]["n_markers"] == before[f]["n_markers"] + rec[f] == boards[f]["n_markers"]
            assert np.array_equal(after[f]["rvec"], boards[f]["rvec"]) and np.array_equal(after[f]["tvec"], boards[f]["tvec"])
            assert len(h.candidates(f)) == rejected[f] - rec[f]
            # the recovered markers carry their own pose, the others are as detection left them
            old = {int(m["id"]): m for m in markers[f]}
            new = [m for m in out[f] if int(m["id"]) not in old]
            assert len(new) == rec[f] and all(m.tobytes() == old[int(m["id"])].tobytes() for m in out[f] if int(m["id"]) in old)
            fresh.append(new)
        # the planar poses and GL matrices see the grown lists
        assert [len(x) for x in h.gl_modelview_batch(3)] == [int(v) for v in n]
        # a second call recovers nothing and changes nothing
        out2, n2, rec2, boards2 = h.board_recover_batch(3, ids, obj, rr.PIX, KF, marker_size=rr.MARKER_SIZE, opt=opt_of(pose_markers=1))
        assert list(rec2) == [0, 0, 0] and all(out2[f].tobytes() == out[f].tobytes() for f in range(3))
        assert list(n2) == list(n)
        # pose_markers: what arucohip_calculate_extrinsics gives on the same corners (it stages through the marker list: last)
        for new in fresh:
            if new:
                bare = np.array(new)
                bare["ssize"], bare["has_pose"], bare["rvec"], bare["tvec"] = -1, 0, 0, 0
                posed = h.calculate_extrinsics(bare, KF, None, rr.MARKER_SIZE)
                assert posed.tobytes() == np.array(new).tobytes() and np.all(posed["has_pose"] == 1)
    finally:
        h.close()


def test_device_output_equals_host_output(scene):
    import torch
    from aruco_amd import capi

    ids, obj = scene["ids"], scene["obj"]
    h = make_handle(3)
    try:
        frames = np.stack(frames_of(scene, 3))
        cap = 16
        h.detect_batch_host(frames, K=KF, marker_size=rr.MARKER_SIZE)
        d_out = torch.zeros(3 * cap * capi.MARKER_DTYPE.itemsize, dtype=torch.uint8, device="cuda")
        d_n = torch.zeros(3, dtype=torch.int32, device="cuda")
        torch.cuda.synchronize()
        h.board_recover_batch_device(3, ids, obj, rr.PIX, d_out.data_ptr(), cap, d_n.data_ptr(), KF, marker_size=rr.MARKER_SIZE)
        h.synchronize()
        dev = np.frombuffer(d_out.cpu().numpy().tobytes(), capi.MARKER_DTYPE).reshape(3, cap)
        dn = d_n.cpu().numpy()
        h.detect_batch_host(frames, K=KF, marker_size=rr.MARKER_SIZE)
        out, n, rec, _ = h.board_recover_batch(3, ids, obj, rr.PIX, KF, marker_size=rr.MARKER_SIZE, cap=cap)
        assert list(dn) == list(n) == [11, 11, 1]
        for f in range(3):
            assert dev[f, :n[f]].tobytes() == out[f].tobytes()
    finally:
        h.close()


def test_pyr_down_level_one(scene):
    ids, obj = scene["ids"], scene["obj"]
    gray = scene["frames"]["dmg2"]
    h = make_handle(1)
    try:
        h.set_pyr_down(1)
        m = h.detect(gray, K=KF, marker_size=rr.MARKER_SIZE)
        exp, out, n, rec, _ = check_batch(h, [gray], [m], scene)
        assert [a[0] for a in exp[0]["adopted"]] == [0, 7] and rec[0] == 2
    finally:
        h.close()


def test_full_marker_list_stops_the_frame(scene):
    from aruco_amd import capi

    ids, obj = scene["ids"], scene["obj"]
    lim = capi.Limits()
    capi.load().arucohip_default_limits(C.byref(lim), rr.W, rr.H, 1)
    lim.markers_per_frame = 10
    h = make_handle(1, limits=lim)
    try:
        gray = scene["frames"]["dmg"]
        m = h.detect(gray, K=KF, marker_size=rr.MARKER_SIZE)
        assert len(m) == 9
        out, n, rec, boards = h.board_recover_batch(1, ids, obj, rr.PIX, KF, marker_size=rr.MARKER_SIZE, allow=(capi.E_CAPACITY,))
        assert rec[0] == 1 and n[0] == 10 and boards[0]["n_markers"] == 10
        # and an output array that is too small reports the count it needs
        out, n, rec, boards = h.board_recover_batch(1, ids, obj, rr.PIX, KF, marker_size=rr.MARKER_SIZE, cap=4, allow=(capi.E_CAPACITY,))
        assert n[0] == 10 and len(out[0]) == 4
    finally:
        h.close()


def test_errors_leave_the_batch_untouched(scene):
    from aruco_amd import capi

    ids, obj = scene["ids"], scene["obj"]
    h = make_handle(1)
    try:
        gray = scene["frames"]["dmg"]
        m = h.detect(gray, K=KF, marker_size=rr.MARKER_SIZE)
        snap = [a.tobytes() for a in h.debug_candidates(0)]

        def code(ids=ids, obj=obj, K=KF, marker_size=rr.MARKER_SIZE, nframes=1, info=rr.PIX, **o):
            try:
                h.board_recover_batch(nframes, ids, obj, info, K, marker_size=marker_size, opt=opt_of(**o) if o else None)
            except capi.ArucoHipError as e:
                assert [a.tobytes() for a in h.debug_candidates(0)] == snap
                return e.code
            return capi.OK

        assert code(K=None) == capi.E_INVALID
        assert code(marker_size=-1.0) == capi.E_INVALID
        assert code(max_corner_dist=0.0) == capi.E_INVALID
        assert code(max_cell_errors=-1) == capi.E_INVALID and code(max_cell_errors=50) == capi.E_INVALID
        assert code(min_markers=0) == capi.E_INVALID
        assert code(nframes=2) == capi.E_INVALID
        assert code(ids=[], obj=np.zeros((0, 4, 3))) == capi.E_BOARD_CONFIG
        assert code(ids=list(range(683)), obj=np.zeros((683, 4, 3))) == capi.E_CAPACITY
        base = h.get_params()
        for field, value in (("corner_method", capi.CORNER_HARRIS), ("corner_method", capi.CORNER_SUBPIX), ("use_locked_corners", 1),
                             ("decoder_kind", 1), ("decoder_kind", 2)):
            p = h.get_params()
            setattr(p, field, value)
            h.set_params(p)
            assert code() == capi.E_UNSUPPORTED, field
            h.set_params(base)
        # and the call still works afterwards
        out, n, rec, _ = h.board_recover_batch(1, ids, obj, rr.PIX, KF, marker_size=rr.MARKER_SIZE)
        assert rec[0] == 2 and n[0] == len(m) + 2
    finally:
        h.close()
