"""The marker-list tail (aruco_amd/csrc/k_finalize.hip: finalize_kernel and the list-driven pose_kernel, fed by border_rect.h) held to
tests/tail_ref.py at its edges, through the test hook arucohip_debug_marker_tail. Every comparison is exact: ids, counts, status bits and
list entries as integers, corners bit for bit, untouched rows by their 0xA5 fill. test_tail_cpu.py pins the reference on the same cases
(hand-computed chains, near-tie pairs, the host-compiled rectangle, the oracle at the rectangle's bounds)."""
import contextlib
import ctypes as C

import numpy as np
import pytest

from tests import pose_ref
from tests import tail_ref as ref

pytestmark = pytest.mark.gpu

W, H = ref.W, ref.H
SENTINEL = bytes([ref.FILL])
K_SMALL = np.array([[500.0, 0.0, 320.0], [0.0, 500.0, 240.0], [0.0, 0.0, 1.0]])   # a 640 x 480 camera


def make_handle(max_w, max_h, max_batch, cands, markers, planes=3, params=None):
    from aruco_amd import capi

    lim = capi.Limits()
    capi.load().arucohip_default_limits(C.byref(lim), max_w, max_h, max_batch)
    lim.candidates_per_frame, lim.markers_per_frame, lim.max_thres_planes = cands, markers, planes
    return capi.Handle(max_w, max_h, max_batch=max_batch, limits=lim, params=params)


@pytest.fixture(scope="module")
def big():
    h = make_handle(W, H, 9, 512, 256)          # the largest lists a handle has
    yield h
    h.close()


@pytest.fixture(scope="module")
def small():
    h = make_handle(W, H, 4, 16, 4)             # capacities within reach
    yield h
    h.close()


@pytest.fixture(scope="module")
def aux():
    from aruco_amd import capi

    h = capi.Handle(W, H, max_batch=1)          # the single calls the batch consumers are compared with
    yield h
    h.close()


@contextlib.contextmanager
def params(h, **kw):
    old = h.get_params()
    p = h.get_params()
    for k, v in kw.items():
        setattr(p, k, v)
    h.set_params(p)
    try:
        yield
    finally:
        h.set_params(old)


EMPTY = (np.zeros(0, np.int32), np.zeros((0, 8), np.float32))


def flatten(frames):
    """the frames' candidates in one list, the frames interleaved: the order inside a frame is what counts"""
    ids, corners, frame_of = [], [], []
    for k in range(max([len(f[0]) for f in frames] + [0])):
        for f, (fi, fc) in enumerate(frames):
            if k < len(fi):
                ids.append(fi[k]), corners.append(fc[k]), frame_of.append(f)
    return np.array(ids, np.int32), np.array(corners, np.float32).reshape(-1, 8), np.array(frame_of, np.int32)


def expected_row(mid, corners):
    from aruco_amd import capi

    m = np.zeros(1, capi.MARKER_DTYPE)
    m["id"], m["corners"], m["ssize"] = mid, corners, -1.0
    return m.tobytes()


def run_and_check(h, frames, width=W, height=H, border_dist=0.025, plane_status=None, what=""):
    """the hook on `frames` against tail_ref.tail, without a camera: counts, status, rows, untouched rows, list, header"""
    capm = h.markers_per_frame()
    ids, corners, frame_of = flatten(frames)
    got = h.debug_marker_tail(len(frames), width, height, ids, corners, frame_of, plane_status=plane_status)
    exp = ref.tail(frames, width, height, capm, border_dist=border_dist, plane_status=plane_status)
    assert got["n"].tolist() == exp["n"], what
    assert got["status"] == exp["status"], what
    for f, (fi, fc) in enumerate(frames):
        if exp["rows"][f] is None:
            continue
        rows = got["rows"][f]
        want = exp["rows"][f]
        assert rows["id"][:len(want)].tolist() == [int(fi[i]) for i in want], "%s frame %d" % (what, f)
        for k, i in enumerate(want):
            assert rows[k].tobytes() == expected_row(fi[i], fc[i]), "%s frame %d row %d" % (what, f, k)
        assert rows[len(want):].tobytes() == SENTINEL * (rows.itemsize * (capm - len(want))), "%s frame %d: rows behind the markers" % (what, f)
    assert got["nmark"] == len(exp["list"]) == len(got["list"]), what
    assert set(got["list"].tolist()) == exp["list"], what                       # a permutation of the kept slots
    assert got["raw_list"][got["nmark"]:].tobytes() == SENTINEL * (4 * (len(got["raw_list"]) - got["nmark"])), what
    if len(frames) == 1:
        assert tuple(got["hdr"].tolist()) == exp["hdr"], what
    else:
        assert got["hdr"].tobytes() == SENTINEL * 8, what                        # only a one-frame call writes it
    return got, exp


# ---- a. order ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("distinct", [False, True], ids=["repeats", "distinct"])
def test_order_by_id_then_candidate_order(big, distinct):
    """1, 63, 64, 65, 130 and candidates_per_frame candidates in a frame, -1 entries between them, ids 0, 1, 1023 and 2^31 - 1 among them:
    with many repeats (the rank decides which neighbours the dedupe compares) and with distinct ids (every candidate comes out, 512 of them
    into 256 rows)."""
    counts = (1, 63, 64, 65, 130, 512)
    frames = [ref.order_frame(n, (200 if not distinct else 100) + n, distinct=distinct) for n in counts]
    got, exp = run_and_check(big, frames, what="six frames")
    if distinct:
        assert exp["n"][-1] > 256 and got["status"] == ref.ST_MARKER_OVERFLOW
    for f in (0, 3, 5):                                                          # and alone: the one-frame header, frame 0's lanes
        run_and_check(big, [frames[f]], what="frame %d alone" % f)


# ---- b. dedupe --------------------------------------------------------------------------------------------------------------------------
def test_dedupe_chains_and_near_ties(big):
    """The hand-computed chains, every order of a run of four, and the near-tie pairs that a perimeter summed in double decides differently"""
    chain = ref.chain_frame()
    perms = ref.permutation_chains()
    perm_frame = (np.repeat(np.arange(len(perms), dtype=np.int32) * 3 + 5, 4), np.concatenate([c for _, c in perms]))
    pid, pc, disagree = ref.near_tie_pairs()
    got, exp = run_and_check(big, [(chain[0], chain[1]), perm_frame, (pid, pc)], what="chains")
    # what the reference side says of them is what test_tail_cpu.py worked out by hand
    for name, (per, want) in ref.CHAINS.items():
        run = chain[2][name]
        assert [run.index(i) for i in exp["kept"][0] if i in run] == want, name
    ids0 = got["rows"][0]["id"][:got["n"][0]].tolist()
    assert ids0.count(100 + 7 * sorted(ref.CHAINS).index("triple_10_5_7")) == 2   # two markers of one id
    assert 100 + 7 * sorted(ref.CHAINS).index("winner_outside") not in ids0
    assert got["n"][2] == len(pid) // 2 and len(disagree) * 4 >= len(pid) // 2


# ---- c. border --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("size", [s for s in ref.RECT_TABLE_SIZES if s != (1, 1)], ids=lambda s: "%dx%d" % s)
def test_border_filter_at_the_rectangle(big, size):
    """Corners on b - 0.5 (ties to even), an ulp to either side, b + 0.5, whole pixels, -0.5 and -0.49, at every bound of the rectangle
    in x and y, for the sizes whose rectangle comes from a half-way product and some that do not"""
    ids, corners = ref.border_frame(*size)
    got, exp = run_and_check(big, [(ids, corners)], width=size[0], height=size[1], what="%d x %d" % size)
    assert 0 < exp["n"][0] < len(ids)


@pytest.mark.parametrize("t", [0.0, 0.0125, 0.5, 0.6])
def test_border_distance_zero_half_and_beyond(big, t):
    """t = 0: the whole frame (-0.5 rounds to 0 and is inside); t = 0.5: an empty rectangle drops everything; t = 0.6: the sorted rectangle"""
    with params(big, border_dist=t):
        for size in ((640, 480), (100, 60)):
            ids, corners = ref.border_frame(size[0], size[1], t)
            got, exp = run_and_check(big, [(ids, corners)], width=size[0], height=size[1], border_dist=t, what="t %g, %d x %d" % (t, size[0], size[1]))
            assert (exp["n"][0] == 0) == (t == 0.5)
    one = (np.array([3], np.int32), np.array([[0, 0, 0, 0, 0, 0, 0, 0]], np.float32))
    with params(big, border_dist=0.0):
        run_and_check(big, [one], width=1, height=1, border_dist=0.0, what="1 x 1")   # [0, 1) x [0, 1) holds the pixel (0, 0)


def test_oracle_leg_frames_through_detect():
    """The frames of test_tail_cpu's oracle leg (one marker, corner method NONE, its extreme corner on b0 - 1, b0, b1 - 1, b1) through the
    whole detection: the oracle's id lists"""
    from aruco_amd import capi
    from tests.test_tail_cpu import ORACLE_SIZES, oracle_leg_cases

    p = capi.default_params()
    p.corner_method = capi.CORNER_NONE
    h = capi.Handle(max(s[0] for s in ORACLE_SIZES), max(s[1] for s in ORACLE_SIZES), max_batch=1, params=p)
    try:
        for size in ORACLE_SIZES:
            cases = oracle_leg_cases(*size)
            assert cases is not None
            for name, frame, corners, ids in cases:
                ms = h.detect(frame)
                assert [int(m["id"]) for m in ms] == ids, "%d x %d, %s" % (size[0], size[1], name)
                if ids:
                    assert np.array_equal(np.asarray(ms[0]["corners"]).reshape(4, 2), corners), name
    finally:
        h.close()


# ---- d. capacity ------------------------------------------------------------------------------------------------------------------------
def kept_frame(n, seed, extra_rejected=2):
    """n candidates that are all kept (distinct ids, inside), and some that are not"""
    rng = np.random.RandomState(seed)
    ids = np.concatenate([rng.permutation(n) + 10, np.full(extra_rejected, -1)]).astype(np.int32)
    return ids, ref.random_quads(rng, len(ids))


def test_marker_rows_hold_cap_markers(small):
    """kept = cap - 1, cap, cap + 1: the true count, the overflow bit only above cap, the first cap markers in order, 0xA5 behind them"""
    cap = small.markers_per_frame()
    assert cap == 4
    for kept in (cap - 1, cap, cap + 1):
        got, exp = run_and_check(small, [kept_frame(kept, 30 + kept)], what="kept %d" % kept)
        assert got["n"].tolist() == [kept] and got["status"] == (ref.ST_MARKER_OVERFLOW if kept > cap else 0)
        assert got["nmark"] == min(kept, cap)
    got, exp = run_and_check(small, [kept_frame(k, 40 + k) for k in (cap + 1, cap - 1, cap)], what="batch of three")
    assert got["n"].tolist() == [cap + 1, cap - 1, cap] and got["status"] == ref.ST_MARKER_OVERFLOW and got["nmark"] == 3 * cap - 1


@pytest.mark.parametrize("out_cap", [2, 4, 6])
def test_write_through_rows(small, out_cap):
    """The caller's device array with out_cap below, equal to and above markers_per_frame: min(n, out_cap, cap) rows per frame, the
    caller's bytes behind them, the true counts"""
    import torch
    from aruco_amd import capi

    cap, isz = small.markers_per_frame(), capi.MARKER_DTYPE.itemsize
    frames = [kept_frame(cap + 1, 51), kept_frame(cap - 1, 52), EMPTY, kept_frame(cap, 53)]
    ids, corners, frame_of = flatten(frames)
    out = torch.full((len(frames) * out_cap * isz,), 0x5A, dtype=torch.uint8, device="cuda")
    n_out = torch.full((len(frames),), -77, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    got = small.debug_marker_tail(len(frames), W, H, ids, corners, frame_of, out_dev=out.data_ptr(), out_cap=out_cap, n_out_dev=n_out.data_ptr())
    exp = ref.tail(frames, W, H, cap, out_cap=out_cap)
    assert n_out.cpu().tolist() == exp["n"] == got["n"].tolist() == [cap + 1, cap - 1, 0, cap]
    rows = np.frombuffer(out.cpu().numpy().tobytes(), capi.MARKER_DTYPE).reshape(len(frames), out_cap)
    for f, (fi, fc) in enumerate(frames):
        want = exp["out_rows"][f]
        assert len(want) == min(exp["n"][f], out_cap, cap)
        for k, i in enumerate(want):
            assert rows[f, k].tobytes() == expected_row(fi[i], fc[i]) == got["rows"][f, k].tobytes(), (f, k)
        assert rows[f, len(want):].tobytes() == bytes([0x5A]) * (isz * (out_cap - len(want))), f


# ---- e. frames given up -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("plane", [0, 1, 2])
def test_a_status_bit_on_any_plane_gives_the_frame_up(small, plane):
    """Three threshold planes, a status bit on one plane of frame 1 of 3 (the last plane included): n = -1 for that frame alone, no list
    entries for it, its neighbours as without the bit"""
    with params(small, thres_param1_range=1):
        frames = [kept_frame(3, 61), kept_frame(4, 62), kept_frame(2, 63)]
        status = np.zeros((3, 3), np.uint32)
        status[1, plane] = 4
        got, exp = run_and_check(small, frames, plane_status=status, what="plane %d" % plane)
        assert got["n"].tolist() == [3, -1, 2] and got["status"] == 4
        assert sorted(got["list"].tolist()) == [0, 1, 2, (2 << 16), (2 << 16) | 1]
        clean, _ = run_and_check(small, frames, plane_status=np.zeros((3, 3), np.uint32), what="no bit")
        assert clean["n"].tolist() == [3, 4, 2]
        for f in (0, 2):
            assert got["rows"][f].tobytes() == clean["rows"][f].tobytes()


def test_one_frame_header(small):
    """One frame per call: the two words behind the rows are the count and the status bits, this kernel's overflow bit included"""
    with params(small, thres_param1_range=1):
        for kept, status, want in ((3, None, (3, 0)), (5, None, (5, 32)), (3, [[0, 2, 0]], (-1, 2)), (5, [[0, 0, 8]], (-1, 8 | 32)), (0, None, (0, 0))):
            got, exp = run_and_check(small, [kept_frame(kept, 70 + kept)], plane_status=status, what="kept %d status %s" % (kept, status))
            assert tuple(got["hdr"].tolist()) == want == (int(got["n"][0]), got["status"])


# ---- f. batch ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nframes", [1, 2, 9])
def test_batches_of_empty_rejected_and_full_frames(big, nframes):
    """1, 2 and max_batch frames: empty frames, frames whose candidates are all undecoded or all outside, full candidate lists; the flat
    list is a permutation of the kept slots and CNT_NMARK their number (both inside run_and_check)"""
    rng = np.random.RandomState(80 + nframes)
    outside = (np.arange(5, dtype=np.int32), np.array([ref.square(2.0, 100.0 + 30 * k, 20.0) for k in range(5)], np.float32))
    undecoded = (np.full(7, -1, np.int32), ref.random_quads(rng, 7))
    pool = [ref.order_frame(512, 81, distinct=True), EMPTY, outside, ref.order_frame(512, 82), undecoded, ref.order_frame(65, 83),
            EMPTY, ref.order_frame(512, 84, distinct=True), ref.order_frame(1, 85)]
    frames = pool[:nframes] if nframes > 1 else [pool[3]]
    got, exp = run_and_check(big, frames, what="%d frames" % nframes)
    if nframes == 9:
        assert got["n"].tolist()[1] == got["n"].tolist()[2] == got["n"].tolist()[4] == got["n"].tolist()[6] == 0
        assert got["n"][0] > 256 and got["n"][7] > 256
    # an empty batch: nothing at all
    got, exp = run_and_check(big, [EMPTY] * nframes, what="%d empty frames" % nframes)
    assert got["nmark"] == 0 and got["n"].tolist() == [0] * nframes


# ---- g. pose on the list ----------------------------------------------------------------------------------------------------------------
def posed_markers(total, seed):
    """`total` markers of 0.05 m seen by K_SMALL, all inside the border rectangle of 640 x 480: ids distinct, corners [total][8]"""
    from tests.planar_ref import brown_project, object_points

    rng = np.random.default_rng(seed)
    rect = ref.border_rect(W, H)
    P = object_points(pose_ref.MARKER_SIZE)
    out = []
    while len(out) < total:
        R = pose_ref.facing_rotation(rng, rng.uniform(0.1, 1.0))
        t = pose_ref.translation(rng, (0.4, 1.5))
        c = brown_project(P, R, t, K_SMALL, None).astype(np.float32).reshape(8)
        if ref.inside(c, rect):
            out.append(c)
    return rng.permutation(total).astype(np.int32) + 1, np.array(out, np.float32)


@pytest.mark.parametrize("y_perp", [False, True], ids=["plain", "y_perp"])
@pytest.mark.parametrize("total", [15, 16, 17, 33])
def test_poses_of_the_listed_markers(big, aux, total, y_perp):
    """15, 16, 17 and 33 kept markers over three frames (the pose kernel takes 16 to a workgroup, from the flat list): every kept slot has
    the pose arucohip_calculate_extrinsics gives the same corners, to the bit (the same device function on the same inputs), the rows
    behind them stay untouched"""
    ids, corners = posed_markers(total, 90 + total)
    cut = (total // 3, total // 3 + total // 2)
    frames = [(ids[:cut[0]], corners[:cut[0]]), (ids[cut[0]:cut[1]], corners[cut[0]:cut[1]]), (ids[cut[1]:], corners[cut[1]:])]
    fi, fc, fo = flatten(frames)
    K32 = K_SMALL.astype(np.float32)
    got = big.debug_marker_tail(3, W, H, fi, fc, fo, K=K32, marker_size=pose_ref.MARKER_SIZE, y_perp=y_perp)
    exp = ref.tail(frames, W, H, big.markers_per_frame())
    assert got["n"].tolist() == exp["n"] == [len(f[0]) for f in frames] and got["nmark"] == total
    bare = big.debug_marker_tail(3, W, H, fi, fc, fo)                        # no camera: ssize -1, no pose, zero vectors
    for f in range(3):
        n = exp["n"][f]
        want = aux.calculate_extrinsics(bare["rows"][f, :n], K32, None, pose_ref.MARKER_SIZE, y_perp=y_perp)
        assert np.all(bare["rows"][f, :n]["ssize"] == -1) and not bare["rows"][f, :n]["has_pose"].any() and not bare["rows"][f, :n]["rvec"].any()
        assert np.all(want["has_pose"] == 1)
        assert got["rows"][f, :n].tobytes() == want.tobytes(), "frame %d" % f
        assert got["rows"][f, n:].tobytes() == SENTINEL * (got["rows"].itemsize * (got["rows"].shape[1] - n))
    # a camera without a marker size poses nothing (detect_core's condition)
    nosize = big.debug_marker_tail(3, W, H, fi, fc, fo, K=K32)
    assert nosize["rows"].tobytes() == bare["rows"].tobytes()


# ---- h. the batch consumers on edge lists -----------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def edge_batch(small):
    """four frames on the handle of four rows: given up (n = -1), empty, six board markers (n > cap), three board markers and a stranger"""
    v = pose_ref.board_view(6, "mild", 0.0, K_SMALL, seed=4242)
    corners = v["corners"].reshape(6, 8)
    rect = ref.border_rect(W, H)
    assert all(ref.inside(c, rect) for c in corners)
    stranger = posed_markers(1, 7)
    frames = [(v["ids"][:3], corners[:3]), EMPTY, (v["ids"], corners),
              (np.concatenate([v["ids"][[0, 2, 5]], [7]]).astype(np.int32), np.concatenate([corners[[0, 2, 5]], stranger[1]]))]
    return v, frames


def run_edge_batch(small, v, frames, which):
    frames = [frames[f] for f in which]
    status = np.array([[4 if f == 0 else 0] for f in which], np.uint32)
    fi, fc, fo = flatten(frames)
    got = small.debug_marker_tail(len(frames), W, H, fi, fc, fo, plane_status=status, K=K_SMALL.astype(np.float32), marker_size=pose_ref.MARKER_SIZE)
    exp = ref.tail(frames, W, H, small.markers_per_frame(), plane_status=status)
    assert got["n"].tolist() == exp["n"]
    return got, exp


def test_gl_modelview_batch_on_edge_lists(small, edge_batch):
    from aruco_amd import capi

    v, frames = edge_batch
    got, exp = run_edge_batch(small, v, frames, (0, 1, 2, 3))
    assert exp["n"] == [-1, 0, 6, 4]
    cap, capm = 6, small.markers_per_frame()
    mv = np.full((4, cap, 16), np.nan)
    n = np.zeros(4, np.int32)
    small._chk(small.L.arucohip_gl_modelview_batch(small.h, 4, cap, mv.ctypes.data_as(C.c_void_p), n.ctypes.data_as(C.c_void_p)))
    assert n.tolist() == [-1, 0, capm, 4]
    for f in range(4):
        live = max(min(exp["n"][f], capm), 0)
        assert not mv[f, live:].any(), f                                      # zero matrices for given-up frames and for slots >= n
        for i in range(live):
            m = got["rows"][f, i]
            assert m["has_pose"] == 1
            assert np.max(np.abs(mv[f, i] - capi.gl_modelview(m["rvec"], m["tvec"]))) < 1e-12, (f, i)   # device sin / cos vs libm
    lists = small.gl_modelview_batch(4, cap=cap)
    assert [len(x) for x in lists] == [0, 0, capm, 4]
    assert all(np.array_equal(lists[f], mv[f, :len(lists[f])]) for f in range(4))


def board_batch_raw(h, nframes, ids, obj, K, marker_size):
    from aruco_amd import capi

    ida, oa, Ka = np.ascontiguousarray(ids, np.int32), np.ascontiguousarray(obj, np.float32), np.ascontiguousarray(K, np.float32)
    out = (capi.BoardOut * nframes)()
    prob = np.full(nframes, np.nan, np.float32)
    rc = h.L.arucohip_board_detect_batch(h.h, nframes, ida.ctypes.data_as(C.c_void_p), oa.ctypes.data_as(C.c_void_p), len(ida), capi.BOARD_METERS,
                                         Ka.ctypes.data_as(C.c_void_p), None, 0, float(marker_size), -1.0, 0, out, prob.ctypes.data_as(C.c_void_p))
    return rc, [{"n_markers": out[f].n_markers, "has_pose": out[f].has_pose, "rvec": np.array(out[f].rvec), "tvec": np.array(out[f].tvec),
                 "prob": float(prob[f])} for f in range(nframes)]


def test_board_detect_batch_on_edge_lists(small, aux, edge_batch):
    """Frames given up and empty frames report no markers and no pose; a live frame is answered as arucohip_board_detect answers the
    markers of its rows. A frame that kept more than markers_per_frame markers has set the batch's marker-overflow bit, which
    arucohip_board_detect_batch reports as ARUCOHIP_E_CAPACITY; what it wrote before is still the board of the rows that exist."""
    from aruco_amd import capi

    v, frames = edge_batch
    K32 = K_SMALL.astype(np.float32)
    for which, want_rc in (((0, 1, 3), capi.OK), ((0, 1, 2, 3), capi.E_CAPACITY)):
        got, exp = run_edge_batch(small, v, frames, which)
        rc, boards = board_batch_raw(small, len(which), v["ids"], v["obj"], K32, pose_ref.MARKER_SIZE)
        assert rc == want_rc, which
        for k, f in enumerate(which):
            live = max(min(exp["n"][k], small.markers_per_frame()), 0)
            if live == 0:
                assert boards[k]["n_markers"] == 0 and boards[k]["has_pose"] == 0 and boards[k]["prob"] == 0, f
                assert not boards[k]["rvec"].any() and not boards[k]["tvec"].any()
                continue
            one = aux.board_detect(got["rows"][k, :live], v["ids"], v["obj"], capi.BOARD_METERS, K=K32, marker_size=pose_ref.MARKER_SIZE)
            assert boards[k]["n_markers"] == len(one["markers"]) == (3 if f == 3 else 4), f
            assert boards[k]["has_pose"] == one["has_pose"] == 1
            assert abs(boards[k]["prob"] - one["prob"]) < 1e-7
            assert max(pose_ref.pose_dev(boards[k]["rvec"], boards[k]["tvec"], one["rvec"], one["tvec"])) < pose_ref.POSE_TOL, f


def test_planar_poses_batch_on_edge_lists(small, aux, edge_batch):
    from aruco_amd import capi

    v, frames = edge_batch
    got, exp = run_edge_batch(small, v, frames, (0, 1, 2, 3))
    capm = small.markers_per_frame()
    K32 = K_SMALL.astype(np.float32)
    out = np.frombuffer(small.planar_poses_batch(4, K32, None, pose_ref.MARKER_SIZE, cap=capm, fill=ref.FILL), capi.PLANAR_DTYPE).reshape(4, capm)
    for f in range(4):
        live = max(min(exp["n"][f], capm), 0)
        single = np.frombuffer(aux.planar_poses(got["rows"][f, :live], K32, None, pose_ref.MARKER_SIZE), capi.PLANAR_DTYPE)
        assert out[f, :live].tobytes() == single.tobytes(), f
        assert np.all(out[f, :live]["n_solutions"] == 2)
        assert out[f, live:].tobytes() == SENTINEL * (out.itemsize * (capm - live)), f     # entries for kept slots only


# ---- the hook's refusals ----------------------------------------------------------------------------------------------------------------
def test_hook_refuses_before_anything_runs(small):
    from aruco_amd import capi

    ok = kept_frame(3, 99)
    for bad in (np.nan, np.inf, 65535.0, -65535.0):
        c = ok[1].copy()
        c[1, 3] = bad
        with pytest.raises(capi.ArucoHipError) as e:
            small.debug_marker_tail(1, W, H, ok[0], c)
        assert e.value.code == capi.E_INVALID
    with pytest.raises(capi.ArucoHipError) as e:                                 # 17 candidates in a frame of 16
        small.debug_marker_tail(1, W, H, np.arange(17), ref.random_quads(np.random.RandomState(1), 17))
    assert e.value.code == capi.E_CAPACITY
    with pytest.raises(capi.ArucoHipError) as e:                                 # five frames on a handle of four
        small.debug_marker_tail(5, W, H, ok[0], ok[1])
    assert e.value.code == capi.E_INVALID
    with pytest.raises(capi.ArucoHipError) as e:
        small.debug_marker_tail(2, W, H, ok[0], ok[1], frame_of=[0, 1, 2, 0, 0])
    assert e.value.code == capi.E_INVALID
    got = small.debug_marker_tail(1, W, H, ok[0], ok[1])                         # and works afterwards
    assert got["n"].tolist() == [3]
