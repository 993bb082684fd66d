"""Overlay pass on the device against tests/overlay_ref.py: bytes, no tolerance. Inputs are chosen so that every projected coordinate the
restatement keeps lies at least 1e-3 from a half-integer (asserted here, on the CPU side): a last-ulp difference between the two
projections then cannot flip a rounding."""
import numpy as np
import pytest

from tests import overlay_ref as ovr

pytestmark = pytest.mark.gpu

ALL = ovr.OUTLINE | ovr.IDS | ovr.AXIS | ovr.CUBE
PAD = 5
DIST = [0.08, -0.12, 0.0011, -0.0017, 0.03]


def small_K(width, height):
    return np.array([[85.5, 0, width / 2 + 0.25], [0, 84.25, height / 2 - 0.5], [0, 0, 1]], np.float32)


def make_buffer(n, width, height, channels, seed=3):
    """[N][H][row_stride] with row_stride = width * channels + 5: a fixed texture in the image, 0xA5 in the padding."""
    rng = np.random.RandomState(seed)
    buf = np.full((n, height, width * channels + PAD), 0xA5, np.uint8)
    buf[:, :, :width * channels] = rng.randint(0, 200, (n, height, width * channels))
    return buf


def marker(mid, corners, ssize=0.05, rvec=None, tvec=None):
    from aruco_amd import capi

    m = np.zeros((), capi.MARKER_DTYPE)
    m["id"], m["corners"], m["ssize"] = mid, np.asarray(corners, np.float32).reshape(8), ssize
    if rvec is not None:
        m["has_pose"], m["rvec"], m["tvec"] = 1, rvec, tvec
    return m


def quad(cx, cy, side, angle):
    """A square of `side` pixels around (cx, cy), turned by `angle`, with corners off the pixel grid."""
    c, s = np.cos(angle), np.sin(angle)
    h = side / 2.0
    pts = np.array([[-h, -h], [h, -h], [h, h], [-h, h]])
    return pts @ np.array([[c, s], [-s, c]]) + [cx + 0.3, cy - 0.2]


def settle(build, K, dist, flags):
    """build(j) -> markers [N][cap], counts for try j: the first try whose kept projected coordinates all lie >= 1e-3 from a half-integer.
    The inputs are chosen, never the case dropped."""
    for j in range(64):
        markers, counts = build(j)
        pr = ovr.Prims()
        for f in range(markers.shape[0]):
            for i in range(min(max(int(counts[f]), 0), markers.shape[1])):
                ovr.marker_prims(pr, markers[f, i], K, dist, flags, 1, ovr.RED)
        if ovr.half_integer_margin(pr.coords) >= 1e-3:
            return markers, counts
    raise AssertionError("no input with every projected coordinate 1e-3 from a half-integer")


def device_draw(h, buf, width, channels, markers, counts, **kw):
    """draw_markers on device copies of everything; returns the frames as numpy."""
    import torch

    t = torch.from_numpy(buf.copy()).cuda()
    mt = torch.from_numpy(markers.view(np.uint8).reshape(-1).copy()).cuda()
    ct = torch.from_numpy(np.asarray(counts, np.int32).copy()).cuda()
    h.draw_markers(t, mt, ct, width=width, channels=channels, **kw)
    h.synchronize()
    return t.cpu().numpy()


def check(h, buf, width, channels, markers, counts, K=None, dist=None, flags=ALL, line_width=1, color=ovr.RED):
    exp = buf.copy()
    coords = ovr.draw_markers(exp, width, channels, markers, counts, K, dist, flags, line_width, color)
    assert ovr.half_integer_margin(coords) >= 1e-3
    got = device_draw(h, buf, width, channels, markers, np.asarray(counts, np.int32), K=K, dist=dist, flags=flags, line_width=line_width, color=color)
    bad = np.argwhere(got != exp)
    assert bad.size == 0, "first differing byte (frame, row, byte): %s, %d differ" % (bad[0], len(bad))
    assert np.all(got[:, :, width * channels:] == 0xA5)
    return got


@pytest.fixture(scope="module")
def handle():
    from aruco_amd import capi

    h = capi.Handle(640, 480, max_batch=4, device=0)
    yield h
    h.close()


@pytest.fixture(scope="module")
def small_cases():
    """Per frame size: 4 frames with counts 2, 0, 1, -1 in a cap of 3; the slots past a frame's count hold markers that must not appear."""
    from aruco_amd import capi

    out = {}
    for width, height in ((70, 50), (64, 48)):
        K = small_K(width, height)

        def build(j, width=width, height=height):
            tz = 0.5 + 0.0137 * j
            poses = [([0.31, -0.52, 0.2], [0.03, -0.02, tz]), ([-0.4, 0.3, -0.6], [-0.06, 0.03, tz + 0.1]), ([0.7, 0.2, 0.1], [0.0, 0.05, tz + 0.05])]
            ms = np.zeros((4, 3), capi.MARKER_DTYPE)
            for f in range(4):
                ms[f, 0] = marker(7 + 100 * f, quad(width * 0.35, height * 0.45, 20, 0.3 + f), 0.05, *poses[0])
                ms[f, 1] = marker(1023 - f, quad(width * 0.7, height * 0.55, 15.5, -0.5 + f), 0.04, *poses[1])
                ms[f, 2] = marker(55, quad(width * 0.5, height * 0.5, 30, 0.1), 0.05, *poses[2])
            return ms, np.array([2, 0, 1, -1], np.int32)

        out[(width, height)] = (K,) + settle(build, K, DIST, ALL)
    return out


@pytest.mark.parametrize("line_width", [1, 2, 3])
@pytest.mark.parametrize("channels", [1, 3])
@pytest.mark.parametrize("size", [(70, 50), (64, 48)])
def test_every_primitive_on_padded_frames(handle, small_cases, size, channels, line_width):
    """All flags, counts 2, 0, 1, -1, row_stride = width * channels + 5: equal to the restatement byte for byte; frames 1 and 3 and every
    padding byte come back as they went in."""
    width, height = size
    K, markers, counts = small_cases[size]
    buf = make_buffer(4, width, height, channels)
    got = check(handle, buf, width, channels, markers, counts, K, DIST, ALL, line_width, (30, 200, 90))
    assert np.array_equal(got[1], buf[1]) and np.array_equal(got[3], buf[3])
    assert not np.array_equal(got[0], buf[0]) and not np.array_equal(got[2], buf[2])
    if line_width == 1:
        # the setYperpendicular cube too
        check(handle, buf, width, channels, markers, counts, K, DIST, ALL | ovr.Y_PERP, 1, (30, 200, 90))


@pytest.mark.parametrize("line_width", [1, 3])
def test_edges_in_every_octant(handle, line_width):
    """One 60 x 60 quad turned through eight angles on 96 x 96 frames: its edges run in every octant."""
    from aruco_amd import capi

    angles = [np.deg2rad(11 + 22.5 * k) for k in range(8)]
    ms = np.zeros((8, 1), capi.MARKER_DTYPE)
    octants = set()
    for k, a in enumerate(angles):
        q = quad(48, 48, 60, a)
        ms[k, 0] = marker(k, q)
        r = np.rint(q.astype(np.float32))
        for i in range(4):
            d = r[(i + 1) % 4] - r[i]
            octants.add(int(np.floor(np.arctan2(d[1], d[0]) / (np.pi / 4))) % 8)
    assert octants == set(range(8))
    for channels in (1, 3):
        check(handle, make_buffer(8, 96, 96, channels), 96, channels, ms, np.ones(8, np.int32), flags=ovr.OUTLINE | ovr.IDS, line_width=line_width,
              color=(255, 255, 0))


def test_a_later_marker_overwrites_an_earlier_one_on_every_run(handle):
    from aruco_amd import capi

    ms = np.zeros((1, 2), capi.MARKER_DTYPE)
    ms[0, 0] = marker(12, quad(30, 24, 26, 0.2))
    ms[0, 1] = marker(345, quad(36, 27, 24, 0.9))
    buf = make_buffer(1, 70, 50, 3)
    kw = dict(flags=ovr.OUTLINE | ovr.IDS, line_width=3, color=(10, 20, 30))
    a = check(handle, buf, 70, 3, ms, [2], **kw)
    b = device_draw(handle, buf, 70, 3, ms, [2], **kw)
    assert a.tobytes() == b.tobytes()
    # the order matters in this input: the other order paints other bytes
    swapped = buf.copy()
    ovr.draw_markers(swapped, 70, 3, ms[:, ::-1], [2], **kw)
    assert not np.array_equal(swapped, a)


def test_clipping_and_dropped_primitives(handle):
    """Corners left of, above and right of the frame; an axis whose z end projects thousands of pixels outside; a marker whose pose
    projects nothing (depth 0 or beyond 2^20): its outline and id are still drawn."""
    from aruco_amd import capi

    width, height = 70, 50
    K = small_K(width, height)
    s = 0.05
    lost = marker(9, quad(35, 25, 18, 0.4), s, [0.0, 0.0, 0.0], [1e6, 0.0, 0.0])
    pr_pose, pr_none = ovr.Prims(), ovr.Prims()
    ovr.marker_prims(pr_pose, lost, K, DIST, ALL, 1, ovr.RED)
    nopose = lost.copy()
    nopose["has_pose"] = 0
    ovr.marker_prims(pr_none, nopose, K, DIST, ALL, 1, ovr.RED)
    assert pr_pose.items == pr_none.items and len(pr_none.items) == 17     # 4 edges, 3 x 4 sides, the id

    def build(j):
        ms = np.zeros((3, 1), capi.MARKER_DTYPE)
        ms[0, 0] = marker(3, [[-12.4, -7.3], [width + 9.6, -3.2], [width + 4.1, 30.7], [-6.6, 41.2]], s, [0.2, 0.1, -0.3], [0.02, 0.01, 0.6 + 0.011 * j])
        # the z axis points at the camera and ends just in front of its plane
        ms[1, 0] = marker(4, quad(30, 20, 16, 0.1), s, [np.pi, 0.0, 0.0], [0.011, -0.007, 3 * np.float32(s) * (1 + 1e-3 + 1e-4 * j)])
        ms[2, 0] = lost
        return ms, np.ones(3, np.int32)

    markers, counts = settle(build, K, None, ALL)
    far = ovr.project(ovr.marker_axis_points(s), markers[1, 0]["rvec"], markers[1, 0]["tvec"], K, None)[3]
    assert 1000 < np.max(np.abs(far)) < 2 ** 20
    for channels in (1, 3):
        got = check(handle, make_buffer(3, width, height, channels), width, channels, markers, counts, K, None, ALL, 2, (0, 255, 255))
        assert not np.array_equal(got[2], make_buffer(3, width, height, channels)[2])


def test_boards(handle):
    """Axis (width 2, labels X Y Z) and cube of a board, both setYperpendicular forms, on 160 x 120; a board without a pose draws nothing."""
    import torch
    from aruco_amd import capi

    width, height = 160, 120
    K = np.array([[150.5, 0, 80.25], [0, 149.25, 59.5], [0, 0, 1]], np.float32)
    for j in range(64):
        boards = np.zeros(2, capi.BOARD_DTYPE)
        boards[0] = (6, 1, [0.5, -0.35, 0.15], [0.01, 0.02, 0.55 + 0.0113 * j])
        boards[1] = (0, 0, [0.5, -0.35, 0.15], [0.01, 0.02, 0.6])
        pr = ovr.Prims()
        for flags in (ovr.AXIS | ovr.CUBE, ovr.AXIS | ovr.CUBE | ovr.Y_PERP):
            ovr.board_prims(pr, boards[0], 0.06, K, DIST, flags)
        if ovr.half_integer_margin(pr.coords) >= 1e-3:
            break
    assert ovr.half_integer_margin(pr.coords) >= 1e-3
    for channels in (1, 3):
        for flags in (ovr.AXIS | ovr.CUBE, ovr.AXIS | ovr.CUBE | ovr.Y_PERP, ovr.CUBE):
            buf = make_buffer(2, width, height, channels)
            exp = buf.copy()
            ovr.draw_boards(exp, width, channels, boards, 0.06, K, DIST, flags)
            t = torch.from_numpy(buf.copy()).cuda()
            handle.draw_boards(t, torch.from_numpy(boards.view(np.uint8).copy()).cuda(), 0.06, K, DIST, flags=flags, width=width, channels=channels)
            handle.synchronize()
            got = t.cpu().numpy()
            assert np.array_equal(got, exp) and not np.array_equal(got[0], buf[0]) and np.array_equal(got[1], buf[1])
            host = buf.copy()
            handle.draw_boards(host, boards, 0.06, K, DIST, flags=flags, width=width, channels=channels)
            assert np.array_equal(host, exp)


def test_detect_then_draw_without_leaving_the_device():
    """One synthetic marker at 320 x 240: detect_batch leaves markers and counts on the device, draw_markers reads them there. Equal to
    drawing from a host copy of the same markers, and to the restatement."""
    import torch
    from aruco_amd import capi, synth

    rng = np.random.RandomState(5)
    lay = synth.frame_layout(rng, 320, 240, n_markers=1, side_range=(80, 100), margin=30)
    gray = synth.render_frame(lay, 320, 240, rng).numpy()
    frames = torch.from_numpy(gray[None].copy()).cuda()
    cap = 8
    h = capi.Handle(320, 240, max_batch=1, device=0)
    out = torch.zeros(cap * capi.MARKER_DTYPE.itemsize, dtype=torch.uint8, device="cuda")
    n = torch.zeros(1, dtype=torch.int32, device="cuda")
    K = None
    for j in range(32):   # the corners do not depend on the camera, the pose does: take the first camera that satisfies the input condition
        K = np.array([[300.5 + 7.25 * j, 0, 160.25], [0, 298.75 + 7.25 * j, 119.5], [0, 0, 1]], np.float32)
        h.detect_batch_device(frames.data_ptr(), 1, 320, 240, out.data_ptr(), cap, n.data_ptr(), K=K, dist=DIST, marker_size=0.05)
        h.synchronize()
        host_m = out.cpu().numpy().view(capi.MARKER_DTYPE).reshape(1, cap).copy()
        host_n = n.cpu().numpy().copy()
        assert host_n[0] == 1 and int(host_m[0, 0]["id"]) == lay[0]["id"] and host_m[0, 0]["has_pose"]
        exp = gray[None].copy()
        if ovr.half_integer_margin(ovr.draw_markers(exp, 320, 1, host_m, host_n, K, DIST, ALL, 2, ovr.RED)) >= 1e-3:
            break
    else:
        raise AssertionError("no camera with every projected coordinate 1e-3 from a half-integer")
    # the chain: detection queued, the drawing behind it on the same stream, no synchronisation in between
    h.detect_batch_device(frames.data_ptr(), 1, 320, 240, out.data_ptr(), cap, n.data_ptr(), K=K, dist=DIST, marker_size=0.05)
    h.draw_markers(frames, out, n, K=K, dist=DIST, flags=ALL, line_width=2)
    h.synchronize()
    got = frames.cpu().numpy()
    assert np.array_equal(got, exp) and not np.array_equal(got, gray[None])
    host = gray[None].copy()
    h.draw_markers(host, host_m, host_n, K=K, dist=DIST, flags=ALL, line_width=2)
    assert np.array_equal(host, exp)
    h.close()


def test_drawing_leaves_the_single_frame_graph_valid():
    """detect three times (the third call replays the captured graph), draw into a 1080p host frame, detect again: the same bytes."""
    from aruco_amd import capi
    from aruco_amd.fixtures import load_case

    gray, doc = load_case("single")
    intr = doc["intrinsics"]
    h = capi.Handle(1920, 1080, max_batch=1, device=0)
    for _ in range(3):
        third = h.detect(gray, K=intr["K"], dist=intr["dist"], marker_size=1.0)
    assert len(third) == len(doc["markers"])
    frame = np.zeros((1, 1080, 1920, 3), np.uint8)
    scaled = third.copy()
    scaled["corners"] *= 2.0
    h.draw_markers(frame, scaled.reshape(1, -1), np.array([len(scaled)], np.int32), K=intr["K"], dist=intr["dist"], flags=ALL, line_width=3)
    assert frame.any()
    again = h.detect(gray, K=intr["K"], dist=intr["dist"], marker_size=1.0)
    assert again.tobytes() == third.tobytes()
    h.close()


def test_invalid_arguments_name_what_is_wrong(handle):
    from aruco_amd import capi

    ms = np.zeros((1, 1), capi.MARKER_DTYPE)
    ms[0, 0] = marker(1, quad(30, 20, 16, 0.1))
    one = np.ones(1, np.int32)
    K = small_K(70, 50)

    def err(code, word, **kw):
        frames = kw.pop("frames", None)
        if frames is None:
            frames = np.zeros((1, 50, 70 * 3), np.uint8)
        args = dict(width=70, channels=3)
        args.update(kw)
        with pytest.raises(capi.ArucoHipError) as e:
            handle.draw_markers(frames, ms, one, **args)
        assert e.value.code == code and word in str(e.value)

    err(capi.E_INVALID, "channels", channels=2)
    err(capi.E_INVALID, "channels", channels=4)
    err(capi.E_INVALID, "line_width", line_width=0)
    err(capi.E_INVALID, "line_width", line_width=8)
    err(capi.E_INVALID, "K is required", flags=ovr.AXIS)
    err(capi.E_INVALID, "K is required", flags=ovr.OUTLINE | ovr.CUBE)
    err(capi.E_INVALID, "row_stride", width=71)
    err(capi.E_UNSUPPORTED, "width", frames=np.zeros((1, 50, 641 * 3), np.uint8), width=641)
    err(capi.E_UNSUPPORTED, "height", frames=np.zeros((1, 481, 70 * 3), np.uint8))
    boards = np.zeros(1, capi.BOARD_DTYPE)
    with pytest.raises(capi.ArucoHipError) as e:
        handle.draw_boards(np.zeros((1, 50, 70), np.uint8), boards, 0.05, None)
    assert e.value.code == capi.E_INVALID and "K is required" in str(e.value)
    with pytest.raises(capi.ArucoHipError) as e:
        handle.draw_boards(np.zeros((1, 50, 140), np.uint8), boards, 0.05, K, width=70, channels=2)
    assert e.value.code == capi.E_INVALID and "channels" in str(e.value)
    # and a valid call still works afterwards
    ok = np.zeros((1, 50, 70 * 3), np.uint8)
    handle.draw_markers(ok, ms, one, width=70, channels=3)
    assert ok.any()
