"""refine_lines_kernel (aruco_amd/csrc/k_refine.hip: refine_one, fit_line) held to tests/lines_ref.py at its edges: every non-hostile case
of the families through the stage entry point arucohip_refine_candidate_lines, against the float64 reference (1e-4 relative of `exact`, the
fine bound in float32 spacings of `f32lines`) and against the oracle (fine bound); the hostile inputs whose contour indices stay in
0..n-1; and the kernel inside detection, on hand-written layouts whose expected corners are the reference applied to the oracle's
candidate contours. test_lines_edges_cpu.py pins the oracle on the same cases and measures the bound."""
import numpy as np
import pytest

from tests import lines_ref as ref

pytestmark = pytest.mark.gpu

FAMILIES = ("raster", "start", "length", "inverse", "short", "duplicate", "tie", "far", "lens")
K_LIST = [1400, 0, 960, 0, 1400, 540, 0, 0, 1]
DIST = list(ref.DIST_MAIN)


@pytest.fixture(scope="module")
def handles():
    """One handle of 640 x 480 and one as wide as a handle gets (16383; the entry point itself takes points up to 32767) for `far`."""
    from aruco_amd import capi

    small, wide = capi.Handle(640, 480, max_batch=1), capi.Handle(16383, 2048, max_batch=1)
    yield {"small": small, "wide": wide}
    small.close(), wide.close()


def cam(c):
    return (None, None) if c["K"] is None else (c["K"].reshape(-1), c["dist"])


@pytest.mark.parametrize("family", FAMILIES)
def test_stage_entry_equals_the_reference_and_the_oracle(family, handles):
    from oracle import orc

    h = handles["wide" if family == "far" else "small"]
    worst_ref = worst_orc = worst_rel = 0.0
    bad = []
    for c in ref.families()[family]:
        r = ref.reference(c)
        K, dist = cam(c)
        got = h.refine_candidate_lines(c["contour"], c["corners"], K=K, dist=dist)
        orac = orc.refine_lines(c["contour"], c["corners"], K=K, dist=dist)
        s_ref, s_orc, rel = float(ref.spacings(got, r["f32lines"]).max()), float(ref.spacings(got, orac).max()), ref.rel_dev(got, r["exact"])
        worst_ref, worst_orc, worst_rel = max(worst_ref, s_ref), max(worst_orc, s_orc), max(worst_rel, rel)
        if not (np.all(np.isfinite(got)) and s_ref <= ref.FINE_BOUND_SPACINGS and s_orc <= ref.FINE_BOUND_SPACINGS and rel <= ref.REL_TOL):
            bad.append((c["name"], s_ref, s_orc, rel))
    print("%-9s device: worst %.3f float32 spacings from f32lines, %.3f from the oracle, %.3g relative from exact (%d cases)"
          % (family, worst_ref, worst_orc, worst_rel, len(ref.families()[family])))
    assert not bad, bad[:8]


def test_hostile_inputs_return_and_leave_the_handle_intact(handles):
    """Inputs the reference has no defined result for. Read against refine_one before they were included: an absent corner's index is
    max(wave_maxi(-1), 0) = 0; every forward index is start + q, q < cnt <= n - 1, folded once into 0..n-1; a side without points
    (cnt == 0) reads only `start`; the backward walk forms (uint64)(j - 1) % n, always in 0..n-1, and stops after 2 n + 1 steps. Nothing is
    asserted about the corners such a call returns, only that it returns and that the next well-formed call gives the bytes it gave before."""
    from aruco_amd import capi

    h = handles["small"]
    probe = ref.families()["raster"][3]
    before = h.refine_candidate_lines(probe["contour"], probe["corners"]).tobytes()
    for c in ref.families()["hostile"]:
        r = ref.refine(c["contour"], c["corners"])
        assert r["hostile"] is not None and len(c["contour"]) <= 2000
        try:
            h.refine_candidate_lines(c["contour"], c["corners"])
        except capi.ArucoHipError as e:
            assert e.code in (capi.E_INVALID, capi.E_CAPACITY), c["name"]
        assert h.refine_candidate_lines(probe["contour"], probe["corners"]).tobytes() == before, c["name"]


# ---------------------------------------------------------------------------------------------------------------------------------
# inside detection
# ---------------------------------------------------------------------------------------------------------------------------------
def marker(mid, cx, cy, side, angle):
    """One layout entry of synth.render_frame: the marker's quad (TL, TR, BR, BL) turned by `angle` degrees about (cx, cy), and the quad of
    its one-cell quiet zone (9 / 7 of the side)."""
    a = np.radians(angle)
    R = np.array([[np.cos(a), -np.sin(a)], [np.sin(a), np.cos(a)]])
    base = np.array([[-0.5, -0.5], [0.5, -0.5], [0.5, 0.5], [-0.5, 0.5]]) * side
    ctr = np.array([cx, cy], np.float64)
    return {"id": int(mid), "quad": base @ R.T + ctr, "quad_q": (base * 9.0 / 7.0) @ R.T + ctr}


def small_layouts():
    """640 x 480: two markers a frame at 0, 45, 90, 135 degrees and one degree either side (the second one turned half a turn further, so
    that every nRotations occurs), sides 60 - 120 px; and one frame with a marker whose quiet zone ends 3 px from the left and top edges
    and one whose quiet zone ends 3 px from the right and bottom edges."""
    lay = []
    for i in range(6):
        a, b = ref.ANGLES[i], ref.ANGLES[i + 6] + 180 + 90 * (i % 2)
        lay.append([marker(10 + i, 170, 240, 60 + 12 * i, a), marker(40 + i, 460, 235, 120 - 12 * i, b)])
    s, q = 98.0, 63.0     # quiet zone of 126 px; the marker's own corners stay 17 px inside, clear of the 0.025 * 640 border filter
    lay.append([marker(77, 3 + q, 3 + q, s, 0), marker(78, 637 - q, 477 - q, s, 90), marker(79, 330, 150, 84, 180), marker(80, 300, 350, 64, 270)])
    return lay


def grid_layout():
    """1280 x 720: 9 x 7 markers whose 98 px quiet zones tile into one white sheet (a quiet zone of its own would be a second candidate per
    marker, and the flat candidate list holds 96 entries a frame). Sides of 76 px: borders of about 300 points clear the size filter of
    0.04 * 1280 * 4 = 205."""
    return [marker(100 + 9 * r + c, 199 + 49 + 98 * c, 17 + 49 + 98 * r, 98 * 7.0 / 9.0, 90 * ((r + c) % 4)) for r in range(7) for c in range(9)]


def render(layouts, width, height, seed):
    from aruco_amd import synth

    rng = np.random.RandomState(seed)
    return [synth.render_frame(l, width, height, rng, device="cpu").numpy() for l in layouts]


_expected = {}


def expected(key, frame, K, dist):
    """The oracle's detection of a frame, its decoded candidates, and the reference's corners for them (lines_ref on the candidate's own
    contour and unrefined quad, rotated by nRotations like :364-366), once per process."""
    from oracle import orc

    if key not in _expected:
        o = orc.Oracle()
        det = o.detect(frame, K=K, dist=dist)
        cands = [c for c in o.candidates(with_contour=True) if c["id"] >= 0]
        borders = o.contours()
        for c in cands:
            r = ref.refine(c["contour"], c["quad0"], None if K is None else np.array(K, np.float64).reshape(3, 3), dist)
            assert r["hostile"] is None
            c["want"] = np.roll(r["f32lines"], c["nrot"], axis=0)
            c["swapped"] = bool(np.array_equal(borders[c["idx"]]["pts"][::-1], c["contour"]) and not np.array_equal(borders[c["idx"]]["pts"], c["contour"]))
        # a marker seen by more than one candidate (its border's outer and inner edge) is reported once: the device is held to the candidate
        # the oracle kept, the one whose corners its detection reports (half a pixel tells two edges of one border apart)
        want = {}
        for m in det:
            same = [c for c in cands if c["id"] == m["id"]]
            d = [float(np.abs(c["want"] - np.array(m["corners"], np.float64).reshape(4, 2)).max()) for c in same]
            assert sorted(d)[0] < 0.5 and (len(d) == 1 or sorted(d)[1] > 0.5), (m["id"], d)
            assert m["id"] not in want
            want[m["id"]] = same[int(np.argmin(d))]["want"]
        _expected[key] = (det, cands, want)
    return _expected[key]


def check_frame(got, key, frame, K, dist):
    det, cands, want = expected(key, frame, K, dist)
    assert [int(m["id"]) for m in got] == [m["id"] for m in det]
    worst = 0.0
    for m in got:
        worst = max(worst, float(ref.spacings(np.array(m["corners"], np.float64).reshape(4, 2), want[int(m["id"])]).max()))
    return worst, len(det)


@pytest.mark.parametrize("with_cam", [False, True])
def test_detection_on_small_frames_equals_the_reference_on_the_oracles_candidates(with_cam):
    from aruco_amd import capi

    K, dist = (K_LIST, DIST) if with_cam else (None, None)
    layouts = small_layouts()
    frames = render(layouts, 640, 480, seed=931)
    h = capi.Handle(640, 480, max_batch=1)
    try:
        worst, swapped, nrots = 0.0, set(), set()
        for f, (frame, lay) in enumerate(zip(frames, layouts)):
            got = h.detect(frame, K=K, dist=dist)
            w, n = check_frame(got, ("small", f, with_cam), frame, K, dist)
            assert n == len(lay)                       # every marker of the layout, the two at the image's edges among them
            worst = max(worst, w)
            for c in expected(("small", f, with_cam), frame, K, dist)[1]:
                swapped.add(c["swapped"]), nrots.add(c["nrot"])
        print("small frames, camera %d: worst %.3f float32 spacings from f32lines; swapped %s, nRotations %s" % (with_cam, worst, sorted(swapped), sorted(nrots)))
        assert True in swapped and nrots == {0, 1, 2, 3}
        assert worst <= ref.FINE_BOUND_SPACINGS
    finally:
        h.close()


@pytest.mark.parametrize("with_cam", [False, True])
@pytest.mark.parametrize("batch", [1, 2])
def test_detection_of_63_markers_takes_the_grid_stride_loop(batch, with_cam):
    """One frame with more decoded candidates than the 48 blocks a frame gets: refine_lines_kernel's loop runs a second time. One frame per
    call on a max_batch = 1 handle and two copies on a max_batch = 2 handle (the two use different border pipelines)."""
    from aruco_amd import capi

    K, dist = (K_LIST, DIST) if with_cam else (None, None)
    frame = render([grid_layout()], 1280, 720, seed=47)[0]
    h = capi.Handle(1280, 720, max_batch=batch)
    try:
        if batch == 1:
            gots = [h.detect(frame, K=K, dist=dist)]
        else:
            gots = h.detect_batch_host(np.stack([frame, frame]), K=K, dist=dist)
        assert len(gots) == batch
        # launch_refine_lines starts 48 blocks a frame over the batch's flat candidate list
        assert all(48 < len(h.debug_candidates(frame=f)[1]) <= 96 for f in range(batch))
        for f, got in enumerate(gots):
            w, n = check_frame(got, ("grid", with_cam), frame, K, dist)
            print("grid of 63, batch %d frame %d, camera %d: %d markers, worst %.3f float32 spacings from f32lines" % (batch, f, with_cam, n, w))
            assert n == 63
            assert w <= ref.FINE_BOUND_SPACINGS
    finally:
        h.close()
