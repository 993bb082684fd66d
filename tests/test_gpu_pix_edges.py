"""refine_pixels_kernel (SUBPIX, HARRIS) and locked_corners_kernel (aruco_amd/csrc/k_refine.hip) held to tests/pixref.py at their edges: every
family through the stage entry point arucohip_debug_refine_pixels, against the float64 reference (the fine bound of pixref.fine_bound about `exact`;
bit for bit where the reference says so: the integers of the pre-pass, returned starts, a padded frame against the packed one) and against the oracle
at the same bound; the refusals of the entry point and what a call leaves of the handle; and the kernels inside detection on 320 x 240 frames whose
markers reach to 3 px from the image's edges. test_pixref_cpu.py pins the oracle on the same cases and measures the bound."""
import ctypes as C

import numpy as np
import pytest

from tests import pixref as ref

pytestmark = pytest.mark.gpu

W0, H0 = 160, 120


@pytest.fixture(scope="module")
def handle():
    from aruco_amd import capi

    h = capi.Handle(W0, H0, max_batch=1)
    lim = capi.Limits()
    capi.load().arucohip_default_limits(C.byref(lim), W0, H0, 1)
    h.cap_corners = 4 * lim.candidates_per_frame
    yield h
    h.close()


def device_call(h):
    return lambda frame, width, pts, method, win, wsize: h.debug_refine_pixels(frame, pts, method, win=win, locked_wsize=wsize, width=width)


_device = {}


def device_side(h, family):
    if family not in _device:
        _device[family] = ref.run(ref.families()[family], device_call(h), limit=h.cap_corners)
    return _device[family]


@pytest.mark.parametrize("family", ref.FAMILIES)
def test_stage_entry_equals_the_reference_and_the_oracle(family, handle):
    from tests.test_pixref_cpu import oracle_side

    cases = ref.families()[family]
    got, orac = device_side(handle, family), oracle_side(family)
    packed = {c["name"]: g for f in ("interior", "locked_interior") for c, g in zip(ref.families()[f], device_side(handle, f))} if family == "stride" else {}
    bad, worst, worst_orc, skipped = [], {}, {}, 0
    for c, g, o in zip(cases, got, orac):
        r = ref.reference(c)
        ok, d, b = ref.judge(c, g)
        if "fragile_det" in r["fragile"]:
            skipped += 1
            continue
        m = ref.bound_key(c["method"])
        if not r["fragile"]:
            worst[m] = max(worst.get(m, 0.0), d)
            # the oracle at the same bound (a fragile case may have taken the other of its two results there)
            d_o = float(np.max(np.abs(g.astype(np.float64) - o.astype(np.float64))))
            worst_orc[m] = max(worst_orc.get(m, 0.0), d_o)
            ok = ok and (np.array_equal(g, o) if b == 0.0 else d_o <= b)
        if family == "stride":
            ok = ok and g.tobytes() == packed[c["name"].replace("stride", "interior").replace("/+%d/" % (c["stride"] - c["image"][1]), "/None/")].tobytes()
        if not ok:
            bad.append((c["name"], g.tolist(), r["exact"].tolist(), o.tolist(), b))
    print("%-16s device: worst from exact %s, from the oracle %s (%d cases, %d left out as fragile_det)"
          % (family, {m: "%.3g px" % v for m, v in worst.items()}, {m: "%.3g px" % v for m, v in worst_orc.items()}, len(cases), skipped))
    assert not bad, (len(bad), bad[:6])


@pytest.mark.parametrize("n", ["full", "odd"])
def test_one_call_carries_every_candidate_slot(n, handle):
    """4 * candidates_per_frame corners, the most a call takes, and a count that is no multiple of 4 (the last candidate repeats its last corner)."""
    n = handle.cap_corners if n == "full" else handle.cap_corners - 5
    cs = ref.many_points(n)
    for method, win, wsize in ((ref.SUBPIX, 7, 0), (ref.NONE, 0, 7)):
        got = handle.debug_refine_pixels(ref.image(cs[0]["image"]), [c["pt"] for c in cs], method, win=win, locked_wsize=wsize)
        assert got.shape == (n, 2)
        bad = []
        for c, g in zip(cs, got):
            r = ref.reference(c if wsize == 0 else dict(c, method="locked", win=0, wsize=7))
            ok, d, b = ref.judge_against(r, "locked" if wsize else "subpix", g, exactly=bool(wsize))
            if not ok:
                bad.append((c["name"], g.tolist(), r["exact"].tolist()))
        assert not bad, bad[:6]


# ---------------------------------------------------------------------------------------------------------------------------------
# refusals, and what a call leaves of the handle
# ---------------------------------------------------------------------------------------------------------------------------------
def test_hostile_inputs_are_refused_and_the_handle_detects_as_before():
    """Everything is checked before anything is launched: no corner that is not finite or beyond +-65534 reaches the device. The handle's
    single-frame graph (captured at the second detect) survives a refused call, an accepted one, and one whose padded frame outgrows the staging
    buffer the graph's launches read (the graph is then captured again)."""
    from aruco_amd import capi
    from aruco_amd.fixtures import load_case

    gray, _ = load_case("single")
    h = capi.Handle(640, 480, max_batch=1)
    lim = capi.Limits()
    capi.load().arucohip_default_limits(C.byref(lim), 640, 480, 1)
    cap = 4 * lim.candidates_per_frame
    img = ref.image(("checker", 64, 48, 10, 11))
    good = np.array([[30, 20], [10.5, 7.25]], np.float32)
    try:
        h.detect(gray)
        before = h.detect(gray).tobytes()
        assert len(before) > 0

        def refused(code, frame, pts, method, win=7, wsize=0, width=None):
            with pytest.raises(capi.ArucoHipError) as e:
                h.debug_refine_pixels(frame, pts, method, win=win, locked_wsize=wsize, width=width)
            assert e.value.code == code, (e.value.code, code)
            assert h.detect(gray).tobytes() == before

        refused(capi.E_INVALID, img, good, ref.SUBPIX, win=0)
        refused(capi.E_UNSUPPORTED, img, good, ref.SUBPIX, win=16)
        refused(capi.E_UNSUPPORTED, img, good, ref.HARRIS, wsize=32)
        refused(capi.E_INVALID, img, good, ref.HARRIS, wsize=-1)
        refused(capi.E_INVALID, img, good, ref.NONE)                                   # nothing to run
        refused(capi.E_INVALID, img, good, 3)                                          # LINES is no pixel method
        refused(capi.E_INVALID, np.zeros((48, 641), np.uint8), good, ref.HARRIS)       # wider than the handle
        refused(capi.E_INVALID, np.zeros((481, 64), np.uint8), good, ref.HARRIS)       # taller
        refused(capi.E_INVALID, img, good, ref.HARRIS, width=65)                       # row_stride < width
        refused(capi.E_CAPACITY, img, np.tile(good, (cap // 2 + 1, 1)), ref.SUBPIX)    # 4 * candidates_per_frame + 2 corners
        for v in (np.nan, np.inf, -np.inf, 65535.0, -65535.0, 1e30):
            for k in range(2):
                pts = good.copy()
                pts[1, k] = v
                refused(capi.E_INVALID, img, pts, ref.SUBPIX)
                refused(capi.E_INVALID, img, pts, ref.NONE, wsize=7)
        assert h.L.arucohip_debug_refine_pixels(h.h, None, 64, 48, 64, None, 1, ref.HARRIS, 0, 0) == capi.E_INVALID      # no frame, no corners
        # accepted calls: the largest coordinates the entry point lets through are harmless (every read is clamped or reflected), the candidate
        # list is borrowed, and the next detection gives the bytes it gave before
        far = np.array([[65534, 65534], [-65534, -65534], [65534, -3], [-1, -1], [65534, 10], [20, 48]], np.float32)
        for method, win, wsize in ((ref.SUBPIX, 15, 0), (ref.HARRIS, 0, 0), (ref.NONE, 0, 31), (ref.SUBPIX, 1, 31)):
            out = h.debug_refine_pixels(img, far, method, win=win, locked_wsize=wsize)
            assert np.all(np.isfinite(out))
            assert h.detect(gray).tobytes() == before
        big = ref.padded(np.ascontiguousarray(gray), 640 + 61)       # more bytes than the packed 640 x 480 frame the graph was captured with
        c = ref.families()["interior"][0]
        one = h.debug_refine_pixels(ref.image(c["image"]), [c["pt"]], ref.SUBPIX, win=c["win"])
        assert ref.judge(c, one[0])[0]
        h.debug_refine_pixels(big, good, ref.SUBPIX, win=7, width=640)
        assert h.detect(gray).tobytes() == before
        assert h.detect(gray).tobytes() == before
    finally:
        h.close()


# ---------------------------------------------------------------------------------------------------------------------------------
# inside detection
# ---------------------------------------------------------------------------------------------------------------------------------
WD, HD = 320, 240


def marker(mid, cx, cy, side, angle):
    """One layout entry of synth.render_frame: the marker's quad (TL, TR, BR, BL) turned by `angle` degrees about (cx, cy), and the quad of
    its one-cell quiet zone (9 / 7 of the side), which the image's edge may cut."""
    a = np.radians(angle)
    R = np.array([[np.cos(a), -np.sin(a)], [np.sin(a), np.cos(a)]])
    base = np.array([[-0.5, -0.5], [0.5, -0.5], [0.5, 0.5], [-0.5, 0.5]]) * side
    ctr = np.array([cx, cy], np.float64)
    return {"id": int(mid), "quad": base @ R.T + ctr, "quad_q": (base * 9.0 / 7.0) @ R.T + ctr}


def layout():
    """Four markers whose corners lie 4, 3, 5 and 6 px inside the left, top, right and bottom edge, and two interior ones, turned."""
    s = 56.0
    return [marker(11, 4 + s / 2, 118, s, 0), marker(12, 150, 3 + s / 2, s, 90), marker(13, WD - 1 - 5 - s / 2, 125, s, 180),
            marker(14, 170, HD - 1 - 6 - s / 2, s, 270), marker(15, 105, 125, 50, 30), marker(16, 215, 118, 48, 75)]


_frame = []


def frame():
    from aruco_amd import synth

    if not _frame:
        _frame.append(np.ascontiguousarray(synth.render_frame(layout(), WD, HD, np.random.RandomState(5), device="cpu").numpy()))
    return _frame[0]


CONFIGS = {"subpix3": (ref.SUBPIX, 3, 0), "subpix7": (ref.SUBPIX, 7, 0), "subpix15": (ref.SUBPIX, 15, 0), "harris": (ref.HARRIS, 7, 0),
           "locked7_subpix": (ref.SUBPIX, 7, 1), "locked7_harris": (ref.HARRIS, 7, 1), "locked31_harris": (ref.HARRIS, 31, 1)}
_expected = {}


def expected(name):
    """For one configuration: border_dist, lowered from the default in steps of 0.005 until the oracle reports every marker of the layout; the
    oracle's detection; and per marker the reference's corners: pixref on the unrefined quad of the oracle's candidate, turned by nRotations
    like :364-366. Once per process, on the CPU."""
    from oracle import orc

    if name not in _expected:
        method, p1, lock = CONFIGS[name]
        g = frame()
        for bd in (0.025, 0.02, 0.015, 0.01, 0.005, 0.0):
            o = orc.Oracle(corner_method=method, thres_p1=p1, use_locked_corners=lock, border_dist=bd)
            det = o.detect(g)
            if len(det) == len(layout()):
                break
        assert len(det) == len(layout()) and sorted(m["id"] for m in det) == sorted(m["id"] for m in layout())
        mname = ("locked+" if lock else "") + ("subpix" if method == ref.SUBPIX else "harris")
        want = {}
        for m in det:
            best = None
            for c in o.candidates():
                if c["id"] != m["id"]:
                    continue
                rs = [ref.reference_on(g, mname, q, win=p1, wsize=p1 if lock else 0) for q in np.roll(c["quad0"], c["nrot"], axis=0)]
                d = float(np.abs(np.array([r["exact"] for r in rs]) - np.array(m["corners"], np.float64).reshape(4, 2)).max())
                if best is None or d < best[0]:
                    best = (d, rs)
            assert best is not None and best[0] < 0.5, (m["id"], best and best[0])
            assert m["id"] not in want
            want[m["id"]] = best[1]
        _expected[name] = (bd, det, want, mname)
    return _expected[name]


def check(name, got):
    """The device's markers of one frame against the reference on the oracle's candidates: worst deviation in px, corners judged, fragile ones."""
    bd, det, want, mname = expected(name)
    assert [int(m["id"]) for m in got] == [m["id"] for m in det]
    worst, n, fragile, bad = 0.0, 0, 0, []
    for m in got:
        for k, r in enumerate(want[int(m["id"])]):
            g = np.array(m["corners"], np.float64).reshape(4, 2)[k]
            ok, d, b = ref.judge_against(r, mname, g, exactly=False)
            n, fragile = n + 1, fragile + bool(r["fragile"])
            if not r["fragile"]:
                worst = max(worst, d)
            if not ok:
                bad.append((int(m["id"]), k, g.tolist(), r["exact"].tolist(), b))
    assert not bad, bad
    return worst, n, fragile


def params_of(name):
    from aruco_amd import capi

    method, p1, lock = CONFIGS[name]
    p = capi.default_params()
    p.corner_method, p.thres_param1, p.use_locked_corners, p.border_dist = method, float(p1), lock, expected(name)[0]
    return p


@pytest.mark.parametrize("name", list(CONFIGS))
def test_detection_near_the_image_edges_equals_the_reference_on_the_oracles_candidates(name):
    from aruco_amd import capi

    h = capi.Handle(WD, HD, max_batch=1, params=params_of(name))
    try:
        got = h.detect(frame())
        worst, n, fragile = check(name, got)
        print("%-16s border_dist %.3f: %d markers, %d corners (%d fragile), worst %.3g px from exact" % (name, expected(name)[0], len(got), n, fragile, worst))
        assert len(got) == len(layout())
    finally:
        h.close()


def test_detection_of_a_padded_batch_on_the_device():
    """Two frames with rows of 333 bytes through detect_batch_device: the kernels index the caller's memory with the row stride."""
    import torch
    from aruco_amd import capi

    name, cap = "subpix7", 32
    g = frame()
    h = capi.Handle(WD, HD, max_batch=2, params=params_of(name))
    try:
        dev = torch.from_numpy(np.stack([ref.padded(g, 333), ref.padded(g, 333)])).cuda()
        out = torch.zeros((2, cap * capi.MARKER_DTYPE.itemsize), dtype=torch.uint8, device="cuda")
        cnt = torch.zeros(2, dtype=torch.int32, device="cuda")
        torch.cuda.synchronize()
        h.detect_batch_device(dev.data_ptr(), 2, WD, HD, out.data_ptr(), cap, cnt.data_ptr(), row_stride=333, frame_stride=333 * HD)
        h.batch_status()
        torch.cuda.synchronize()
        c = cnt.cpu().numpy()
        m = np.frombuffer(out.cpu().numpy().tobytes(), dtype=capi.MARKER_DTYPE).reshape(2, cap)
        for f in range(2):
            assert c[f] == len(layout())
            worst, n, fragile = check(name, m[f][:c[f]])
            print("padded batch, frame %d: %d corners (%d fragile), worst %.3g px from exact" % (f, n, fragile, worst))
        assert m[0][:c[0]].tobytes() == m[1][:c[1]].tobytes()
    finally:
        h.close()


def test_detection_of_a_bgr_frame():
    from aruco_amd import capi

    name = "locked7_harris"
    g = frame()
    h = capi.Handle(WD, HD, max_batch=1, params=params_of(name))
    try:
        bgr = np.ascontiguousarray(np.repeat(g[:, :, None], 3, axis=2))
        assert np.array_equal(h.bgr_to_gray(bgr), g)        # a gray pixel stays what it is: the expected corners are those of `g`
        worst, n, fragile = check(name, h.detect_bgr(bgr))
        print("bgr: %d corners (%d fragile), worst %.3g px from exact" % (n, fragile, worst))
    finally:
        h.close()
