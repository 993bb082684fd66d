"""Camera calibration on the device (arucohip_calibrate_camera / arucohip_calibrate_board_batch, cv::calibrateCamera for planar
views): exact and noisy synthetic views against the truth and against a scipy solve of the same model, every flag, the board
detections of a rendered stream left on the device, determinism, the single-frame graph after a calibration, and the errors."""
import numpy as np
import pytest

from tests import calib_ref as cr

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def handle():
    import torch  # noqa: F401
    from aruco_amd import capi

    h = capi.Handle(640, 480, max_batch=1)
    yield h
    h.close()


def rel(a, b):
    return np.abs(np.asarray(a) - np.asarray(b)) / np.maximum(np.abs(np.asarray(b)), 1e-300)


def assert_matches_scipy(got, ref, dist_scale=1.0):
    gi = cr.intr_of_result(got)
    # intrinsics 1e-6 relative; distortion coefficients 1e-6 absolute: k2 / k3 sit in a flat valley of the cost, where 30
    # Levenberg-Marquardt steps (OpenCV's stopping rule) from a perturbed guess end a few 1e-7 from the minimum
    scale = np.concatenate([np.abs(ref["intr"][:4]), np.maximum(np.abs(ref["intr"][4:]), dist_scale)])
    assert np.all(np.abs(gi - ref["intr"]) <= 1e-6 * scale), (gi, ref["intr"])
    assert abs(got["rms"] - ref["rms"]) <= 1e-7 * ref["rms"], (got["rms"], ref["rms"])


def test_exact_views_recover_the_camera(handle):
    objs, imgs = cr.make_views(20, noise=0.0)
    r = handle.calibrate_camera(objs, imgs, cr.SIZE)
    assert np.all(rel(r["K"][[0, 1, 0, 1], [0, 1, 2, 2]], cr.K_TRUE[[0, 1, 0, 1], [0, 1, 2, 2]]) < 1e-5), r["K"]
    assert np.max(np.abs(r["dist"] - cr.DIST_TRUE)) < 1e-4, r["dist"]
    assert r["rms"] < 1e-3
    assert r["rvecs"].shape == (20, 3) and r["tvecs"].shape == (20, 3) and np.all(r["per_view_rms"] < 1e-3)
    assert r["K"][2, 2] == 1 and r["K"][0, 1] == 0 and r["K"][1, 0] == 0


def test_noisy_views_equal_scipy(handle):
    objs, imgs = cr.make_views(20, noise=0.2, seed=11)
    r = handle.calibrate_camera(objs, imgs, cr.SIZE)
    ref = cr.scipy_calibrate(objs, imgs, cr.SIZE)
    assert_matches_scipy(r, ref)
    # per-view RMS and RMS are consistent: sqrt(sum n_v rms_v^2 / sum n_v)
    n = np.array([len(o) for o in objs])
    assert abs(np.sqrt(np.sum(n * r["per_view_rms"] ** 2) / n.sum()) - r["rms"]) < 1e-12 * r["rms"]


@pytest.mark.parametrize("flag", ["FIX_K3", "ZERO_TANGENT_DIST", "FIX_PRINCIPAL_POINT", "FIX_FOCAL_LENGTH", "FIX_ASPECT_RATIO",
                                  "USE_INTRINSIC_GUESS"])
def test_flags(handle, flag):
    from aruco_amd import capi

    flags = getattr(capi, "CALIB_" + flag)
    objs, imgs = cr.make_views(20, noise=0.2, seed=3)
    K0 = D0 = None
    if flag == "FIX_ASPECT_RATIO":   # only the ratio of K counts without USE_INTRINSIC_GUESS
        K0 = np.array([[700.0, 0, 0], [0, 695.0, 0], [0, 0, 1]])
    if flag == "FIX_FOCAL_LENGTH":   # focal lengths fixed at the guess
        flags |= capi.CALIB_USE_INTRINSIC_GUESS
        K0, D0 = cr.K_TRUE * np.array([[1, 1, 0.99], [1, 1, 1.01], [1, 1, 1]]), np.zeros(5)
    if flag == "USE_INTRINSIC_GUESS":
        K0 = cr.K_TRUE * np.array([[1.03, 1, 0.99], [1, 0.97, 1.01], [1, 1, 1]])
        D0 = np.array([-0.1, 0.0, 0.0, 0.0, 0.0])
    r = handle.calibrate_camera(objs, imgs, cr.SIZE, flags=flags, K=K0, dist=D0)
    ref = cr.scipy_calibrate(objs, imgs, cr.SIZE, flags=flags, K=K0, dist=D0)
    start = ref["start"]
    got = cr.intr_of_result(r)
    if flag == "FIX_K3":
        assert got[8] == start[8] == 0
    elif flag == "ZERO_TANGENT_DIST":
        assert got[6] == 0 and got[7] == 0
    elif flag == "FIX_PRINCIPAL_POINT":
        assert got[2] == (cr.SIZE[0] - 1) * 0.5 and got[3] == (cr.SIZE[1] - 1) * 0.5
    elif flag == "FIX_FOCAL_LENGTH":
        assert got[0] == K0[0, 0] and got[1] == K0[1, 1]
    elif flag == "FIX_ASPECT_RATIO":
        assert abs(got[0] / got[1] - 700.0 / 695.0) < 1e-14
    else:
        assert np.all(rel(got[:4], cr.intr_of(cr.K_TRUE, cr.DIST_TRUE)[:4]) < 2e-3), got
    assert_matches_scipy(r, ref)


def test_bit_reproducible(handle):
    objs, imgs = cr.make_views(16, noise=0.3, seed=21)
    a = handle.calibrate_camera(objs, imgs, cr.SIZE)
    b = handle.calibrate_camera(objs, imgs, cr.SIZE)
    for k in ("K", "dist", "rvecs", "tvecs", "per_view_rms"):
        assert a[k].tobytes() == b[k].tobytes(), k
    assert a["rms"] == b["rms"]


def test_device_resident_input_equals_host_input(handle):
    import torch

    objs, imgs = cr.make_views(10, noise=0.2, seed=8)
    a = handle.calibrate_camera(objs, imgs, cr.SIZE)
    o = torch.from_numpy(np.concatenate(objs)).cuda()
    m = torch.from_numpy(np.concatenate(imgs)).cuda()
    n = torch.tensor([len(x) for x in objs], dtype=torch.int32).cuda()
    b = handle.calibrate_camera_device(o.data_ptr(), m.data_ptr(), n.data_ptr(), len(objs), cr.SIZE)
    for k in ("K", "dist", "rvecs", "tvecs", "per_view_rms"):
        assert a[k].tobytes() == b[k].tobytes(), k


def test_nonplanar_and_invalid_inputs(handle):
    import ctypes as C
    from aruco_amd import capi
    from tests.util import load_case

    objs, imgs = cr.make_views(6, seed=2)
    bad = [o.copy() for o in objs]
    bad[2][5, 2] = 0.01
    with pytest.raises(capi.ArucoHipError) as e:
        handle.calibrate_camera(bad, imgs, cr.SIZE)
    assert e.value.code == capi.E_UNSUPPORTED
    L, h = handle.L, handle.h
    oa, ia = np.concatenate(objs), np.concatenate(imgs)
    npts = np.array([len(o) for o in objs], np.int32)
    K, d, rms = np.zeros(9), np.zeros(5), C.c_double()

    def call(n=npts, nviews=len(objs), w=cr.SIZE[0], hh=cr.SIZE[1], Kp=K, dp=d):
        p = lambda a: None if a is None else a.ctypes.data_as(C.c_void_p)
        return L.arucohip_calibrate_camera(h, p(oa), p(ia), p(n), nviews, 0, w, hh, 0, p(Kp), p(dp), None, None, None, C.byref(rms))

    few = npts.copy()
    few[1] = 3
    over = npts.copy()
    over[0] = capi.CALIB_MAX_VIEW_POINTS + 1
    assert call(nviews=0) == capi.E_INVALID
    assert call(n=few) == capi.E_INVALID
    assert call(w=0) == capi.E_INVALID and call(hh=-1) == capi.E_INVALID
    assert call(Kp=None) == capi.E_INVALID and call(dp=None) == capi.E_INVALID
    assert call(n=over) == capi.E_CAPACITY
    # the handle still detects correctly
    gray, doc = load_case("single")
    got = handle.detect(gray)
    assert [int(m["id"]) for m in got] == [e["id"] for e in doc["markers"]]


def board_setup(W=1920, H=1080):
    from tests.util import load_case

    _, doc = load_case("board")
    bc = doc["board_conf"]
    K = np.array([[1700.0, 0, 955.0], [0, 1690.0, 545.0], [0, 0, 1]], np.float32)
    return bc, K


def host_correspondences(markers, bc, marker_size, min_markers):
    """what the device gathers: the board markers of every frame (detection order), board corners scaled to metres"""
    obj = np.asarray(bc["obj"], np.float32).reshape(-1, 4, 3)
    side = np.float32(obj[0, 0, 0] - obj[0, 1, 0]), np.float32(obj[0, 0, 1] - obj[0, 1, 1]), np.float32(obj[0, 0, 2] - obj[0, 1, 2])
    mpp = float(np.float32(marker_size)) / np.sqrt(sum(float(s) * float(s) for s in side))   # the C ABI takes marker_size as float
    slot = {int(i): k for k, i in enumerate(bc["ids"])}
    objs, imgs, used = [], [], []
    for ms in markers:
        o, m = [], []
        for mk in ms:
            k = slot.get(int(mk["id"]))
            if k is None:
                continue
            o.append((obj[k].astype(np.float64) * mpp).astype(np.float32))
            m.append(np.asarray(mk["corners"], np.float32).reshape(4, 2))
        used.append(len(o) >= min_markers)
        if used[-1]:
            objs.append(np.concatenate(o))
            imgs.append(np.concatenate(m))
    return objs, imgs, np.array(used)


@pytest.mark.parametrize("streams", [1, 4], ids=["one_chunk", "four_chunks"])
def test_board_stream_end_to_end(monkeypatch, streams):
    import torch
    from aruco_amd import capi, synth

    W, H, NB = 1920, 1080, 256
    bc, K = board_setup(W, H)
    frames, _ = synth.make_board_stream(NB, bc["ids"], bc["obj"], K.reshape(-1), width=W, height=H, seed=77, device="cuda")
    torch.cuda.synchronize()
    host = frames.cpu().numpy()
    p = capi.default_params()
    p.corner_method = capi.CORNER_SUBPIX   # what the reference's calibration app detects with
    monkeypatch.setenv("ARUCOHIP_STREAMS", str(streams))
    h = capi.Handle(W, H, max_batch=NB, params=p)
    monkeypatch.delenv("ARUCOHIP_STREAMS")
    try:
        markers = h.detect_batch_host(host)
        if streams > 1:
            assert h.batch_chunks()[0] == streams
        r = h.calibrate_board_batch(NB, bc["ids"], bc["obj"], bc["info_type"], (W, H), marker_size=0.039, min_markers=8)
        objs, imgs, used = host_correspondences(markers, bc, 0.039, 8)
        assert np.array_equal(r["used"], used) and used.sum() >= 200
        ref = h.calibrate_camera(objs, imgs, (W, H))
    finally:
        h.close()
    assert abs(r["K"][0, 0] / K[0, 0] - 1) < 5e-3 and abs(r["K"][1, 1] / K[1, 1] - 1) < 5e-3, r["K"]
    assert abs(r["K"][0, 2] - K[0, 2]) < 3 and abs(r["K"][1, 2] - K[1, 2]) < 3, r["K"]
    assert r["rms"] < 0.3
    for k in ("K", "dist", "rvecs", "tvecs"):
        assert r[k].tobytes() == ref[k].tobytes(), k
    assert r["rms"] == ref["rms"]


def test_detect_graph_after_calibration(monkeypatch):
    """detect x3 (the third replays the captured single-frame graph), a calibration that allocates scratch no captured launch reads, detect:
    the bytes of every result equal an ARUCOHIP_GRAPH=0 handle's."""
    from aruco_amd import capi
    from tests.util import load_case

    gray, _ = load_case("board")
    objs, imgs = cr.make_views(30, noise=0.2, seed=4)
    monkeypatch.setenv("ARUCOHIP_GRAPH", "0")
    eager = capi.Handle(640, 480, max_batch=4)
    monkeypatch.delenv("ARUCOHIP_GRAPH")
    graphed = capi.Handle(640, 480, max_batch=4)
    try:
        outs = []
        for h in (graphed, eager):
            seq = [h.detect(gray) for _ in range(3)]
            c = h.calibrate_camera(objs, imgs, cr.SIZE)
            seq.append(h.detect(gray))
            outs.append((seq, c))
        (sg, cg), (se, ce) = outs
        for a, b in zip(sg, se):
            assert len(a) > 0 and np.asarray(a).tobytes() == np.asarray(b).tobytes()
        assert cg["K"].tobytes() == ce["K"].tobytes() and cg["rms"] == ce["rms"]
    finally:
        graphed.close()
        eager.close()


def build_shim_calib(out):
    import os
    import subprocess

    from aruco_amd import build_library

    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    build_library()
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-I" + os.path.join(root, "include"), os.path.join(root, "tests", "cpp", "shim_calib.cpp"),
                    "-o", str(out), "-L" + os.path.join(root, "aruco_amd"), "-larucohip", "-L/opt/rocm/lib",
                    "-Wl,-rpath," + os.path.join(root, "aruco_amd"), "-Wl,-rpath,/opt/rocm/lib"], check=True)


def test_shim_calibrate_save_read(tmp_path):
    """cv::calibrateCamera through the shim, CameraParameters::saveToFile, readFromXMLFile."""
    import subprocess

    exe = tmp_path / "shim_calib"
    build_shim_calib(exe)
    out = subprocess.run([str(exe), str(tmp_path / "camera.yml")], stdout=subprocess.PIPE, text=True, check=True).stdout.splitlines()
    rms = float(out[0])
    K, D = np.array(out[1].split(), float), np.array(out[2].split(), float)
    mem, back = np.array(out[3].split(), float), np.array(out[4].split(), float)
    assert rms < 1e-3
    assert np.all(np.abs(K[[0, 2, 4, 5]] - [1400, 965, 1390, 535]) < 1e-5 * np.array([1400, 965, 1390, 535]))
    assert np.max(np.abs(D - [-0.12, 0.05, 1e-3, -8e-4, 0.01])) < 1e-4
    assert np.all(np.abs(back - mem) <= 1e-9 * np.maximum(np.abs(mem), 1)) and list(back[-2:]) == [1920, 1080]
    assert np.all(np.abs(mem[:9] - K) <= 1e-6 * np.abs(K))
    text = (tmp_path / "camera.yml").read_text()
    for key in ("camera_matrix", "distortion_coefficients", "image_width", "image_height"):
        assert key in text
