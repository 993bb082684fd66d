"""HRM dictionary and board generation on the device (arucohip_hrm_*, k_hrm.hip) against the NumPy restatement (tests/hrm_ref.py):
the device's glibc stream, dictionaries (codes, order, tau0, candidates examined), a large dictionary's invariants, determinism,
board images against the reference's board4x4.png and the restatement, errors, a rendered board found end to end, the single-frame
graph after these calls, and the shim's calls of the reference's two HRM utilities."""
import json
import os
import subprocess

import numpy as np
import pytest

from tests import hrm_ref as hr
from tests.test_hrm_create_cpu import load_board4x4

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def handle():
    import torch  # noqa: F401
    from aruco_amd import capi

    h = capi.Handle(640, 480, max_batch=1)
    yield h
    h.close()


@pytest.mark.parametrize("seed", [0, 1, 42, 2**31 + 7, 2**32 - 1])
@pytest.mark.parametrize("offset,count", [(0, 5000), (1, 777), (10_000_019, 4099)])
def test_device_stream(handle, seed, offset, count):
    assert np.array_equal(handle.debug_hrm_stream(seed, offset, count), hr.stream(seed, offset, count))


# every case lowers tau at least once; (8, 40) and (6, 40) lower it with |D| < 2, where the limit becomes 100000 / 15
CASES = [(3, 20, 1234), (4, 30, 1234), (5, 40, 1234), (5, 12, 7), (6, 40, 1234), (8, 40, 1234)]


@pytest.mark.parametrize("n,size,seed", CASES)
def test_dictionary_equals_restatement(handle, n, size, seed):
    events = []
    codes, tau0, examined = hr.create_dictionary(n, size, seed, events=events)
    assert events and tau0 < hr.initial_tau(n)
    if n in (6, 8):
        assert any(d < 2 and lim == hr.LIMIT // 15 for _, d, lim in events)
    got, gtau, gex = handle.hrm_create_dictionary(n, size, seed)
    assert got.tobytes() == codes.tobytes()
    assert (gtau, gex) == (tau0, examined)
    c = handle.debug_hrm_counters()
    assert c["accepted"] == size and c["decrements"] == len(events)
    assert c["syncs"] == c["windows"] == (examined - 1) // 65536 + 1


def test_tau_reaches_zero(handle):
    from aruco_amd import capi

    with pytest.raises(hr.TauZero):
        hr.create_dictionary(3, 100, 5)
    with pytest.raises(capi.ArucoHipError) as e:
        handle.hrm_create_dictionary(3, 100, 5)
    assert e.value.code == capi.E_INVALID and "tau reached 0" in str(e.value)


def test_large_dictionary_invariants(handle):
    n, size = 8, 1000
    codes, tau0, examined = handle.hrm_create_dictionary(n, size, 99)
    assert codes.size == size and len(set(codes.tolist())) == size and 1 <= tau0 <= hr.initial_tau(n)
    rot = hr.rotations(codes, n)   # (size, 4)
    selfd = np.min(hr.popcount(rot[:, 1:] ^ rot[:, :1]), axis=1)
    assert selfd.min() >= tau0
    # every pair, every rotation of the later marker against the earlier one's rotation 0
    d = np.min(hr.popcount(rot[None, :, :] ^ codes[:, None, None]), axis=2)
    iu = np.triu_indices(size, 1)
    assert d[iu].min() >= tau0
    assert examined > size


def test_repeat_and_seeds(handle):
    a = handle.hrm_create_dictionary(5, 30, 2024)
    b = handle.hrm_create_dictionary(5, 30, 2024)
    c = handle.hrm_create_dictionary(5, 30, 2025)
    assert a[0].tobytes() == b[0].tobytes() and a[1:] == b[1:]
    assert a[0].tobytes() != c[0].tobytes()


def test_board4x4_fixture(handle):
    png, yml, codes = load_board4x4()
    img, ids, obj = handle.hrm_board_image(codes, 4, (4, 4), False)
    assert img.tobytes() == png.tobytes()
    # the fixture's ids were written by an older getId() (1 << pos): the current one (2 << pos) is twice as large
    assert np.array_equal(ids, 2 * np.array(yml["ids"]))
    assert np.array_equal(obj, np.array(yml["obj"], np.float32))


@pytest.mark.parametrize("chromatic", [False, True])
def test_board_images_equal_restatement(handle, chromatic):
    rng = np.random.default_rng(5 + chromatic)
    for n in range(3, 9):
        gw, gh = (int(x) for x in rng.integers(1, 6, 2))
        nb = gw * gh
        codes = rng.integers(0, 1 << 62, nb + 3, dtype=np.uint64) & np.uint64((1 << (n * n)) - 1 if n < 8 else 2**64 - 1)
        img, ids, obj = handle.hrm_board_image(codes, n, (gw, gh), chromatic)
        want, wids, wobj = hr.board_image(codes, n, gw, gh, chromatic)
        assert img.shape == want.shape and img.tobytes() == want.tobytes(), (n, gw, gh)
        assert np.array_equal(obj, wobj)
        if n <= 5:
            assert np.array_equal(ids, wids)
        else:
            assert ids is None


def test_errors(handle):
    from aruco_amd import capi

    def code(f, *a):
        with pytest.raises(capi.ArucoHipError) as e:
            f(*a)
        return e.value.code

    for n in (2, 9):
        assert code(handle.hrm_create_dictionary, n, 10, 1) == capi.E_INVALID
    for size in (0, 4097):
        assert code(handle.hrm_create_dictionary, 5, size, 1) == capi.E_INVALID
    codes = np.arange(16, dtype=np.uint64)
    assert code(handle.hrm_board_image, codes[:15], 4, (4, 4), False) == capi.E_INVALID
    assert code(handle.hrm_board_image, codes, 2, (4, 4), False) == capi.E_INVALID
    assert code(handle.hrm_board_image, np.full(16, 1 << 40, np.uint64), 5, (4, 4), False) == capi.E_INVALID
    # getId() past 32 bits: ids refused for n >= 6, the image and obj work
    L, h = handle.L, handle.h
    img = np.zeros((1000, 1000), np.uint8)
    ids = np.zeros(4, np.int32)
    rc = L.arucohip_hrm_board_image(h, 6, 4, codes.ctypes.data, 2, 2, 0, img.ctypes.data, 1000, 0, ids.ctypes.data, None)
    assert rc == capi.E_UNSUPPORTED
    img6, ids6, obj6 = handle.hrm_board_image(codes[:4], 6, (2, 2), False)
    assert ids6 is None and img6.shape == (2 * 160 + 32, 2 * 160 + 32)


def rodrigues(r):
    r = np.asarray(r, float)
    th = np.linalg.norm(r)
    if th < 1e-15:
        return np.eye(3)
    k = r / th
    Kx = np.array([[0, -k[2], k[1]], [k[2], 0, -k[0]], [-k[1], k[0], 0]])
    return np.eye(3) + np.sin(th) * Kx + (1 - np.cos(th)) * Kx @ Kx


def test_end_to_end_board(handle):
    """a device dictionary (n = 5, 24 markers) rendered with position ids, scaled 1.5x into a white 1080p frame, detected with the
    HRM decoder, then found by board_detect: every marker with its id, the pose reprojecting within 1 px"""
    from aruco_amd import capi

    n = 5
    codes, tau0, _ = handle.hrm_create_dictionary(n, 24, 31337)
    img, ids, obj = handle.hrm_board_image(codes, n, (6, 4), False)
    H, W = 1080, 1920
    sh, sw = int(img.shape[0] * 1.5), int(img.shape[1] * 1.5)
    big = img[(np.arange(sh) / 1.5).astype(int)][:, (np.arange(sw) / 1.5).astype(int)]
    frame = np.full((H, W), 255, np.uint8)
    y0, x0 = (H - sh) // 2, (W - sw) // 2
    frame[y0:y0 + sh, x0:x0 + sw] = big
    K = np.array([[1000, 0, W / 2], [0, 1000, H / 2], [0, 0, 1]], np.float32)
    h = capi.Handle(W, H)
    try:
        h.set_dictionary(["".join("1" if (int(c) >> i) & 1 else "0" for i in range(n * n)) for c in codes], tau0)
        ms = h.detect(frame, K=K, dist=np.zeros(5, np.float32), marker_size=0.05)
        assert sorted(int(m["id"]) for m in ms) == list(range(24))
        pos = np.arange(24, dtype=np.int32)   # HRM detection reports the position in the dictionary, not getId()
        b = h.board_detect(ms, pos, obj, 0, K=K, dist=np.zeros(5, np.float32), marker_size=0.05)
        assert b["has_pose"] and len(b["markers"]) == 24 and b["prob"] == pytest.approx(1.0)
        R, t = rodrigues(b["rvec"]), np.asarray(b["tvec"], float)
        scale = 0.05 / 140.0
        err = 0.0
        for m in b["markers"]:
            X = obj[int(m["id"])].astype(float) * scale
            p = (K.astype(float) @ (R @ X.T + t[:, None])).T
            p = p[:, :2] / p[:, 2:]
            err = max(err, np.max(np.abs(p - np.asarray(m["corners"], float).reshape(4, 2))))
        assert err < 1.0
    finally:
        h.close()


def test_detect_graph_after_hrm_calls(monkeypatch):
    """detect x3 (the third replays the single-frame graph), HRM generation calls, detect: equal to an ARUCOHIP_GRAPH=0 handle's bytes"""
    from aruco_amd import capi
    from tests.util import load_case

    gray, _ = load_case("board")
    monkeypatch.setenv("ARUCOHIP_GRAPH", "0")
    eager = capi.Handle(640, 480, max_batch=4)
    monkeypatch.delenv("ARUCOHIP_GRAPH")
    graphed = capi.Handle(640, 480, max_batch=4)
    try:
        outs = []
        for h in (graphed, eager):
            seq = [h.detect(gray) for _ in range(3)]
            d = h.hrm_create_dictionary(5, 20, 3)
            seq.append(h.detect(gray))
            im = h.hrm_board_image(d[0], 5, (4, 5), True)
            s = h.debug_hrm_stream(3, 10**7, 100000)
            seq.append(h.detect(gray))
            outs.append((seq, d[0], im[0], s))
        (sg, *rg), (se, *re_) = outs
        for a, b in zip(sg, se):
            assert len(a) > 0 and np.asarray(a).tobytes() == np.asarray(b).tobytes()
        for a, b in zip(rg, re_):
            assert a.tobytes() == b.tobytes()
    finally:
        graphed.close()
        eager.close()


def test_shim_hrm_create(tmp_path):
    """tests/cpp/shim_hrm_create.cpp: the calls of the reference's aruco_hrm_create_dictionary and aruco_hrm_create_board through the
    shim, the toFile / fromFile and saveToFile / readFromFile round trips, MarkerCode's distances"""
    from aruco_amd import build_library

    build_library()
    exe = str(tmp_path / "shim_hrm_create")
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"),
                    os.path.join(ROOT, "tests", "cpp", "shim_hrm_create.cpp"), "-o", exe, "-L" + os.path.join(ROOT, "aruco_amd"), "-larucohip",
                    "-L/opt/rocm/lib", "-Wl,-rpath," + os.path.join(ROOT, "aruco_amd"), "-Wl,-rpath,/opt/rocm/lib"], check=True)
    out = subprocess.run([exe, str(tmp_path)], stdout=subprocess.PIPE, text=True, check=True, timeout=300).stdout
    res = json.loads(out.strip().splitlines()[-1])
    codes, tau0, examined = hr.create_dictionary(5, 12, 7)
    assert res["codes"] == [int(c) for c in codes] and res["tau0"] == tau0
    assert res["dict_roundtrip"] and res["board_roundtrip"] and res["two_arg"]
    D = [int(c) for c in codes]
    assert res["min_distance"] == hr.minimum_distance(D, 5)
    assert res["self"] == [int(x) for x in hr.self_distance(codes, 5)]
    assert res["d01"] == hr.distance(D[0], D[1], 5)
    assert res["dict_distance"] == int(hr.dict_distance(D[1:], [D[0]], 5)[0])
    assert res["ids"] == [hr.get_id(c, 5) for c in D[:4]]
    img, _, _ = hr.board_image(codes, 5, 2, 2)
    assert np.fromfile(os.path.join(str(tmp_path), "board.raw"), np.uint8).tobytes() == img.tobytes()
    cimg, _, _ = hr.board_image(codes, 5, 2, 2, True)
    assert np.fromfile(os.path.join(str(tmp_path), "board_chromatic.raw"), np.uint8).tobytes() == cimg.tobytes()
    assert res["marker_img"] == int((hr.marker_image(D[0], 5, 70) == 255).sum())
