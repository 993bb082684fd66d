"""5x5 fiducial marker, board and marker-set generation without a GPU: the NumPy restatement (tests/fiducial_ref.py) against the
reference's own artefacts (tests/golden/fiducial.json), the host-only entry points of the library against the restatement, error
codes, the C ABI symbols, and the compilation of the shim test program."""
import ctypes as C
import json
import os
import subprocess

import numpy as np
import pytest

from tests import fiducial_ref as fr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
SYMBOLS = ("arucohip_fiducial_marker_images", "arucohip_fiducial_marker_side", "arucohip_fiducial_marker_mat", "arucohip_fiducial_shuffle_ids",
           "arucohip_fiducial_board_size", "arucohip_fiducial_board_image", "arucohip_board_pix_to_meters", "arucohip_fiducial_distances",
           "arucohip_fiducial_select")
# the reference's CreateBoard test: 5 x 5, 100 px, distance int(100 * 0.2f), cv::theRNG().state = 4711, in this order
CREATE_BOARD = (("default", fr.PANEL, 20), ("chessboard", fr.CHESSBOARD, 0), ("frame", fr.FRAME, 20))


def run_lengths_image(d):
    v = np.zeros(len(d["runs"]), np.uint8)
    v[(0 if d["first"] else 1)::2] = 255
    return np.repeat(v, d["runs"]).reshape(d["shape"])


def load_fixture():
    doc = json.load(open(os.path.join(GOLDEN, "fiducial.json")))
    doc["images"] = {k: run_lengths_image(v) for k, v in doc["images"].items()}
    return doc


def watermark_golden(doc):
    """wartermark-marker-expected.png rebuilt: (image, [[y, x, value]] of its pixels that are neither 0 nor 255)"""
    img = run_lengths_image(doc["watermark"]["white"])
    grey = np.array(doc["watermark"]["grey"])
    img[grey[:, 0], grey[:, 1]] = grey[:, 2]
    return img, grey


def test_marker_images_restated():
    doc = load_fixture()
    mid, size = doc["marker"]["id"], doc["marker"]["size"]
    assert (mid, size) == (471, 500)
    assert fr.marker_image(mid, size).tobytes() == doc["images"]["marker"].tobytes()
    locked = fr.marker_image(mid, size, locked=True)
    assert locked.shape == (750, 750) and locked.tobytes() == doc["images"]["locked_marker"].tobytes()


def test_watermark_golden_differs_only_inside_the_bottom_border():
    doc = load_fixture()
    wm, grey = watermark_golden(doc)
    plain = fr.marker_image(471, 500)
    known = (wm == 0) | (wm == 255)
    assert np.array_equal(wm[known], plain[known])
    assert len(grey) == (~known).sum() <= 0.005 * wm.size
    sw = 500 // 7
    assert grey[:, 2].max() <= 30 and grey[:, 0].min() >= 6 * sw and grey[:, 0].max() < 7 * sw


def test_create_board_ids_and_corners_restated():
    doc = load_fixture()
    rng = fr.RNG(4711)
    for name, btype, dist in CREATE_BOARD:
        _, _, drawn, _, _ = fr.board_layout(btype, 5, 5, 100, dist)
        ids = fr.shuffle_ids(rng, drawn)
        _, used, obj = fr.board_image(btype, 5, 5, 100, dist, ids)
        want = doc["boards"][name]
        assert used == want["ids"] and want["info_type"] == 0, name
        assert obj.tobytes() == np.array(want["obj"], np.float32).tobytes(), name
    assert [len(doc["boards"][n]["ids"]) for n, _, _ in CREATE_BOARD] == [25, 13, 16]


def test_board_png_and_meters_restated():
    doc = load_fixture()
    pix, met = doc["boards"]["board_pix"], doc["boards"]["board_meters"]
    img, used, obj = fr.board_image(fr.PANEL, 4, 6, 150, 30, pix["ids"])
    assert img.shape == (1050, 690) and img.tobytes() == doc["images"]["board"].tobytes()
    # board_pix.yml describes the same board at 100 px per marker
    assert (obj * np.float32(100) / np.float32(150)).tobytes() == np.array(pix["obj"], np.float32).tobytes()
    assert met["ids"] == pix["ids"] and (pix["info_type"], met["info_type"]) == (0, 1)
    assert fr.pix_to_meters(pix["obj"], 0.039).tobytes() == np.array(met["obj"], np.float32).tobytes()


def test_selection_restated():
    D, E = fr.distance_matrix(), fr.entropies()
    assert np.array_equal(D, D.T) and not np.diag(D).any() and D.max() <= 25
    # the definition, literally, on a few pairs
    rng = np.random.default_rng(3)
    for i, j in rng.integers(0, 1024, (40, 2)):
        m, d = fr.marker_mat(int(i)), 99
        for _ in range(4):
            d = min(d, int((m != fr.marker_mat(int(j))).sum()))
            m = fr.rotate(m)
        assert D[i, j] == d
    ok, ids, md = fr.select(8, 0, D, E)
    assert ok and ids == sorted(ids) and len(set(ids)) == 8
    assert md == min(D[a, b] for a in ids for b in ids if a != b)
    assert int(np.argmax(E)) in ids
    ok, ids, _ = fr.select(5, int(E.max()) + 1, D, E)
    assert not ok and ids == [int(np.argmax(E))]


def test_c_abi_symbols():
    from aruco_amd import capi

    hdr = open(os.path.join(ROOT, "include", "arucohip.h")).read()
    names = subprocess.run(["nm", "-D", "--defined-only", capi.library_path()], stdout=subprocess.PIPE, text=True, check=True).stdout.split()
    for s in SYMBOLS:
        assert s in capi.SYMBOLS and (s + "(") in hdr and s in names, s


def test_header_is_c99():
    r = subprocess.run(["gcc", "-std=c99", "-Wall", "-Wextra", "-pedantic", "-Werror", "-fsyntax-only", "-x", "c",
                        os.path.join(ROOT, "include", "arucohip.h")], capture_output=True, text=True)
    assert r.returncode == 0 and "warning" not in r.stderr, r.stderr[-2000:]
    assert "arucohip_fiducial_select(" in open(os.path.join(ROOT, "include", "arucohip.h")).read()


def test_marker_mat_and_side_through_the_library():
    from aruco_amd import capi

    for mid in range(1024):
        assert np.array_equal(capi.fiducial_marker_mat(mid), fr.marker_mat(mid)), mid
    for size in (7, 8, 56, 99, 100, 150, 500, 1001, 10922):
        for locked in (False, True):
            assert capi.fiducial_marker_side(size, locked) == fr.marker_side(size, locked), (size, locked)
    assert capi.fiducial_marker_side(6) == 0 and capi.fiducial_marker_side(16384) == 0 and capi.fiducial_marker_side(16383) == 16383
    assert capi.fiducial_marker_side(10923, True) == 16383 and capi.fiducial_marker_side(10924, True) == 0   # 10924 + 2 * 2731 = 16386
    for mid in (-1, 1024):
        with pytest.raises(capi.ArucoHipError) as e:
            capi.fiducial_marker_mat(mid)
        assert e.value.code == capi.E_INVALID


def test_shuffle_through_the_library():
    from aruco_amd import capi

    doc = load_fixture()
    state, rng = 4711, fr.RNG(4711)
    for name, btype, dist in CREATE_BOARD:
        _, _, drawn, nm = capi.fiducial_board_size(btype, (5, 5), 100, dist)
        ids, state = capi.fiducial_shuffle_ids(state, drawn)
        assert ids.tolist() == fr.shuffle_ids(rng, drawn) and state == rng.state
        assert ids[:nm].tolist() == doc["boards"][name]["ids"]
    excluded = [0, 5, 1023, 77, 5]
    ids, state = capi.fiducial_shuffle_ids(2**63 + 12345, 1019, excluded)
    rng = fr.RNG(2**63 + 12345)
    assert ids.tolist() == fr.shuffle_ids(rng, 1019, excluded) and state == rng.state
    assert not set(ids.tolist()) & set(excluded) and len(set(ids.tolist())) == 1019
    assert capi.fiducial_shuffle_ids(1, 0)[0].size == 0
    for n, ex in ((1025, []), (1020, excluded), (3, [1024]), (3, [-1])):
        with pytest.raises(capi.ArucoHipError) as e:
            capi.fiducial_shuffle_ids(1, n, ex)
        assert e.value.code == capi.E_INVALID


def test_board_size_through_the_library():
    from aruco_amd import capi

    for btype in (fr.PANEL, fr.CHESSBOARD, fr.FRAME):
        for gw, gh, size, dist in ((5, 5, 100, 20), (4, 6, 150, 30), (1, 7, 57, 0), (7, 1, 8, 3), (2, 2, 7, 1), (3, 4, 64, 10), (1, 1, 70, 5)):
            W, H, drawn, cells, _ = fr.board_layout(btype, gw, gh, size, dist)
            if btype == fr.CHESSBOARD and len(cells) > drawn:
                with pytest.raises(capi.ArucoHipError) as e:
                    capi.fiducial_board_size(btype, (gw, gh), size, dist)
                assert e.value.code == capi.E_INVALID
            else:
                assert capi.fiducial_board_size(btype, (gw, gh), size, dist) == (W, H, drawn, len(cells)), (btype, gw, gh, size, dist)
    for args in ((3, (2, 2), 100, 0), (-1, (2, 2), 100, 0), (0, (0, 2), 100, 0), (0, (2, 129), 7, 0), (0, (2, 2), 6, 0), (0, (2, 2), 100, -1),
                 (0, (128, 2), 128, 1), (0, (40, 40), 7, 0)):
        with pytest.raises(capi.ArucoHipError) as e:
            capi.fiducial_board_size(*args)
        assert e.value.code == capi.E_INVALID, args
    # the outputs may be NULL
    assert capi.load().arucohip_fiducial_board_size(0, 2, 2, 100, 10, None, None, None, None) == capi.OK


def test_pix_to_meters_through_the_library():
    from aruco_amd import capi

    doc = load_fixture()
    pix, met = doc["boards"]["board_pix"], doc["boards"]["board_meters"]
    assert capi.board_pix_to_meters(pix["obj"], 0.039).tobytes() == np.array(met["obj"], np.float32).tobytes()
    rng = np.random.default_rng(11)
    obj = rng.uniform(-900, 900, (7, 4, 3)).astype(np.float32)
    assert capi.board_pix_to_meters(obj, 0.1234).tobytes() == fr.pix_to_meters(obj, 0.1234).tobytes()
    with pytest.raises(capi.ArucoHipError) as e:
        capi.board_pix_to_meters(np.zeros((2, 4, 3), np.float32), 0.05)
    assert e.value.code == capi.E_INVALID
    L = capi.load()
    assert L.arucohip_board_pix_to_meters(None, 1, 0.05, None) == capi.E_INVALID
    # NULL handles: the device calls refuse before touching anything
    buf = np.zeros(64, np.int32)
    n = C.c_int()
    assert L.arucohip_fiducial_marker_images(None, buf.ctypes.data, 1, 56, 0, buf.ctypes.data, 56, 0, 0) == capi.E_INVALID
    assert L.arucohip_fiducial_board_image(None, 0, 1, 1, 56, 0, 1, buf.ctypes.data, 1, buf.ctypes.data, 56, 0, None) == capi.E_INVALID
    assert L.arucohip_fiducial_distances(None, buf.ctypes.data, 0) == capi.E_INVALID
    assert L.arucohip_fiducial_select(None, 1, 0, buf.ctypes.data, C.byref(n), None) == capi.E_INVALID


def test_shim_program_compiles_and_links(tmp_path):
    """tests/cpp/shim_fiducial_create.cpp (the CreateMarker / CreateBoard sequences and the calls of the reference's four generator
    utilities through the shim) compiles warning-free in the shim's own branch and against the mock OpenCV headers, and links."""
    from aruco_amd import build_library

    build_library()
    src = os.path.join(ROOT, "tests", "cpp", "shim_fiducial_create.cpp")
    inc = "-I" + os.path.join(ROOT, "include")
    link = ["-L" + os.path.join(ROOT, "aruco_amd"), "-larucohip", "-L/opt/rocm/lib", "-Wl,-rpath," + os.path.join(ROOT, "aruco_amd"),
            "-Wl,-rpath,/opt/rocm/lib"]
    r = subprocess.run(["g++", "-std=c++11", "-O1", "-Wall", "-Wextra", "-Werror", inc, src, "-o", str(tmp_path / "shim_fiducial_create")] + link,
                       capture_output=True, text=True)
    assert r.returncode == 0 and "warning" not in r.stderr, r.stderr[-3000:]
    r = subprocess.run(["g++", "-std=c++11", "-Wall", "-Wextra", "-DARUCOHIP_USE_OPENCV", "-I" + os.path.join(ROOT, "tests", "cpp", "mock_opencv"), inc,
                        "-fsyntax-only", src], capture_output=True, text=True)
    assert r.returncode == 0 and "warning" not in r.stderr, r.stderr[-3000:]


REFERENCE = os.environ.get("REFERENCE", "/root/reference")   # the checkout oracle/Makefile reads too
UTILITIES = ("aruco_create_marker", "aruco_create_board", "aruco_selectoptimalmarkers", "aruco_board_pix2meters")


@pytest.mark.skipif(not os.path.exists(os.path.join(REFERENCE, "utils", UTILITIES[0] + ".cpp")), reason="no reference checkout")
@pytest.mark.parametrize("name", UTILITIES)
def test_reference_generator_utilities_compile_against_the_shim(tmp_path, name):
    """The reference's four generator utilities, compiled exactly as they lie in its checkout (nothing copied): "aruco.h", "board.h" and
    "arucofidmarkers.h" resolve to the shim (tests/cpp/ref_compat/), OpenCV's core + highgui to the mock headers. -Wno-unused-variable:
    aruco_create_board.cpp has an unused local of its own. Run without arguments they print their usage line."""
    from aruco_amd import build_library

    build_library()
    exe = str(tmp_path / name)
    cpp = os.path.join(ROOT, "tests", "cpp")
    r = subprocess.run(["g++", "-std=c++11", "-Wall", "-Wextra", "-Wno-unused-variable", "-DARUCOHIP_USE_OPENCV", "-I" + os.path.join(cpp, "ref_compat"),
                        "-I" + os.path.join(cpp, "mock_opencv"), "-I" + os.path.join(ROOT, "include"), os.path.join(REFERENCE, "utils", name + ".cpp"),
                        os.path.join(cpp, "ref_compat", "drawing_stubs.cpp"), "-o", exe, "-L" + os.path.join(ROOT, "aruco_amd"), "-larucohip",
                        "-L/opt/rocm/lib", "-Wl,-rpath," + os.path.join(ROOT, "aruco_amd"), "-Wl,-rpath,/opt/rocm/lib"], capture_output=True, text=True)
    assert r.returncode == 0 and "warning" not in r.stderr, r.stderr[-3000:]
    r = subprocess.run([exe], capture_output=True, text=True)
    assert "Usage" in r.stderr
