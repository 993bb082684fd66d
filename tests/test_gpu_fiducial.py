"""5x5 fiducial marker, board and marker-set generation on the device (arucohip_fiducial_*, k_fiducial.hip) against the reference's
own artefacts (tests/golden/fiducial.json) and the NumPy restatement (tests/fiducial_ref.py): marker images (plain, locked, every
id in one call, host and device destinations, odd strides), the watermark golden, the three board layouts, the selection, a
generated board found end to end like the CPU oracle finds it, the single-frame graph after these calls, and the shim program."""
import json
import os
import subprocess

import numpy as np
import pytest

from tests import fiducial_ref as fr
from tests.test_fiducial_cpu import CREATE_BOARD, load_fixture, watermark_golden
from tests.util import rel_err

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# tests/test_gpu_parity.py: the tolerances of every comparison with the CPU oracle (ids and order exact)
CORNER_REL_TOL = 1e-4
POSE_REL_TOL = 1e-4


@pytest.fixture(scope="module")
def handle():
    import torch  # noqa: F401
    from aruco_amd import capi

    h = capi.Handle(640, 480, max_batch=1)
    yield h
    h.close()


@pytest.fixture(scope="module")
def doc():
    return load_fixture()


def code(f, *a, **kw):
    from aruco_amd import capi

    with pytest.raises(capi.ArucoHipError) as e:
        f(*a, **kw)
    return e.value.code


def test_marker_goldens(handle, doc):
    plain = handle.fiducial_marker_images([471], 500)
    assert plain.shape == (1, 500, 500) and plain[0].tobytes() == doc["images"]["marker"].tobytes()
    locked = handle.fiducial_marker_images([471], 500, locked=True)
    assert locked.shape == (1, 750, 750) and locked[0].tobytes() == doc["images"]["locked_marker"].tobytes()


def test_watermark_golden(handle, doc):
    wm, grey = watermark_golden(doc)
    got = handle.fiducial_marker_images([471], 500)[0]
    known = (wm == 0) | (wm == 255)
    excluded = int((~known).sum())
    print("watermark pixels excluded: %d of %d (%.3f %%)" % (excluded, wm.size, 100.0 * excluded / wm.size))
    assert excluded <= 0.005 * wm.size
    assert np.array_equal(got[known], wm[known])
    sw = 500 // 7
    assert wm[~known].max() <= 30 and grey[:, 0].min() >= 6 * sw and grey[:, 0].max() < 7 * sw


@pytest.mark.parametrize("size", [56, 100, 150])
@pytest.mark.parametrize("locked", [False, True])
def test_all_ids_in_one_call(handle, size, locked):
    got = handle.fiducial_marker_images(np.arange(1024), size, locked)
    side = fr.marker_side(size, locked)
    assert got.shape == (1024, side, side)
    for mid in range(1024):
        assert got[mid].tobytes() == fr.marker_image(mid, size, locked).tobytes(), mid


@pytest.mark.parametrize("size,locked,row_stride", [(100, False, 100), (100, False, 128), (100, True, 151), (57, False, 61), (150, True, 227),
                                                    (7, False, 7), (7, True, 9), (33, False, 35)])
def test_device_destination_and_strides(handle, size, locked, row_stride):
    """rows at every alignment: a device destination is painted in place, whatever its row stride; the bytes between the rows and the
    images stay untouched"""
    import torch

    ids = np.array([471, 0, 1023, 582, 5], np.int32)
    side = fr.marker_side(size, locked)
    image_stride = side * row_stride + 3
    for offset in (0, 1, 5):   # the first row's own misalignment
        buf = torch.full((offset + ids.size * image_stride + 16,), 77, dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()
        rc = handle.L.arucohip_fiducial_marker_images(handle.h, ids.ctypes.data, ids.size, size, int(locked), buf.data_ptr() + offset, row_stride,
                                                      image_stride, 1)
        assert rc == 0
        assert np.array_equal(buf.cpu().numpy(), _strided(ids, size, locked, row_stride, image_stride, offset)), offset
    # the same strides into host memory
    host = np.full(ids.size * image_stride + 16, 77, np.uint8)
    rc = handle.L.arucohip_fiducial_marker_images(handle.h, ids.ctypes.data, ids.size, size, int(locked), host.ctypes.data, row_stride, image_stride, 0)
    assert rc == 0
    assert np.array_equal(host, _strided(ids, size, locked, row_stride, image_stride, 0))


def _strided(ids, size, locked, row_stride, image_stride, offset):
    """what a buffer of 77s holds after the images were written at `offset` with these strides"""
    side = fr.marker_side(size, locked)
    want = np.full(offset + ids.size * image_stride + 16, 77, np.uint8)
    for i, mid in enumerate(ids):
        img = fr.marker_image(int(mid), size, locked)
        for y in range(side):
            o = offset + i * image_stride + y * row_stride
            want[o:o + side] = img[y]
    return want


def test_every_marker_decodes_to_its_id(handle):
    """each id's image on white goes through arucohip_detect and comes back as that id"""
    from aruco_amd import capi

    size, pitch, margin, per_row, rows = 100, 150, 60, 10, 5   # the margin keeps the corners clear of the detector's image-border filter
    W, H = per_row * pitch + 2 * margin, rows * pitch + 2 * margin
    imgs = handle.fiducial_marker_images(np.arange(1024), size)
    per_frame = per_row * rows
    det = capi.Handle(W, H, max_batch=1)
    try:
        for first in range(0, 1024, per_frame):
            frame = np.full((H, W), 255, np.uint8)
            ids = list(range(first, min(first + per_frame, 1024)))
            for k, mid in enumerate(ids):
                y0, x0 = margin + (k // per_row) * pitch + 25, margin + (k % per_row) * pitch + 25
                frame[y0:y0 + size, x0:x0 + size] = imgs[mid]
            found = det.detect(frame, cap=256)
            assert sorted(int(m["id"]) for m in found) == ids, first
    finally:
        det.close()


def test_board_png(handle, doc):
    pix = doc["boards"]["board_pix"]
    img, ids, obj = handle.fiducial_board_image(fr.PANEL, (4, 6), 150, 30, pix["ids"])
    assert img.shape == (1050, 690) and img.tobytes() == doc["images"]["board"].tobytes()
    assert ids.tolist() == pix["ids"]
    assert (obj * np.float32(100) / np.float32(150)).tobytes() == np.array(pix["obj"], np.float32).tobytes()


def test_create_board_goldens(handle, doc):
    from aruco_amd import capi

    state = 4711
    for name, btype, dist in CREATE_BOARD:
        _, _, drawn, nm = capi.fiducial_board_size(btype, (5, 5), 100, dist)
        drawn_ids, state = capi.fiducial_shuffle_ids(state, drawn)
        img, ids, obj = handle.fiducial_board_image(btype, (5, 5), 100, dist, drawn_ids)
        want = doc["boards"][name]
        assert ids.tolist() == want["ids"] and len(ids) == nm, name
        assert obj.tobytes() == np.array(want["obj"], np.float32).tobytes(), name
        assert img.tobytes() == fr.board_image(btype, 5, 5, 100, dist, drawn_ids.tolist())[0].tobytes(), name


GRIDS = [(1, 1, 56, 0), (1, 1, 100, 13), (1, 5, 57, 9), (6, 1, 64, 1), (3, 4, 150, 30), (5, 5, 99, 0), (7, 3, 8, 2), (2, 9, 45, 17), (4, 4, 7, 0)]


@pytest.mark.parametrize("btype", [fr.PANEL, fr.CHESSBOARD, fr.FRAME])
@pytest.mark.parametrize("centered", [True, False])
def test_board_images_equal_restatement(handle, btype, centered):
    from aruco_amd import capi

    rng = np.random.default_rng(17 + btype)
    for gw, gh, size, dist in GRIDS:
        ids = rng.permutation(1024)[:gw * gh + 2].astype(np.int32)
        want = fr.board_image(btype, gw, gh, size, dist, ids.tolist(), centered)
        if want is None:
            assert btype == fr.CHESSBOARD
            assert code(handle.fiducial_board_image, btype, (gw, gh), size, dist, ids, centered) == capi.E_INVALID
            continue
        img, used, obj = handle.fiducial_board_image(btype, (gw, gh), size, dist, ids, centered)
        assert img.shape == want[0].shape and img.tobytes() == want[0].tobytes(), (gw, gh, size, dist)
        assert used.tolist() == want[1] and obj.tobytes() == want[2].tobytes(), (gw, gh, size, dist)
    assert fr.board_image(fr.CHESSBOARD, 1, 1, 56, 0, [3]) is None   # the 1 x 1 chessboard is one of the refused grids


def test_board_device_destination(handle):
    import torch

    gw, gh, size, dist, row_stride, offset = 3, 2, 57, 9, 211, 3
    ids = np.array([471, 5, 26, 99, 182, 253], np.int32)
    want_img, _, want_obj = fr.board_image(fr.PANEL, gw, gh, size, dist, ids.tolist())
    H, W = want_img.shape
    buf = torch.full((offset + H * row_stride + 16,), 77, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    obj = np.zeros((6, 4, 3), np.float32)
    rc = handle.L.arucohip_fiducial_board_image(handle.h, fr.PANEL, gw, gh, size, dist, 1, ids.ctypes.data, ids.size, buf.data_ptr() + offset,
                                                row_stride, 1, obj.ctypes.data)
    assert rc == 0
    want = np.full(buf.numel(), 77, np.uint8)
    for y in range(H):
        want[offset + y * row_stride:offset + y * row_stride + W] = want_img[y]
    assert np.array_equal(buf.cpu().numpy(), want) and obj.tobytes() == want_obj.tobytes()


def test_errors(handle):
    from aruco_amd import capi

    assert code(handle.fiducial_marker_images, [1024], 100) == capi.E_INVALID
    assert code(handle.fiducial_marker_images, [-1], 100) == capi.E_INVALID
    assert code(handle.fiducial_marker_images, [5], 6) == capi.E_INVALID
    assert code(handle.fiducial_marker_images, [], 100) == capi.E_INVALID
    assert code(handle.fiducial_marker_images, np.zeros(1025, np.int32), 56) == capi.E_INVALID
    img = np.zeros(100 * 100, np.uint8)
    one = np.array([5, 6], np.int32)
    L, h = handle.L, handle.h
    assert L.arucohip_fiducial_marker_images(h, one.ctypes.data, 1, 100, 0, img.ctypes.data, 99, 0, 0) == capi.E_INVALID       # row_stride < side
    assert L.arucohip_fiducial_marker_images(h, one.ctypes.data, 2, 50, 0, img.ctypes.data, 50, 2000, 0) == capi.E_INVALID     # images overlap
    assert code(handle.fiducial_board_image, fr.PANEL, (2, 2), 100, 10, [1, 2, 3]) == capi.E_INVALID       # fewer ids than markers
    assert code(handle.fiducial_board_image, fr.PANEL, (2, 2), 100, 10, [1, 2, 3, 1024]) == capi.E_INVALID
    assert code(handle.fiducial_board_image, 3, (2, 2), 100, 10, [1, 2, 3, 4]) == capi.E_INVALID
    assert code(handle.fiducial_board_image, fr.FRAME, (2, 2), 6, 10, [1, 2, 3, 4]) == capi.E_INVALID
    assert code(handle.fiducial_select, 0) == capi.E_INVALID and code(handle.fiducial_select, 1025) == capi.E_INVALID


def test_distances(handle):
    import torch

    D = fr.distance_matrix()
    got = handle.fiducial_distances()
    assert got.dtype == np.int32 and np.array_equal(got, D)
    assert np.array_equal(got, got.T) and not np.diag(got).any()
    dev = torch.full((1024, 1024), -1, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    assert handle.L.arucohip_fiducial_distances(handle.h, dev.data_ptr(), 1) == 0
    assert np.array_equal(dev.cpu().numpy(), D)


def test_select(handle):
    from aruco_amd import capi

    D, E = fr.distance_matrix(), fr.entropies()
    for min_entropy in (0, 20):
        for n in (1, 2, 8, 24, 64, 200):
            ok, want, md = fr.select(n, min_entropy, D, E)
            assert ok
            ids, got_md = handle.fiducial_select(n, min_entropy)
            assert ids.tolist() == want and got_md == md, (n, min_entropy)
    # an entropy floor that leaves too few markers: the reference gives up part of the way
    floor = int(E.max()) - 3
    ok, want, _ = fr.select(200, floor, D, E)
    assert not ok and 1 <= len(want) < 200
    with pytest.raises(capi.ArucoHipError) as e:
        handle.fiducial_select(200, floor)
    assert e.value.code == capi.E_INVALID and "COUDL NOT ADD ANY MARKER" in str(e.value)
    assert e.value.partial.tolist() == want
    # above every marker's entropy only the first one is found
    with pytest.raises(capi.ArucoHipError) as e:
        handle.fiducial_select(2, int(E.max()) + 1)
    assert e.value.partial.tolist() == [int(np.argmax(E))]


def test_generated_board_end_to_end(handle, doc):
    """the board_pix panel as the generator paints it, on a white quiet zone: arucohip_detect and arucohip_board_detect with the
    generator's own ids / obj, against the CPU oracle on the same image (tests/test_gpu_parity.py's tolerances; ids and order exact)"""
    from aruco_amd import capi
    from oracle import orc

    pix = doc["boards"]["board_pix"]
    img, ids, obj = handle.fiducial_board_image(fr.PANEL, (4, 6), 150, 30, pix["ids"])
    margin = 60
    frame = np.full((img.shape[0] + 2 * margin, img.shape[1] + 2 * margin), 255, np.uint8)
    frame[margin:-margin, margin:-margin] = img
    # a quarter turn: the board faces the camera squarely, and a rotation vector near zero has no relative error to speak of
    frame = np.ascontiguousarray(np.rot90(frame))
    H, W = frame.shape
    K = np.array([[1200, 0, W / 2], [0, 1200, H / 2], [0, 0, 1]], np.float32)
    dist = np.zeros(5, np.float32)
    det = capi.Handle(W, H, max_batch=1)
    try:
        got = det.detect(frame, K=K, dist=dist, marker_size=0.039)
        ref = orc.Oracle().detect(frame, K=K, dist=dist, marker_size=0.039)
        assert sorted(int(m["id"]) for m in got) == sorted(pix["ids"])
        assert [int(m["id"]) for m in got] == [m["id"] for m in ref]
        for a, b in zip(got, ref):
            ca, cb = np.asarray(a["corners"], float).reshape(4, 2), np.asarray(b["corners"], float).reshape(4, 2)
            assert np.max(np.abs(ca - cb) / np.maximum(np.abs(cb), 1.0)) < CORNER_REL_TOL
        b = det.board_detect(got, ids, obj, 0, K, dist, 0.039)
        ob = orc.board_detect(ref, ids, obj, 0, K, dist, 0.039)
        assert b["has_pose"] == 1 and ob["has_pose"] == 1 and abs(b["prob"] - 1.0) < 1e-6 and abs(ob["prob"] - 1.0) < 1e-6
        assert [int(m["id"]) for m in b["markers"]] == [m["id"] for m in ob["markers"]]
        assert rel_err(b["rvec"], ob["rvec"]) < POSE_REL_TOL and rel_err(b["tvec"], ob["tvec"]) < POSE_REL_TOL
        # the same board in metres (aruco_board_pix2meters) gives the same pose
        bm = det.board_detect(got, ids, capi.board_pix_to_meters(obj, 0.039), 1, K, dist, 0.039)
        om = orc.board_detect(ref, ids, fr.pix_to_meters(obj, 0.039), 1, K, dist, 0.039)
        assert rel_err(bm["rvec"], om["rvec"]) < POSE_REL_TOL and rel_err(bm["tvec"], om["tvec"]) < POSE_REL_TOL
    finally:
        det.close()


def test_detect_graph_after_fiducial_calls(monkeypatch):
    """detect x3 (the third replays the single-frame graph), a generator call of each kind, detect: equal to an ARUCOHIP_GRAPH=0 handle's bytes"""
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
            m = h.fiducial_marker_images(np.arange(0, 1024, 7), 150, True)
            seq.append(h.detect(gray))
            b = h.fiducial_board_image(fr.FRAME, (6, 5), 120, 24, np.arange(100, 200))
            seq.append(h.detect(gray))
            d = h.fiducial_distances()
            s = h.fiducial_select(24)
            seq.append(h.detect(gray))
            outs.append((seq, m, b[0], d, s[0]))
        (sg, *rg), (se, *re_) = outs
        for a, b in zip(sg, se):
            assert len(a) > 0 and np.asarray(a).tobytes() == np.asarray(b).tobytes()
        for a, b in zip(rg, re_):
            assert a.tobytes() == b.tobytes()
    finally:
        graphed.close()
        eager.close()


def fnv1a(img):
    h = 1469598103934665603
    for v in img.tobytes():
        h = ((h ^ v) * 1099511628211) & 0xFFFFFFFFFFFFFFFF
    return "%x" % h


def test_shim_fiducial_create(tmp_path, doc):
    """tests/cpp/shim_fiducial_create.cpp: the reference's CreateMarker / CreateBoard sequences through the shim"""
    from aruco_amd import build_library

    build_library()
    exe = str(tmp_path / "shim_fiducial_create")
    subprocess.run(["g++", "-std=c++11", "-O1", "-Wall", "-Wextra", "-Werror", "-I" + os.path.join(ROOT, "include"),
                    os.path.join(ROOT, "tests", "cpp", "shim_fiducial_create.cpp"), "-o", exe, "-L" + os.path.join(ROOT, "aruco_amd"), "-larucohip",
                    "-L/opt/rocm/lib", "-Wl,-rpath," + os.path.join(ROOT, "aruco_amd"), "-Wl,-rpath,/opt/rocm/lib"], check=True)
    out = subprocess.run([exe], stdout=subprocess.PIPE, text=True, check=True, timeout=300).stdout
    res = json.loads(out.strip().splitlines()[-1])
    assert res["marker"] == {"side": 500, "digest": fnv1a(doc["images"]["marker"])}
    assert res["locked"] == {"side": 750, "digest": fnv1a(doc["images"]["locked_marker"])}
    assert res["watermark_arg"] == res["marker"]["digest"] and res["default_side"] == 70
    assert res["cells"] == int(fr.marker_mat(471).sum())
    for name, btype, dist in CREATE_BOARD:
        want, got = doc["boards"][name], res[name]
        assert got["ids"] == want["ids"] and got["info_type"] == 0, name
        assert np.array(got["obj"], np.float32).tobytes() == np.array(want["obj"], np.float32).tobytes(), name
        img = fr.board_image(btype, 5, 5, 100, dist, want["ids"])[0]
        assert got["shape"] == list(img.shape) and got["digest"] == fnv1a(img), name
    assert res["appended"] and res["pixels"] and res["bad_id_throws"]
