"""MarkerDetector::pyrDown(level) on the device: pyr_down_kernel bit for bit against the integer definition (tests/pyr_ref.py), and detection
on the reduced image against the reference chain composed from the oracle's stage functions (pyr_ref.chain)."""
import ctypes as C

import numpy as np
import pytest

from tests import pyr_ref
from tests.util import rel_err

pytestmark = pytest.mark.gpu

SHAPES = [(1, 1), (2, 3), (3, 2), (4, 5), (5, 5), (7, 6), (33, 17), (130, 67), (257, 129), (1023, 9), (640, 480)]   # W x H
CAP = 64


@pytest.fixture(scope="module")
def env():
    import torch
    from aruco_amd import capi
    from oracle import orc

    assert torch.cuda.is_available()
    capi.load()
    return {"capi": capi, "orc": orc, "torch": torch}


@pytest.fixture(scope="module")
def kh(env):
    h = env["capi"].Handle(1024, 512, max_batch=3)
    yield h
    h.close()


@pytest.fixture(scope="module")
def handles(env):
    hs = {name: env["capi"].Handle(v[0], v[1], max_batch=3) for name, v in pyr_ref.FRAME_SETS.items()}
    yield hs
    for h in hs.values():
        h.close()


def _padded(rng, n, W, H, row_stride, frame_stride):
    """n random frames inside a buffer of 255s (row and frame padding), and the frames themselves."""
    buf = np.full(n * frame_stride, 255, np.uint8)
    frames = rng.randint(0, 256, size=(n, H, W)).astype(np.uint8)
    for f in range(n):
        for y in range(H):
            at = f * frame_stride + y * row_stride
            buf[at:at + W] = frames[f, y]
    return buf, frames


def _pyr(env, h, buf, n, W, H, rs, fs, levels, on_device):
    """arucohip_pyr_down of the frames in buf, from host memory to host memory or from device memory to device memory."""
    torch = env["torch"]
    wo, ho = W, H
    for _ in range(levels):
        wo, ho = (wo + 1) // 2, (ho + 1) // 2
    if not on_device:
        out = np.zeros((n, ho, wo), np.uint8)
        h._chk(h.L.arucohip_pyr_down(h.h, buf.ctypes.data_as(C.c_void_p), n, W, H, rs, fs, 0, levels, out.ctypes.data_as(C.c_void_p), 0))
        return out
    src = torch.from_numpy(buf).cuda()
    dst = torch.zeros((n, ho, wo), dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    h._chk(h.L.arucohip_pyr_down(h.h, C.c_void_p(src.data_ptr()), n, W, H, rs, fs, 1, levels, C.c_void_p(dst.data_ptr()), 1))
    h.synchronize()
    return dst.cpu().numpy()


@pytest.mark.parametrize("levels", [1, 2, 3])
@pytest.mark.parametrize("shape", SHAPES, ids=["%dx%d" % s for s in SHAPES])
def test_kernel_bit_exact(env, kh, shape, levels):
    """Random bytes, tightly packed rows and rows padded with 255 to a multiple of 8 (the 8-byte loads), host and device input."""
    W, H = shape
    rng = np.random.RandomState(W * 1000 + H + levels)
    for rs in (W, (W + 7) // 8 * 8 + 8):
        buf, frames = _padded(rng, 1, W, H, rs, rs * H + 16)
        exp = pyr_ref.pyr_down_levels(frames[0], levels)
        for on_device in (False, True):
            got = _pyr(env, kh, buf, 1, W, H, rs, rs * H + 16, levels, on_device)
            assert got.shape[1:] == exp.shape
            assert np.array_equal(got[0], exp), (rs, on_device)


@pytest.mark.parametrize("levels", [1, 2, 3])
def test_kernel_strided_batch(env, kh, levels):
    """3 frames of 130 x 67 with row_stride 144 and a padded frame stride; the padding holds 255, so a read past `width` shows."""
    W, H, rs = 130, 67, 144
    fs = rs * H + 64
    buf, frames = _padded(np.random.RandomState(5 + levels), 3, W, H, rs, fs)
    exp = np.stack([pyr_ref.pyr_down_levels(frames[f], levels) for f in range(3)])
    for on_device in (False, True):
        assert np.array_equal(_pyr(env, kh, buf, 3, W, H, rs, fs, levels, on_device), exp), on_device
    assert np.array_equal(kh.pyr_down_image(frames, levels), exp)
    assert np.array_equal(kh.pyr_down_image(frames[1], levels), exp[1])


def _same(got, exp, pose=False):
    """ids and order exact; corners (and poses) at the project's standing tolerance for device float32 against the restatement
    (tests/test_gpu_fullsize.py)."""
    assert [int(m["id"]) for m in got] == [m["id"] for m in exp]
    for a, b in zip(got, exp):
        ca, cb = np.asarray(a["corners"], float).reshape(4, 2), np.asarray(b["corners"], float).reshape(4, 2)
        assert np.max(np.abs(ca - cb) / np.maximum(np.abs(cb), 1.0)) < 1e-4
        if pose:
            assert int(a["has_pose"]) == 1 and b["has_pose"] == 1
            assert rel_err(a["rvec"], b["rvec"]) < 1e-4 and rel_err(a["tvec"], b["tvec"]) < 1e-4


@pytest.mark.parametrize("level", [1, 2])
@pytest.mark.parametrize("name", ["640x480", "1280x720"])
def test_detection_equals_the_chain(handles, name, level):
    frames, truth = pyr_ref.frames_of(name)
    h = handles[name]
    h.set_pyr_down(level)
    try:
        assert h.pyr_down == level
        batch = h.detect_batch_host(frames, cap=CAP)
        for f in range(3):
            exp, _ = pyr_ref.chain_cached(name, f, level)
            assert len(exp) == len(truth[f]) == pyr_ref.FRAME_SETS[name][2]
            _same(h.detect(frames[f], cap=CAP), exp)
            _same(batch[f], exp)
    finally:
        h.set_pyr_down(0)


def test_detection_with_camera(handles):
    frames, truth = pyr_ref.frames_of("640x480")
    h = handles["640x480"]
    h.set_pyr_down(1)
    try:
        cam = dict(K=pyr_ref.CAM_K, dist=pyr_ref.CAM_DIST, marker_size=pyr_ref.CAM_SIZE)
        batch = h.detect_batch_host(frames, cap=CAP, **cam)
        for f in range(3):
            exp, _ = pyr_ref.chain_cached("640x480", f, 1, cam=True)
            assert len(exp) == len(truth[f])
            _same(h.detect(frames[f], cap=CAP, **cam), exp, pose=True)
            _same(batch[f], exp, pose=True)
    finally:
        h.set_pyr_down(0)


def test_subpix_runs_on_the_full_frame(env):
    """SUBPIX at level 1 against chain(corner_method=SUBPIX), at the tolerance of test_corner_methods_vs_oracle[SUBPIX] (1e-4 relative)."""
    capi = env["capi"]
    frames, truth = pyr_ref.frames_of("640x480")
    p = capi.default_params()
    p.corner_method = 2
    h = capi.Handle(640, 480, params=p)
    try:
        h.set_pyr_down(1)
        exp, _ = pyr_ref.chain_cached("640x480", 0, 1, corner_method=pyr_ref.SUBPIX)
        assert len(exp) == len(truth[0])
        _same(h.detect(frames[0], cap=CAP), exp)
    finally:
        h.close()


@pytest.mark.parametrize("level", [1, 2])
def test_getters_report_full_frame_coordinates(env, handles, level):
    orc = env["orc"]
    frames, _ = pyr_ref.frames_of("640x480")
    h = handles["640x480"]
    s = 1 << level
    h.set_pyr_down(level)
    try:
        h.detect(frames[0], cap=CAP)
        _, d = pyr_ref.chain_cached("640x480", 0, level)
        reduced = pyr_ref.pyr_down_levels(frames[0], level)
        assert np.array_equal(h.thresholded(0, shape=reduced.shape), orc.adaptive_threshold(reduced, 7, 7.0))
        q, ids, _ = h.debug_candidates(0)
        assert len(q) == len(d["quads"]) > 0
        assert [int(i) for i in ids] == d["ids"]
        for a, b in zip(q, d["quads"]):
            assert np.array_equal(a, b)
        rejected = [b for b, i in zip(d["quads"], d["ids"]) if i == -1]
        cand = h.candidates(0)
        assert len(cand) == len(rejected)
        for a, b in zip(cand, rejected):
            assert np.array_equal(a, b)
        cs = h.debug_contours(0)
        assert len(cs) > 0
        for c in cs:
            assert np.all(c["pts"] % s == 0) and c["start"][0] % s == 0 and c["start"][1] % s == 0
            assert c["pts"][:, 0].max() < 640 and c["pts"][:, 1].max() < 480
    finally:
        h.set_pyr_down(0)


def test_level_zero_is_the_path_without_the_option(env):
    """A handle whose level went to 1 and back returns the bytes of a fresh handle, batch and single frame (three calls each, so that the
    one-frame graph of both is captured and replayed; the library has no query for the path a call took, so bytes are what is compared)."""
    capi = env["capi"]
    frames, _ = pyr_ref.frames_of("640x480")
    fresh, back = capi.Handle(640, 480, max_batch=3), capi.Handle(640, 480, max_batch=3)
    try:
        back.set_pyr_down(1)
        back.detect(frames[0], cap=CAP)
        back.detect_batch_host(frames, cap=CAP)
        back.set_pyr_down(0)
        assert back.pyr_down == 0
        for a, b in zip(fresh.detect_batch_host(frames, cap=CAP), back.detect_batch_host(frames, cap=CAP)):
            assert len(a) > 0 and a.tobytes() == b.tobytes()
        for _ in range(3):
            for f in range(3):
                a, b = fresh.detect(frames[f], cap=CAP), back.detect(frames[f], cap=CAP)
                assert len(a) > 0 and a.tobytes() == b.tobytes()
    finally:
        fresh.close(), back.close()


def test_batches_in_flight_take_the_level(env):
    capi = env["capi"]
    frames, _ = pyr_ref.frames_of("640x480")
    frames = np.ascontiguousarray(frames)
    h = capi.Handle(640, 480, max_batch=3)
    try:
        h.set_pyr_down(1)
        h.set_pipeline_depth(2)        # the lanes inherit the level
        for level in (1, 2):
            h.set_pyr_down(level)      # the second time: lanes that exist take it
            sync = h.detect_batch_host(frames, cap=CAP)
            outs = [np.zeros((3, CAP), capi.MARKER_DTYPE) for _ in range(2)]
            ns = [np.zeros(3, np.int32) for _ in range(2)]
            tickets = [h.submit_host(frames, outs[i], ns[i]) for i in range(2)]
            for t in tickets:
                h.wait(t)
            for i in range(2):
                for f in range(3):
                    assert ns[i][f] == len(sync[f]) > 0
                    assert outs[i][f, :ns[i][f]].tobytes() == sync[f].tobytes()
    finally:
        h.close()


def test_bgr_reduces_the_converted_gray_image(handles):
    frames, truth = pyr_ref.frames_of("640x480")
    h = handles["640x480"]
    h.set_pyr_down(1)
    try:
        gray = h.detect(frames[0], cap=CAP)
        bgr = h.detect_bgr(np.repeat(frames[0][:, :, None], 3, axis=2), cap=CAP)   # equal channels convert to the gray value itself
        assert [int(m["id"]) for m in bgr] == truth[0]
        assert bgr.tobytes() == gray.tobytes()
    finally:
        h.set_pyr_down(0)


def test_levels_outside_0_to_3_are_refused(env, handles):
    capi = env["capi"]
    h = handles["640x480"]
    h.set_pyr_down(2)
    try:
        for bad in (-1, 4):
            assert h.L.arucohip_set_pyr_down(h.h, bad) == capi.E_INVALID
            assert h.pyr_down == 2
            with pytest.raises(capi.ArucoHipError):
                h.set_pyr_down(bad)
    finally:
        h.set_pyr_down(0)
    assert h.pyr_down == 0
