"""Board occlusion mask on the device (arucohip_chromatic_*, k_chromatic.hip) against the NumPy restatement (tests/chromatic_ref.py):
geometry, cell maps, histograms, the EM, classify / classify2 masks, update, the quirk cases, determinism, the batched path over
one and four chunks, the single-frame graph after chromatic calls, and the errors."""
import math

import numpy as np
import pytest

from tests import chromatic_ref as cr
from tests.test_chromatic_cpu import scene

pytestmark = pytest.mark.gpu

SIZES = [(640, 480), (1920, 1080)]


def rel(a, b):
    a, b = np.asarray(a, float), np.asarray(b, float)
    return np.max(np.abs(a - b) / np.maximum(np.abs(b), 1e-300))


def model_close(a, b):
    """1e-12 relative, scaled by |ln p| far in the tails: exp turns an ulp of the log-likelihood into |ln p| ulps of p, and the
    device's exp / log need not round as the host libm does"""
    a, b = np.asarray(a, float), np.asarray(b, float)
    tol = 1e-12 * np.maximum(1.0, np.abs(np.log(np.maximum(b, 1e-320)))) * np.abs(b)
    return bool(np.all(np.abs(a - b) <= tol))


@pytest.fixture(scope="module")
def handle():
    import torch  # noqa: F401
    from aruco_amd import capi

    h = capi.Handle(640, 480, max_batch=1)
    yield h
    h.close()


def make(handle, sc, W, H, mc=6, thresh=1e-4):
    return handle.chromatic(mc, mc, thresh, sc["K"], None, W, H, sc["corners"])


def ref_with(dev, sc, W, H, mc=6, thresh=1e-4):
    """a restatement object that holds the device's model"""
    m = cr.ChromaticMask(mc, mc, thresh, sc["K"], None, W, H, sc["corners"])
    m.prob, m.trained = [np.array(x) for x in dev.get_model()]
    return m


@pytest.mark.parametrize("W,H", SIZES)
def test_train_classify_update_equal_restatement(handle, W, H):
    sc = scene(W, H)
    dev = make(handle, sc, W, H)
    try:
        r, t = sc["rvec"], sc["tvec"]
        dev.train(sc["img"], r, t)
        assert dev.is_valid()
        c2, Ht, Hc = dev.debug_geometry()
        rc2, rHt, rHc, rrect = sc["m"].geometry(r, t)
        assert rel(c2, rc2) < 1e-6 and rel(Ht, rHt) < 1e-9 and rel(Hc, rHc) < 1e-9
        # with the device's H: the cell map, the raw and discretised histograms and the < 10 outcomes are exact
        cmap = cr.cell_map(Ht, 6, 6, W, H)
        assert np.array_equal(dev.cell_map(), cmap)
        raw, hc, fitted = dev.debug_hist()
        assert np.array_equal(raw, cr.raw_hist(cmap, sc["img"], 36))
        prob, trained = dev.get_model()
        for i in range(36):
            p, _, ok, c = cr.em_fit(raw[i], 1e-4)
            assert np.array_equal(hc[i], c) and fitted[i] == (1 if ok else 0) and trained[i] == ok
            assert model_close(prob[i], p), i
        # with the device's model: classify and classify2 masks byte for byte
        ref = ref_with(dev, sc, W, H)
        m1 = dev.classify(sc["occ"], r, t, method=1)
        assert np.array_equal(m1, cr.classify(cr.cell_map(dev.debug_geometry()[1], 6, 6, W, H), ref.prob > 1e-4, sc["occ"]))
        m2 = dev.classify(sc["occ"], r, t, method=2)
        _, _, Hc2 = dev.debug_geometry()
        assert np.array_equal(m2, cr.classify2(Hc2, cr.rect(dev.debug_geometry()[0], W, H), ref.prob, sc["occ"], 6, 6, 1e-4))
        assert 1 - m2[sc["occ_in"]].mean() >= 0.99 and m2[sc["visible"]].mean() >= 0.75
        # update: the last cell map (train's) times classify2's mask
        ref.cellmap, ref.mask = dev.cell_map(), m2
        rraw, (rfit, rcnt) = ref.update(sc["occ"])
        dev.update(sc["occ"])
        raw, hc, fitted = dev.debug_hist()
        assert np.array_equal(raw, rraw) and np.array_equal(fitted, rfit)
        prob, _ = dev.get_model()
        assert model_close(prob, ref.prob)
    finally:
        dev.close()


def test_quirk_cases(handle):
    """odd frame size (last row / column of the cell map stay 0), empty neighbour lists (first row / column never set), a pixel that
    truncates to cell 0 from outside (point in (-1, -0.5))"""
    W, H = 641, 481
    sc = scene(640, 480, rvec=(0.1, -0.15, 0.6))   # rotated in the image plane: the bounding rectangle reaches past the cells
    img = np.zeros((H, W), np.uint8)
    img[:480, :640] = sc["occ"]
    dev = make(handle, sc, W, H)
    try:
        dev.train(img, sc["rvec"], sc["tvec"])
        cm = dev.cell_map()
        c2, Ht, Hc = dev.debug_geometry()
        assert np.array_equal(cm, cr.cell_map(Ht, 6, 6, W, H)) and not cm[480].any() and not cm[:, 640].any()
        ref = ref_with(dev, sc, W, H)
        sparse, det = cr.classify2_samples(Hc, cr.rect(c2, W, H), ref.prob, img, 6, 6, 1e-4)
        assert (det["ok"] & ~det["full"]).any()                                   # samples with an empty neighbour list
        assert (det["ok"] & ((det["px"] < -0.5) | (det["py"] < -0.5))).any()       # truncated to cell 0 from outside
        assert not det["set"][~det["full"]].any()
        m2 = dev.classify(img, sc["rvec"], sc["tvec"], method=2)
        assert np.array_equal(m2, cr.close3(sparse))
        a = dev.classify(img, sc["rvec"], sc["tvec"], method=1)
        b = dev.classify(img, sc["rvec"], sc["tvec"], method=1)
        assert a.tobytes() == b.tobytes()
    finally:
        dev.close()


@pytest.mark.parametrize("shift", [(-260, 0), (0, -200)], ids=["left_edge", "top_edge"])
def test_board_across_the_frame_edge(handle, shift):
    """fitRectToSize clamps the start to 0 and keeps the width: for a board cut by the left (top) edge classify2 scans as many
    columns (rows) past the board's right (bottom) end as the rectangle started outside the frame"""
    W, H = 640, 480
    sc = scene(W, H)
    K = sc["K"].copy()
    K[0, 2] += shift[0]
    K[1, 2] += shift[1]
    dev = handle.chromatic(6, 6, 1e-4, K, None, W, H, sc["corners"])
    try:
        dev.train(sc["img"], sc["rvec"], sc["tvec"])
        m2 = dev.classify(sc["img"], sc["rvec"], sc["tvec"], 2)
        c2, _, Hc = dev.debug_geometry()
        rc = cr.rect(c2, W, H)
        bx0, by0 = math.floor(float(c2[:, 0].min())), math.floor(float(c2[:, 1].min()))
        bx1, by1 = math.floor(float(c2[:, 0].max())) + 1, math.floor(float(c2[:, 1].max())) + 1
        assert (bx0 < 0 and rc[0] == 0 and rc[2] == min(bx1 - bx0, W)) or (by0 < 0 and rc[1] == 0 and rc[3] == min(by1 - by0, H))
        assert rc[2] > bx1 or rc[3] > by1   # the extra strip exists
        ref = ref_with(dev, sc, W, H)
        sparse, det = cr.classify2_samples(Hc, rc, ref.prob, sc["img"], 6, 6, 1e-4)
        past = (det["x"] >= bx1) | (det["y"] >= by1)
        assert past.any() and det["ok"][past].any()   # samples in the strip reach cells
        if shift[1]:
            assert det["set"][past].any()   # and, for this pose, set pixels there
        assert np.array_equal(m2, cr.close3(sparse))
    finally:
        dev.close()


def test_em_fit_equals_restatement(handle):
    rng = np.random.RandomState(9)
    s = np.concatenate([rng.normal(60, 5, 500), rng.normal(170, 9, 700)]).round().clip(0, 255).astype(int)
    raw = np.bincount(s, minlength=256)
    p, inside, ok = handle.em_fit(raw, 1e-4)
    rp, rin, rok, _ = cr.em_fit(raw, 1e-4)
    assert ok and rok and model_close(p, rp) and np.array_equal(inside, p > 1e-4)
    prev = np.linspace(0, 1, 256)
    p, _, ok = handle.em_fit(np.zeros(256), 0.5, prev)
    assert not ok and np.array_equal(p, prev)


def test_deterministic(handle):
    sc = scene(640, 480)
    outs = []
    for _ in range(2):
        dev = make(handle, sc, 640, 480)
        dev.train(sc["img"], sc["rvec"], sc["tvec"])
        m2 = dev.classify(sc["occ"], sc["rvec"], sc["tvec"], 2)
        dev.update(sc["occ"])
        outs.append((dev.get_model()[0].tobytes(), m2.tobytes(), dev.cell_map().tobytes()))
        dev.close()
    assert outs[0] == outs[1]


def occluded_stream(n, W, H, K, bc, seed):
    """board frames (make_board_stream poses) with a flat grey occluder on about a quarter of them"""
    import torch
    from aruco_amd import synth

    frames, poses = synth.make_board_stream(n, bc["ids"], bc["obj"], K.reshape(-1), width=W, height=H, seed=seed, device="cuda")
    torch.cuda.synchronize()
    host = frames.cpu().numpy()
    rng = np.random.RandomState(seed)
    for f in range(n):
        if rng.rand() < 0.25:
            x0, y0 = rng.randint(W // 3, W // 2), rng.randint(H // 3, H // 2)
            host[f, y0:y0 + H // 8, x0:x0 + W // 8] = 128
    return host, poses


@pytest.mark.parametrize("streams", [1, 4], ids=["one_chunk", "four_chunks"])
def test_classify_batch_equals_single_frame(monkeypatch, streams):
    import torch
    from aruco_amd import capi

    W, H, NB = 1920, 1080, 1024
    sc = scene(640, 480)
    bc = sc["board"]
    K = np.array([[1700.0, 0, 955.0], [0, 1690.0, 545.0], [0, 0, 1]], np.float32)
    host, poses = occluded_stream(NB, W, H, K, bc, seed=31)
    monkeypatch.setenv("ARUCOHIP_STREAMS", str(streams))
    h = capi.Handle(W, H, max_batch=NB)
    monkeypatch.delenv("ARUCOHIP_STREAMS")
    try:
        h.detect_batch_host(host)
        if streams > 1:
            assert h.batch_chunks()[0] == streams
        boards = h.board_detect_batch(NB, bc["ids"], bc["obj"], bc["info_type"], K=K, marker_size=0.039)
        dev = h.chromatic(6, 6, 1e-4, K, None, W, H, sc["corners"])
        f0 = next(f for f in range(NB) if boards[f]["has_pose"] and boards[f]["prob"] > 0.9)
        dev.train(host[f0], boards[f0]["rvec"], boards[f0]["tvec"])
        min_prob = 0.9
        masks, npix = dev.classify_batch(h, host, method=2, min_prob=min_prob)
        assert np.array_equal(npix, masks.reshape(NB, -1).sum(axis=1))
        fd = torch.from_numpy(host).cuda()
        md = torch.zeros((NB, H, W), dtype=torch.uint8, device="cuda")
        dev.classify_batch_device(h, fd.data_ptr(), NB, W, W * H, md.data_ptr(), method=2, min_prob=min_prob)
        torch.cuda.synchronize()
        assert np.array_equal(md.cpu().numpy(), masks)
        m1, _ = dev.classify_batch(h, host, method=1, min_prob=min_prob, npix=False)
        live = 0
        for f in range(NB):
            b = boards[f]
            if b["has_pose"] and b["prob"] > min_prob:
                live += 1
                assert np.array_equal(masks[f], dev.classify(host[f], b["rvec"], b["tvec"], 2)), f
                assert np.array_equal(m1[f], dev.classify(host[f], b["rvec"], b["tvec"], 1)), f
            else:
                assert not masks[f].any() and not m1[f].any()
        assert live > 50
        assert any(not (b["has_pose"] and b["prob"] > min_prob) for b in boards) or min_prob < 0
        dev.close()
    finally:
        h.close()


def test_detect_graph_after_chromatic(monkeypatch):
    """detect x3 (the third replays the single-frame graph), chromatic calls that allocate, detect: every result equals an
    ARUCOHIP_GRAPH=0 handle's byte for byte."""
    from aruco_amd import capi
    from tests.util import load_case

    gray, _ = load_case("board")
    sc = scene(640, 480)
    monkeypatch.setenv("ARUCOHIP_GRAPH", "0")
    eager = capi.Handle(640, 480, max_batch=4)
    monkeypatch.delenv("ARUCOHIP_GRAPH")
    graphed = capi.Handle(640, 480, max_batch=4)
    try:
        outs = []
        for h in (graphed, eager):
            seq = [h.detect(gray) for _ in range(3)]
            m = h.chromatic(6, 6, 1e-4, sc["K"], None, 640, 480, sc["corners"])
            m.train(sc["img"], sc["rvec"], sc["tvec"])
            mk = m.classify(sc["occ"], sc["rvec"], sc["tvec"], 2)
            seq.append(h.detect(gray))
            m.close()
            seq.append(h.detect(gray))
            outs.append((seq, mk))
        (sg, mg), (se, me) = outs
        for a, b in zip(sg, se):
            assert len(a) > 0 and np.asarray(a).tobytes() == np.asarray(b).tobytes()
        assert mg.tobytes() == me.tobytes()
    finally:
        graphed.close()
        eager.close()


def test_errors(handle):
    import ctypes as C

    from aruco_amd import capi

    sc = scene(640, 480)
    L, hh = handle.L, handle.h
    K = np.ascontiguousarray(sc["K"].reshape(9))
    cor = np.ascontiguousarray(sc["corners"].reshape(12))
    p = lambda a: None if a is None else a.ctypes.data_as(C.c_void_p)
    out = C.c_void_p()

    def create(mc=6, nc=6, Kp=K, W=640, H=480, cp=cor):
        return L.arucohip_chromatic_create(hh, mc, nc, 1e-4, p(Kp), None, 0, W, H, p(cp), C.byref(out))

    assert create(nc=7) == capi.E_UNSUPPORTED
    assert create(mc=16, nc=16) == capi.E_UNSUPPORTED
    assert create(mc=0) == capi.E_UNSUPPORTED and create(nc=0) == capi.E_UNSUPPORTED
    assert create(Kp=None) == capi.E_INVALID and create(cp=None) == capi.E_INVALID and create(W=0) == capi.E_INVALID
    assert L.arucohip_chromatic_create(hh, 6, 6, 1e-4, p(K), None, 0, 640, 480, p(cor), None) == capi.E_INVALID
    m = handle.chromatic(6, 6, 1e-4, sc["K"], None, 640, 480, sc["corners"])
    try:
        r, t = np.zeros(3), np.array([0, 0, 0.5])
        img = np.zeros((480, 640), np.uint8)
        assert L.arucohip_chromatic_classify(m.m, p(img), 0, 640, p(r), p(t), 3) == capi.E_INVALID
        assert L.arucohip_chromatic_classify(m.m, p(img), 0, 640, p(r), p(t), 0) == capi.E_INVALID
        assert L.arucohip_chromatic_train(m.m, None, 0, 640, p(r), p(t)) == capi.E_INVALID
        assert L.arucohip_chromatic_train(m.m, p(img), 0, 640, None, p(t)) == capi.E_INVALID
        assert L.arucohip_chromatic_train(m.m, p(img), 0, 320, p(r), p(t)) == capi.E_INVALID
        assert L.arucohip_chromatic_get_mask(m.m, None, 0) == capi.E_INVALID
        frames = np.zeros((2, 480, 640), np.uint8)
        masks = np.zeros((2, 480, 640), np.uint8)
        # no board batch on this handle
        assert L.arucohip_chromatic_classify_batch(m.m, hh, p(frames), 2, 640, 480, 640, 640 * 480, 0, 2, 0.0, p(masks), 0, None) == capi.E_INVALID
        # a board batch of 1 frame, then a call for 2, a wrong size and a wrong method
        h2 = capi.Handle(640, 480, max_batch=2)
        try:
            h2.detect_batch_host(np.stack([sc["img"], sc["img"]]))
            bc = sc["board"]
            h2.board_detect_batch(1, bc["ids"], bc["obj"], bc["info_type"], K=sc["K"], marker_size=0.039)
            call = lambda n=2, W=640, method=2: L.arucohip_chromatic_classify_batch(m.m, h2.h, p(frames), n, W, 480, 640, 640 * 480, 0, method,
                                                                                   0.0, p(masks), 0, None)
            assert call(n=2) == capi.E_INVALID
            assert call(n=1, W=320) == capi.E_INVALID and call(n=1, method=0) == capi.E_INVALID
            assert call(n=1) == capi.OK
            # a single-frame detect replaces the lists: the board poses no longer belong to the last detection
            h2.detect(sc["img"])
            assert call(n=1) == capi.E_INVALID
            h2.detect_batch_host(np.stack([sc["img"], sc["img"]]))
            assert call(n=1) == capi.E_INVALID
        finally:
            h2.close()
        assert L.arucohip_chromatic_classify_batch(m.m, hh, None, 1, 640, 480, 640, 640 * 480, 0, 2, 0.0, p(masks), 0, None) == capi.E_INVALID
    finally:
        m.close()
    assert L.arucohip_chromatic_board_corners(None, 1, 0, 0.039, p(np.zeros(12, np.float32))) == capi.E_INVALID
    m = handle.chromatic(6, 6, 1e-4, sc["K"], None, 640, 480, sc["corners"])
    with pytest.raises(ValueError):
        m.classify_batch(handle, np.zeros((2, 240, 320), np.uint8))
    m.close()


def test_shim_chromatic_equals_c_abi(tmp_path):
    """the reference's call sequence through the shim (setParams(BC, markersize), train, classify2, getMask, update, classify2,
    getMask, getCellMap) gives the masks and cell map of the same calls through the Python C ABI binding"""
    import os
    import subprocess

    from aruco_amd import build_library, capi

    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    build_library()
    exe = str(tmp_path / "shim_chromatic")
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-I" + os.path.join(root, "include"), os.path.join(root, "tests", "cpp", "shim_chromatic.cpp"),
                    "-o", exe, "-L" + os.path.join(root, "aruco_amd"), "-larucohip", "-L/opt/rocm/lib", "-Wl,-rpath," + os.path.join(root, "aruco_amd"),
                    "-Wl,-rpath,/opt/rocm/lib"], check=True)
    W, H = 640, 480
    sc = scene(W, H)
    bc = sc["board"]
    obj = np.asarray(bc["obj"], np.float32).reshape(-1, 12)
    lines = ["%d %d" % (W, H), " ".join("%.9g" % v for v in sc["K"].reshape(9)), " ".join(repr(float(v)) for v in sc["rvec"]),
             " ".join(repr(float(v)) for v in sc["tvec"]), "6 6 0.0001 0.039 %d %d" % (bc["info_type"], len(obj))]
    lines += [" ".join("%.9g" % v for v in row) for row in obj]
    (tmp_path / "in.txt").write_text("\n".join(lines) + "\n")
    sc["img"].tofile(str(tmp_path / "frame.raw"))
    sc["occ"].tofile(str(tmp_path / "occ.raw"))
    out = subprocess.run([exe, str(tmp_path / "in.txt"), str(tmp_path / "frame.raw"), str(tmp_path / "occ.raw"), str(tmp_path / "out.raw")],
                         stdout=subprocess.PIPE, text=True, check=True).stdout.split()
    got = np.fromfile(str(tmp_path / "out.raw"), np.uint8).reshape(3, H, W)
    h = capi.Handle(W, H)
    try:
        m = h.chromatic(6, 6, 1e-4, sc["K"], np.zeros(5, np.float32), W, H, capi.chromatic_board_corners(bc["obj"], bc["info_type"], 0.039))
        m.train(sc["img"], sc["rvec"], sc["tvec"])
        a = m.classify(sc["occ"], sc["rvec"], sc["tvec"], 2)
        m.update(sc["occ"])
        b = m.classify(sc["occ"], sc["rvec"], sc["tvec"], 2)
        assert np.array_equal(got[0], a) and np.array_equal(got[1], b) and np.array_equal(got[2], m.cell_map())
        assert a.any() and got[2].any()
        m.close()
        # EMClassifier through the shim: 300 samples around 42 and 203
        assert out[0] == "300" and out[1] == "1" and out[2] == "0" and float(out[3]) > 1e-4
    finally:
        h.close()
