"""Board occlusion mask (ChromaticMask): the NumPy restatement's quirks against hand-written expectations, the EM definition, an
occluded rendered board, and the C ABI symbols. No GPU."""
import ctypes as C
import json
import math
import os

import numpy as np
import pytest

from tests import chromatic_ref as cr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("mc,nc", [(2, 2), (3, 2), (5, 4), (6, 6)])
def test_neighbour_lists(mc, nc):
    # the unsigned loops leave i == 0 or j == 0 empty; every other cell lists (i-1,j-1) (i,j-1) (i-1,j) (i,j)
    want = []
    for j in range(nc):
        for i in range(mc):
            want.append([] if i == 0 or j == 0 else [(j - 1) * mc + i - 1, (j - 1) * mc + i, j * mc + i - 1, j * mc + i])
    assert cr.neighbour_lists(mc, nc) == want
    if (mc, nc) == (3, 2):
        assert cr.neighbour_lists(3, 2) == [[], [], [], [], [0, 1, 3, 4], [1, 2, 4, 5]]


def test_cell_number_uses_nc():
    # an identity-scaled transform: block (x, y) maps to cell (x / 20, y / 20); the cell number is y * nc + x, not y * mc + x
    mc, nc, W, H = 5, 3, 100, 60
    Ht = np.eye(3)
    cm = cr.cell_map(Ht, mc, nc, W, H)
    for cy in range(nc):
        for cx in range(mc):
            assert cm[20 * cy + 4, 20 * cx + 4] == 1 + cy * nc + cx
    # odd frame: the last row and column are never written
    cm = cr.cell_map(Ht, mc, nc, 61, 41)
    assert not cm[40].any() and not cm[:, 60].any() and cm[38, 58] != 0


def test_histogram_discretisation():
    raw = np.zeros(256, np.int64)
    raw[0], raw[100], raw[255] = 4, 10, 1
    r = raw.copy()
    h = np.zeros(256)
    for v in range(256):
        for _ in range(r[v]):
            h[v] += 3
            if v > 0:
                h[v - 1] += 2
            if v < 255:
                h[v + 1] += 2
            if v > 1:
                h[v - 2] += 1
            if v < 254:
                h[v + 2] += 1
    want = np.array([int(200 * (x / h.sum())) for x in h])
    assert np.array_equal(cr.hist_count(raw), want)
    assert cr.hist_count(np.zeros(256, np.int64)).sum() == 0


def test_fewer_than_10_samples_keep_the_model():
    # the discretisation is of the normalised histogram: a narrow cell keeps close to 200 samples, a flat one loses them all to the
    # truncation (200 * 9 / 2304 < 1 per level) and the previous model stays, as does the model of a cell without samples
    raw = np.zeros(256, np.int64)
    raw[[10, 200]] = 1
    assert 150 <= cr.hist_count(raw).sum() <= 200
    prev = np.linspace(0, 1, 256)
    for raw in (np.ones(256, np.int64), np.zeros(256, np.int64)):
        p, inside, fitted, c = cr.em_fit(raw, 0.3, prev)
        assert c.sum() < 10 and not fitted and np.array_equal(p, prev) and np.array_equal(inside, prev > 0.3)


def test_update_rule_more_than_50_samples():
    K = np.array([[500.0, 0, 80], [0, 500, 60], [0, 0, 1]], np.float32)
    corners = np.array([[-0.1, -0.1, 0], [-0.1, 0.1, 0], [0.1, 0.1, 0], [0.1, -0.1, 0]], np.float32)
    m = cr.ChromaticMask(2, 2, 1e-4, K, None, 160, 120, corners)
    img = np.full((120, 160), 200, np.uint8)
    m.train(img, [0, 0, 0], [0, 0, 1.0])
    m.mask = np.zeros((120, 160), np.uint8)
    m.mask[m.cellmap == 1] = 1
    idx = np.argwhere(m.cellmap == 2)[:50]
    m.mask[idx[:, 0], idx[:, 1]] = 1   # exactly 50 samples: not retrained
    prob0 = m.prob.copy()
    raw, (fitted, _) = m.update(np.full((120, 160), 90, np.uint8))
    assert raw[1].sum() == 50 and fitted[1] == -1 and np.array_equal(m.prob[1], prob0[1])
    assert raw[0].sum() > 50 and fitted[0] == 1 and abs(int(m.prob[0].argmax()) - 90) <= 1
    assert fitted[2] == fitted[3] == -1


def test_em_two_modes():
    rng = np.random.RandomState(3)
    s = np.concatenate([rng.normal(40, 4, 3000), rng.normal(190, 6, 1000)]).round().clip(0, 255).astype(int)
    raw = np.bincount(s, minlength=256)
    p, inside, fitted, c = cr.em_fit(raw, 1e-4)
    assert fitted and 150 <= c.sum() <= 200
    pi, mu, var = cr.em_fit.params
    order = np.argsort(mu)
    assert abs(mu[order[0]] - 40) < 1.5 and abs(mu[order[1]] - 190) < 1.5
    assert abs(pi[order[0]] - 0.75) < 0.05
    v = np.arange(256.0)
    dens = sum(pi[k] * np.exp(-(v - mu[k]) ** 2 / (2 * var[k])) / math.sqrt(2 * math.pi * var[k]) for k in range(2))
    assert np.allclose(p, dens, rtol=1e-12, atol=1e-300)
    assert inside[40] and inside[190] and not inside[115]


def test_occluded_board_classify2():
    """train on a rendered board, classify2 with a flat grey occluder: measured on the restatement (deterministic): the occluder
    is all 0, and 81 % of the visible board pixels are 1 — the restated quirks (centres of the list ordinals, truncation) cost the
    rest. Counted outside the first cell row and column, where classify2 never sets a sample."""
    sc = scene()
    m2 = sc["m"].classify2(sc["occ"], sc["rvec"], sc["tvec"])
    assert 1 - m2[sc["occ_in"]].mean() >= 0.99
    assert m2[sc["visible"]].mean() >= 0.78


def scene(W=640, H=480, mc=6, thresh=1e-4, rvec=(0.1, -0.15, 0.05)):
    """the occluded rendered board of the CPU and GPU tests"""
    from aruco_amd import synth

    d = json.load(open(os.path.join(ROOT, "tests", "golden", "board.json")))["board_conf"]
    K = np.array([[560.0 * W / 640, 0, W / 2], [0, 560.0 * W / 640, H / 2], [0, 0, 1]], np.float32)
    rng = np.random.RandomState(5)
    rvec, tvec = np.array(rvec, float), np.array([0.0, 0.0, 0.55])
    img, _ = synth.render_board(d["ids"], d["obj"], K.astype(float), rvec, tvec, W, H, rng, unit=0.039 / 100)
    img = img.numpy()
    corners = cr.board_corners(d["obj"], d["info_type"], 0.039)
    m = cr.ChromaticMask(mc, mc, thresh, K, None, W, H, corners)
    m.train(img, rvec, tvec)
    occ = img.copy()
    oy0, oy1, ox0, ox1 = H * 200 // 480, H * 300 // 480, W * 300 // 640, W * 420 // 640
    occ[oy0:oy1, ox0:ox1] = 128
    _, _, Hc, _ = m.geometry(rvec, tvec)
    ys, xs = np.mgrid[0:H, 0:W]
    Hf = Hc.astype(np.float32).reshape(9)
    den = xs * Hf[6] + ys * Hf[7] + Hf[8]
    px, py = (xs * Hf[0] + ys * Hf[1] + Hf[2]) / den, (xs * Hf[3] + ys * Hf[4] + Hf[5]) / den
    reg = (px >= 0.5) & (py >= 0.5) & (px < mc - 1) & (py < mc - 1)
    o = np.zeros((H, W), bool)
    o[oy0:oy1, ox0:ox1] = True
    oi = np.zeros((H, W), bool)
    oi[oy0 + 2:oy1 - 2, ox0 + 2:ox1 - 2] = True
    return {"m": m, "img": img, "occ": occ, "rvec": rvec, "tvec": tvec, "K": K, "corners": corners, "occ_in": oi & reg,
            "visible": reg & ~o, "board": d}


def test_board_corners_rule():
    d = json.load(open(os.path.join(ROOT, "tests", "golden", "board.json")))["board_conf"]
    c = cr.board_corners(d["obj"], 0, 0.039)
    s = np.float32(0.039) / np.float32(100)
    assert np.allclose(c, np.array([[-230, -350, 0], [-230, 350, 0], [230, 350, 0], [230, -350, 0]]) * float(s), rtol=1e-6)
    with pytest.raises(ValueError):
        cr.board_corners(d["obj"], 0, -1)


def test_symbols_exported():
    from aruco_amd.build import library_path

    path = library_path()
    if not os.path.exists(path):
        pytest.skip("libarucohip.so not built")
    L = C.CDLL(path)
    for name in ("arucohip_chromatic_board_corners", "arucohip_chromatic_create", "arucohip_chromatic_destroy", "arucohip_chromatic_train",
                 "arucohip_chromatic_classify", "arucohip_chromatic_update", "arucohip_chromatic_get_mask", "arucohip_chromatic_get_cell_map",
                 "arucohip_chromatic_get_model", "arucohip_chromatic_set_model", "arucohip_em_fit", "arucohip_chromatic_debug_geometry",
                 "arucohip_chromatic_classify_batch"):
        assert hasattr(L, name), name


def test_board_corners_c_abi_equals_restatement():
    from aruco_amd import capi
    from aruco_amd.build import library_path

    if not os.path.exists(library_path()):
        pytest.skip("libarucohip.so not built")
    d = json.load(open(os.path.join(ROOT, "tests", "golden", "board.json")))["board_conf"]
    got = capi.chromatic_board_corners(d["obj"], 0, 0.039)
    assert got.tobytes() == cr.board_corners(d["obj"], 0, 0.039).tobytes()
    obj_m = (np.asarray(d["obj"], np.float32) * np.float32(0.00039)).astype(np.float32)
    assert capi.chromatic_board_corners(obj_m, 1).tobytes() == cr.board_corners(obj_m, 1).tobytes()
    with pytest.raises(capi.ArucoHipError):
        capi.chromatic_board_corners(d["obj"], 0, -1)
