"""MarkerDetector::pyrDown on the CPU side: the reference definition of the reduction (tests/pyr_ref.py), the restated tail of detect()
against the oracle, the conditions the GPU tests rest on, and the new entry points of the interface."""
import os
import re
import subprocess

import numpy as np
import pytest

from tests import pyr_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ["arucohip_set_pyr_down", "arucohip_get_pyr_down", "arucohip_pyr_down"]


@pytest.mark.parametrize("shape", [(1, 1), (2, 3), (5, 4), (9, 7)])
def test_pyr_down_equals_the_double_loop(shape):
    g = np.random.RandomState(shape[0] * 31 + shape[1]).randint(0, 256, size=shape).astype(np.uint8)
    out = pyr_ref.pyr_down(g)
    assert out.shape == ((shape[0] + 1) // 2, (shape[1] + 1) // 2)
    assert np.array_equal(out, pyr_ref.pyr_down_brute(g))


def test_constant_image_stays_constant():
    for v in (0, 1, 77, 255):
        assert np.all(pyr_ref.pyr_down(np.full((11, 14), v, np.uint8)) == v)   # (256 v + 128) >> 8 = v


def test_checkerboard_value():
    """A 0 / 255 checkerboard: the taps 1, 6, 1 fall on one colour and 4, 4 on the other in each direction, so a pixel centred on white sees
    (8 * 8 + 8 * 8) * 255 = 32640 of 65536, away from the border and, by the reflection about the edge pixel, at it: (32640 + 128) >> 8 = 128.
    Every output pixel is centred on an even position, which is white."""
    yy, xx = np.mgrid[0:12, 0:16]
    g = (((yy + xx) % 2 == 0) * 255).astype(np.uint8)
    assert np.all(pyr_ref.pyr_down(g) == 128)


@pytest.mark.parametrize("name", ["640x480", "1280x720"])
@pytest.mark.parametrize("cam", [False, True])
def test_chain_level0_equals_the_oracle_bit_for_bit(name, cam):
    from oracle import orc
    frames, _ = pyr_ref.frames_of(name)
    for f in range(3):
        got, _ = pyr_ref.chain_cached(name, f, 0, cam=cam)
        if cam:
            exp = orc.Oracle().detect(frames[f], K=pyr_ref.CAM_K, dist=pyr_ref.CAM_DIST, marker_size=pyr_ref.CAM_SIZE)
        else:
            exp = orc.Oracle().detect(frames[f])
        assert [m["id"] for m in got] == [m["id"] for m in exp]
        for a, b in zip(got, exp):
            assert np.asarray(a["corners"], np.float32).tobytes() == np.asarray(b["corners"], np.float32).tobytes()
            assert a["has_pose"] == b["has_pose"]
            assert np.asarray(a["rvec"]).tobytes() == np.asarray(b["rvec"]).tobytes()
            assert np.asarray(a["tvec"]).tobytes() == np.asarray(b["tvec"]).tobytes()


@pytest.mark.parametrize("name", ["640x480", "1280x720"])
@pytest.mark.parametrize("level", [1, 2])
def test_chain_finds_the_truth_ids(name, level):
    """What keeps the GPU tests from comparing two empty lists."""
    _, truth = pyr_ref.frames_of(name)
    n = pyr_ref.FRAME_SETS[name][2]
    for f in range(3):
        got, _ = pyr_ref.chain_cached(name, f, level)
        assert len(truth[f]) == n
        assert [m["id"] for m in got] == truth[f]


def test_library_exports_the_new_symbols():
    from aruco_amd import capi
    from aruco_amd.build import library_path
    out = subprocess.run(["nm", "-D", "--defined-only", library_path()], stdout=subprocess.PIPE, text=True, check=True).stdout
    names = set(line.split()[-1] for line in out.splitlines() if line.strip())
    for s in NEW_SYMBOLS:
        assert s in names and s in capi.SYMBOLS


def test_header_declares_the_new_symbols():
    text = open(os.path.join(ROOT, "include", "arucohip.h")).read()
    for s in NEW_SYMBOLS:
        assert re.search(r"\b%s\s*\(" % s, text), s
    shim = open(os.path.join(ROOT, "include", "aruco_hip_shim.hpp")).read()
    assert re.search(r"void\s+pyrDown\s*\(\s*unsigned int", shim)


def test_python_handle_has_the_option():
    from aruco_amd import capi
    assert callable(getattr(capi.Handle, "set_pyr_down"))
    assert isinstance(capi.Handle.pyr_down, property)
    assert callable(getattr(capi.Handle, "pyr_down_image"))
