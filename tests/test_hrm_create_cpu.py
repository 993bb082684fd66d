"""HRM dictionary and board generation: the NumPy restatement (tests/hrm_ref.py) against glibc's rand() and the reference's
board4x4 fixture, the chromatic form, the C ABI symbols, and the shim test program's compilation. No GPU."""
import ctypes as C
import json
import os
import subprocess

import numpy as np
import pytest

from tests import hrm_ref as hr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")


def read_pgm(path):
    with open(path, "rb") as f:
        data = f.read()
    parts = data.split(maxsplit=4)
    assert parts[0] == b"P5" and parts[3] == b"255"
    w, h = int(parts[1]), int(parts[2])
    return np.frombuffer(parts[4], np.uint8, count=w * h).reshape(h, w)


def load_board4x4():
    """(board4x4.png as gray, {ids, obj} of board4x4.yml, the 16 codes it was made from: d4x4_100's first 16 markers)"""
    png = read_pgm(os.path.join(GOLDEN, "board4x4.pgm"))
    doc = json.load(open(os.path.join(GOLDEN, "board4x4.json")))
    d = json.load(open(os.path.join(GOLDEN, "hrm.json")))["dictionary"]
    codes = np.array([sum(1 << i for i, ch in enumerate(m) if ch == "1") for m in d["markers"][:16]], np.uint64)
    return png, doc["board"], codes


@pytest.mark.parametrize("seed", [0, 1, 42, 2**31 + 7, 2**32 - 1])
def test_stream_equals_libc_rand(seed):
    libc = C.CDLL(None)
    libc.srand(C.c_uint(seed))
    want = [libc.rand() for _ in range(30000)]
    assert hr.rand_python(seed, 2000) == want[:2000]
    assert hr.stream(seed, 0, 30000, run=1000).tolist() == want
    assert hr.stream(seed, 12345, 7000).tolist() == want[12345:19345]


def test_block_walk_equals_literal_loop():
    # one candidate at a time on libc's rand() (134 094 candidates, 4 tau decrements, three with the |D| < 2 limit) and the block walk agree
    libc = C.CDLL(None)
    libc.srand(3)
    a = hr.create_dictionary_literal(5, 4, libc.rand)
    b = hr.create_dictionary(5, 4, 3)
    assert a[0].tobytes() == b[0].tobytes() and a[1:] == b[1:] == (12, 134094)


def test_board4x4_restated():
    png, yml, codes = load_board4x4()
    img, ids, obj = hr.board_image(codes, 4, 4, 4)
    assert img.tobytes() == png.tobytes()
    assert np.array_equal(obj, np.array(yml["obj"], np.float32))
    # written by an older getId() (1 << pos): the current one (2 << pos) gives twice the fixture's ids
    assert np.array_equal(ids, 2 * np.array(yml["ids"]))
    assert yml["info_type"] == 0


def test_chromatic_restated():
    _, _, codes = load_board4x4()
    gray, _, _ = hr.board_image(codes, 4, 4, 4)
    img, _, _ = hr.board_image(codes, 4, 4, 4, chromatic=True)
    gap = 24
    assert img.shape == (552 + 2 * gap, 552 + 2 * gap, 3)
    colours = {tuple(c) for c in img.reshape(-1, 3)}
    assert colours == {(250, 134, 4), (0, 255, 0)}
    inner = img[gap:-gap, gap:-gap]
    assert np.array_equal(np.all(inner == (0, 255, 0), axis=2), gray == 0)
    assert np.all(img[:gap] == (250, 134, 4)) and np.all(img[:, -gap:] == (250, 134, 4))


def test_restated_marker_code():
    # rotation 1 of a single bit at (0, 0) lands at (0, n - 1); getId = 2 << pos; self distance of a symmetric code is 0
    n = 4
    assert int(hr.rotations(1, n)[0, 1]) == 1 << (n - 1)
    assert int(hr.rotations(1, n)[0, 2]) == 1 << (n * n - 1)
    assert hr.get_id(0b101, n) == 2 + 8
    full = (1 << 16) - 1
    assert int(hr.self_distance(full, n)[0]) == 0 and hr.distance(full, 0, n) == 16


def test_c_abi_symbols():
    from aruco_amd import capi

    hdr = open(os.path.join(ROOT, "include", "arucohip.h")).read()
    for s in ("arucohip_hrm_create_dictionary", "arucohip_hrm_board_size", "arucohip_hrm_board_image", "arucohip_debug_hrm_stream",
              "arucohip_debug_hrm_counters"):
        assert s in capi.SYMBOLS and (s + "(") in hdr
    names = subprocess.run(["nm", "-D", "--defined-only", capi.library_path()], stdout=subprocess.PIPE, text=True, check=True).stdout
    for s in ("arucohip_hrm_create_dictionary", "arucohip_hrm_board_size", "arucohip_hrm_board_image", "arucohip_debug_hrm_stream",
              "arucohip_debug_hrm_counters"):
        assert s in names.split()


def test_board_size_without_gpu():
    from aruco_amd import capi

    L = capi.load()
    w, h, ch = C.c_int(), C.c_int(), C.c_int()
    assert L.arucohip_hrm_board_size(4, 4, 4, 0, C.byref(w), C.byref(h), C.byref(ch)) == 0 and (w.value, h.value, ch.value) == (552, 552, 1)
    assert L.arucohip_hrm_board_size(5, 6, 4, 1, C.byref(w), C.byref(h), C.byref(ch)) == 0
    assert (w.value, h.value, ch.value) == (980 + 56, 644 + 56, 3)
    assert L.arucohip_hrm_board_size(2, 4, 4, 0, C.byref(w), C.byref(h), C.byref(ch)) == capi.E_INVALID


def test_shim_program_compiles(tmp_path):
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror", "-fsyntax-only", "-I" + os.path.join(ROOT, "include"),
                    "-I/opt/rocm/include", os.path.join(ROOT, "tests", "cpp", "shim_hrm_create.cpp")], check=True)
