"""Camera calibration, host side: the C ABI and the library declare and export both entry points, the shim's calibrateCamera /
saveToFile caller compiles, and the host model the GPU tests compare against (tests/calib_ref.py) recovers a known camera."""
import os
import subprocess

import numpy as np

from tests import calib_ref as cr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("arucohip_calibrate_camera", "arucohip_calibrate_board_batch", "arucohip_debug_calib_start")


def test_library_exports_the_calibration_entry_points():
    from aruco_amd import build_library, capi

    lib = build_library()
    names = subprocess.run(["nm", "-D", "--defined-only", lib], stdout=subprocess.PIPE, text=True, check=True).stdout
    exported = set(line.split()[-1] for line in names.splitlines() if line.strip())
    header = open(os.path.join(ROOT, "include", "arucohip.h")).read()
    for s in NEW:
        assert s in exported and s in capi.SYMBOLS and (s + "(") in header
    assert (capi.CALIB_USE_INTRINSIC_GUESS, capi.CALIB_FIX_ASPECT_RATIO, capi.CALIB_FIX_PRINCIPAL_POINT, capi.CALIB_ZERO_TANGENT_DIST,
            capi.CALIB_FIX_FOCAL_LENGTH, capi.CALIB_FIX_K1, capi.CALIB_FIX_K2, capi.CALIB_FIX_K3) == (1, 2, 4, 8, 16, 32, 64, 128)


def test_shim_calibration_caller_compiles(tmp_path):
    from tests.test_gpu_calib import build_shim_calib

    exe = tmp_path / "shim_calib"
    build_shim_calib(exe)
    assert exe.exists()


def test_host_model_recovers_the_camera():
    objs, imgs = cr.make_views(12, noise=0.0, seed=9)
    start, _, _ = cr.start_values(objs, imgs, cr.SIZE)
    assert np.all(np.abs(start[:2] / [1400, 1390] - 1) < 0.05)
    ref = cr.scipy_calibrate(objs, imgs, cr.SIZE)
    assert np.all(np.abs(ref["intr"][:4] / cr.intr_of(cr.K_TRUE, cr.DIST_TRUE)[:4] - 1) < 1e-5)
    assert np.max(np.abs(ref["intr"][4:] - cr.DIST_TRUE)) < 1e-4 and ref["rms"] < 1e-3
