"""The run rule of one start candidate (aruco_amd/csrc/cand_rule.h, what every lane of candidates_sparse_kernel runs) compiled for the host and
compared with a pixel-by-pixel loop: tests/cpp/cand_rule_check.cpp. No GPU."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_cand_rule16_equals_the_pixel_loop(tmp_path):
    exe = str(tmp_path / "cand_rule_check")
    subprocess.run(["g++", "-std=c++17", "-O2", "-Wall", "-Wextra", "-Werror", os.path.join(ROOT, "tests", "cpp", "cand_rule_check.cpp"), "-o", exe], check=True)
    r = subprocess.run([exe], stdout=subprocess.PIPE, text=True)
    assert r.returncode == 0, r.stdout
    assert "cases equal" in r.stdout
