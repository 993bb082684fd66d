"""aruco_amd/csrc/frames_host.h on the CPU: the record of a batch of strided images that the C ABI's image entry points share."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_image_batch_record_against_enumeration(tmp_path):
    """The header is plain C++ so that tests/cpp/frames_check.cpp can walk it with the host compiler over small batches: the stride check
    refuses exactly the two rules, extent() is one past the largest byte offset, the overlap test is the intersection of the two
    intervals (touching and one-byte placements included), and the copy plan between the caller's layout and the packed one, replayed
    with memcpy on arrays of exactly extent() bytes, moves every image byte to its own packed byte and back, touches no padding, and
    is one copy for a gap-free batch and one per image otherwise."""
    exe = str(tmp_path / "frames_check")
    subprocess.run(["g++", "-std=c++17", "-O2", "-Wall", "-Wextra", "-Werror", os.path.join(ROOT, "tests", "cpp", "frames_check.cpp"), "-o", exe], check=True)
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr[-3000:]
    assert " 0 failures" in r.stdout
