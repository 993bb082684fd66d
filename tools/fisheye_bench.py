#!/usr/bin/env python3
"""What the fisheye calls cost on a stream, event-timed on the handle's stream in one process (the median of --runs):
- markers: arucohip_fisheye_undistort_markers_batch (device output) on the resident markers of an N-frame 1080p batch of
  synth.make_stream (20 markers a frame; --distinct rendered frames, repeated), after an untimed detect_batch each time;
- map: arucohip_fisheye_undistort of --remap-frames device frames with a new map (max_angle alternates, so the map is rebuilt) and
  with the kept map; their difference is the map build. The same for arucohip_undistort with a pinhole model (dist alternates).
Run it under `rocprofv3 --kernel-trace --stats -- python tools/fisheye_bench.py` for the kernels' own times (fisheye_markers_kernel,
fisheye_map_kernel, undist_map_kernel, remap_linear_kernel). Prints one JSON line."""
import argparse
import ctypes as C
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

from aruco_amd import capi, synth

ap = argparse.ArgumentParser()
ap.add_argument("--frames", type=int, default=1024)
ap.add_argument("--distinct", type=int, default=32)
ap.add_argument("--remap-frames", type=int, default=64)
ap.add_argument("--runs", type=int, default=7)
ap.add_argument("--warmup", type=int, default=2)
a = ap.parse_args()
assert torch.cuda.is_available(), "fisheye_bench.py needs a GPU"
W, H, N, CAP = 1920, 1080, a.frames, 64
base, _ = synth.make_stream(a.distinct, seed=4711, device="cuda")
frames = base.repeat((N + a.distinct - 1) // a.distinct, 1, 1)[:N].contiguous()
torch.cuda.synchronize()
h = capi.Handle(W, H, max_batch=N)
stream = torch.cuda.ExternalStream(h.get_stream())
MODEL = (np.array([[1000.0, 0, 959.5], [0, 1000.0, 539.5], [0, 0, 1]]), np.array([-0.03, 0.01, -0.004, 0.001]))
KNEW = np.array([[700.0, 0, 959.5], [0, 700.0, 539.5], [0, 0, 1]], np.float32)
KPIN = np.array([[1400.0, 0, 959.5], [0, 1400.0, 539.5], [0, 0, 1]], np.float32)


def timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record(stream)
    fn()
    e1.record(stream)
    e1.synchronize()
    return e0.elapsed_time(e1)


def median(fn, prepare=None):
    t = []
    for i in range(a.warmup + a.runs):
        if prepare:
            prepare(i)
        ms = timed(lambda: fn(i))
        if i >= a.warmup:
            t.append(ms)
    return round(float(np.median(t)), 4), [round(x, 4) for x in t]


out = torch.zeros((N, CAP * 96), dtype=torch.uint8, device="cuda")
cnt = torch.zeros(N, dtype=torch.int32, device="cuda")
torch.cuda.synchronize()
res = {"frames": N, "width": W, "height": H, "runs": a.runs}
ms, runs = median(lambda i: h.fisheye_undistort_markers_batch_device(N, MODEL, out.data_ptr(), CAP, cnt.data_ptr(), KNEW),
                  prepare=lambda i: h.detect_batch_device(frames.data_ptr(), N, W, H, out.data_ptr(), CAP, cnt.data_ptr()))
h.synchronize()
res["markers"] = {"ms_with_device_copy": ms, "runs_ms": runs, "markers_kept": int(cnt.clamp(min=0).sum().item())}

R = a.remap_frames
dst = torch.zeros((R, H, W), dtype=torch.uint8, device="cuda")
torch.cuda.synchronize()
fish_new, _ = median(lambda i: h.fisheye_undistort_device(frames.data_ptr(), R, W, H, 1, dst.data_ptr(), MODEL, KNEW, 1.2 + 0.01 * (i % 2)))
fish_kept, _ = median(lambda i: h.fisheye_undistort_device(frames.data_ptr(), R, W, H, 1, dst.data_ptr(), MODEL, KNEW, 1.2))


def pinhole(dist):
    d = np.asarray(dist, np.float32)
    h._chk(h.L.arucohip_undistort(h.h, C.c_void_p(frames.data_ptr()), R, W, H, W, W * H, 1, 1, KPIN.ctypes.data_as(C.c_void_p),
                                  d.ctypes.data_as(C.c_void_p), d.size, C.c_void_p(dst.data_ptr()), 1))


pin_new, _ = median(lambda i: pinhole([-0.12 - 0.001 * (i % 2), 0.05, 1e-3, -8e-4, 0.01]))
pin_kept, _ = median(lambda i: pinhole([-0.12, 0.05, 1e-3, -8e-4, 0.01]))
res["remap"] = {"frames": R, "fisheye_ms_new_map": fish_new, "fisheye_ms_kept_map": fish_kept, "fisheye_map_build_ms": round(fish_new - fish_kept, 4),
                "pinhole_ms_new_map": pin_new, "pinhole_ms_kept_map": pin_kept, "pinhole_map_build_ms": round(pin_new - pin_kept, 4)}
print(json.dumps(res))
h.close()
