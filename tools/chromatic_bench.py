#!/usr/bin/env python3
"""Throughput of the board occlusion mask: arucohip_chromatic_classify_batch over N resident 1080p board frames (device frames and
masks), timed with device events after warm-up; the median of --runs. Bytes are counted from shapes: the mask writes (W x H per
frame) plus the rows classify2 reads inside each frame's rectangle (every other row). The per-kernel split comes from a separate
`rocprofv3 --kernel-trace --stats -- python tools/chromatic_bench.py` run."""
import argparse
import json
import math
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

from aruco_amd import capi, synth
from aruco_amd.fixtures import load_case

COPY_TBPS = 6.29   # the measured device-to-device copy rate of one MI355X

ap = argparse.ArgumentParser()
ap.add_argument("--frames", type=int, default=1024)
ap.add_argument("--runs", type=int, default=7)
ap.add_argument("--warmup", type=int, default=2)
ap.add_argument("--method", type=int, default=2)
ap.add_argument("--grid", type=int, default=6)
a = ap.parse_args()
W, H, N = 1920, 1080, a.frames
_, doc = load_case("board")
bc = doc["board_conf"]
K = np.array([[1700.0, 0, 955.0], [0, 1690.0, 545.0], [0, 0, 1]], np.float32)
frames, _ = synth.make_board_stream(N, bc["ids"], bc["obj"], K.reshape(-1), width=W, height=H, seed=77, device="cuda")
torch.cuda.synchronize()
h = capi.Handle(W, H, max_batch=N)
marks = torch.zeros((N, 128 * 96), dtype=torch.uint8, device="cuda")
cnt = torch.zeros(N, dtype=torch.int32, device="cuda")
h.detect_batch_device(frames.data_ptr(), N, W, H, marks.data_ptr(), 128, cnt.data_ptr())
h.batch_status()
boards = h.board_detect_batch(N, bc["ids"], bc["obj"], bc["info_type"], K=K, marker_size=0.039)
m = h.chromatic(a.grid, a.grid, 1e-4, K, None, W, H, capi.chromatic_board_corners(bc["obj"], bc["info_type"], 0.039))
f0 = next(f for f in range(N) if boards[f]["has_pose"])
m.train(frames[f0].cpu().numpy(), boards[f0]["rvec"], boards[f0]["tvec"])
masks = torch.empty((N, H, W), dtype=torch.uint8, device="cuda")
npix = np.zeros(N, np.int32)
stream = torch.cuda.ExternalStream(h.get_stream())
times = []
for i in range(a.warmup + a.runs):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record(stream)
    m.classify_batch_device(h, frames.data_ptr(), N, W, W * H, masks.data_ptr(), method=a.method, npix=npix)
    e1.record(stream)
    e1.synchronize()
    if i >= a.warmup:
        times.append(e0.elapsed_time(e1))
ms = float(np.median(times))
read = 0
for f in range(N):
    c2 = m.debug_geometry(f)[0]
    # classify2's rectangle: boundingRect, then fitRectToSize (start clamped to 0, end = clamped start + width, clipped)
    x, y = math.floor(c2[:, 0].min()), math.floor(c2[:, 1].min())
    x0, y0 = max(x, 0), max(y, 0)
    x1, y1 = min(x0 + math.floor(c2[:, 0].max()) + 1 - x, W), min(y0 + math.floor(c2[:, 1].max()) + 1 - y, H)
    if boards[f]["has_pose"] and x1 > x0 and y1 > y0:
        read += (x1 - x0) * ((y1 - y0 + 1) // 2)
nbytes = N * W * H + read
print(json.dumps({"frames": N, "method": a.method, "grid": a.grid, "ms_per_batch": round(ms, 4), "frames_per_s": round(N / ms * 1e3, 1),
                  "runs_ms": [round(t, 4) for t in times], "bytes": nbytes, "tb_per_s": round(nbytes / ms / 1e9, 3),
                  "fraction_of_copy_rate": round(nbytes / ms / 1e9 / COPY_TBPS, 3), "frames_with_pose": int(sum(b["has_pose"] for b in boards)),
                  "mean_npix": float(npix.mean())}))
m.close()
h.close()
