#!/usr/bin/env python3
"""What arucohip_charuco_corners_batch costs, beside refine_pixels_kernel of a SUBPIX batch of the same frame count.

One process: --frames device-resident 1080p frames of a 7 x 5 chessboard-corner board (24 inner corners, 17 markers; --distinct views
are rendered by tests/charuco_ref.py and repeated to fill the batch). Per run: detect_batch (untimed), then charuco_corners_batch on
device frames into a device array, between two events on the handle's stream. Then a SUBPIX handle detects --frames frames of
synth.make_stream (20 markers, 80 corners a frame) with per-kernel timing on, and refine_pixels_kernel's time is read from
arucohip_kernel_times. Prints one JSON line with the medians."""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

from aruco_amd import capi, synth
from tests import charuco_ref as cr

ap = argparse.ArgumentParser()
ap.add_argument("--frames", type=int, default=1024)
ap.add_argument("--distinct", type=int, default=8)
ap.add_argument("--runs", type=int, default=5)
ap.add_argument("--warmup", type=int, default=1)
a = ap.parse_args()
assert torch.cuda.is_available(), "charuco_bench.py needs a GPU"
W, H, N, D, CAP = 1920, 1080, a.frames, min(a.distinct, a.frames), 64
L = (7, 5, 100, 70)
ids = list(range(40, 40 + cr.board_size(L)[2]))
K = np.array([[1400.0, 0, 960.0], [0, 1400.0, 540.0], [0, 0, 1]])
rng = np.random.RandomState(7)
views = []
for i in range(D):   # squares of about 150 px
    rv = rng.uniform(-0.3, 0.3, 3)
    tv = (rng.uniform(-0.05, 0.05), rng.uniform(-0.03, 0.03), 1400.0 * cr.UNIT * L[2] / rng.uniform(140, 160))
    views.append(cr.render(L, ids, rv, tv, seed=100 + i, width=W, height=H, Kc=K)[0])
frames = torch.from_numpy(np.stack(views)).cuda().repeat((N + D - 1) // D, 1, 1)[:N].contiguous()
lay = capi.charuco_layout(L[:2], L[2], L[3])
nc = cr.board_size(L)[3]
h = capi.Handle(W, H, max_batch=N)
stream = torch.cuda.ExternalStream(h.get_stream())
out = torch.zeros((N, CAP * 96), dtype=torch.uint8, device="cuda")
cnt = torch.zeros(N, dtype=torch.int32, device="cuda")
rec = torch.zeros((N, nc, 32), dtype=torch.uint8, device="cuda")
torch.cuda.synchronize()
times, nf = [], None
for i in range(a.warmup + a.runs):
    h.detect_batch_device(frames.data_ptr(), N, W, H, out.data_ptr(), CAP, cnt.data_ptr())
    h.batch_status()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record(stream)
    nf = h.charuco_corners_batch_device(lay, ids, frames.data_ptr(), N, W, H, rec.data_ptr())
    e1.record(stream)
    e1.synchronize()
    if i >= a.warmup:
        times.append(e0.elapsed_time(e1))
markers = float(cnt.float().mean().item())
h.close()
del frames, rec
# the SUBPIX batch: refine_pixels_kernel on every corner of every decoded candidate
p = capi.default_params()
p.corner_method = capi.CORNER_SUBPIX
sframes, _ = synth.make_stream(min(D * 4, N), width=W, height=H, device="cuda")
sframes = sframes.repeat((N + len(sframes) - 1) // len(sframes), 1, 1)[:N].contiguous()
h = capi.Handle(W, H, max_batch=N, params=p)
h.enable_timing(True)
for i in range(a.warmup + a.runs):
    h.detect_batch_device(sframes.data_ptr(), N, W, H, out.data_ptr(), CAP, cnt.data_ptr())
    h.batch_status()
kt = h.kernel_times()
smarkers = float(cnt.float().mean().item())
h.close()
print(json.dumps({"frames": N, "distinct_views": D, "width": W, "height": H, "corners_per_frame": nc, "runs": a.runs,
                  "charuco_corners_batch_ms": round(float(np.median(times)), 3), "runs_ms": [round(t, 3) for t in times],
                  "found_per_frame": round(float(nf.mean()), 2), "markers_per_frame": round(markers, 2),
                  "subpix_refine_pixels_kernel_ms": round(float(kt["refine_pixels_kernel"]), 3), "subpix_markers_per_frame": round(smarkers, 2)}))
