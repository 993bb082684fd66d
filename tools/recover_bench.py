#!/usr/bin/env python3
"""What arucohip_board_recover_batch costs beside arucohip_board_detect_batch, and what it brings back.

One process: a batch of --frames device-resident 4K frames of the bench's board stream (synth.make_board_stream as bench.py --config 4
sets it up; --distinct frames are rendered and repeated to fill the batch), two inner cells of one marker repainted in every fourth
distinct frame. Per run: detect_batch (untimed: a recovery works once per batch), then board_detect_batch and board_recover_batch on
that batch, each between two events on the handle's stream, both returning boards and prob to the host. Prints one JSON line: the
medians, and the share of the board's missing members that came back."""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

from aruco_amd import capi, synth
from aruco_amd.fixtures import load_case

ap = argparse.ArgumentParser()
ap.add_argument("--frames", type=int, default=1024)
ap.add_argument("--distinct", type=int, default=128)
ap.add_argument("--runs", type=int, default=5)
ap.add_argument("--warmup", type=int, default=1)
a = ap.parse_args()
assert torch.cuda.is_available(), "recover_bench.py needs a GPU"
W, H, N, D, CAP = 3840, 2160, a.frames, min(a.distinct, a.frames), 64
UNIT, SIZE = 0.039 / 100.0, 0.039
_, doc = load_case("board")
board = doc["board_conf"]
ids, obj = [int(i) for i in board["ids"]], np.asarray(board["obj"], np.float64).reshape(-1, 4, 3)
K = np.array(doc["intrinsics"]["K"], np.float32).reshape(3, 3)   # CameraParameters::resize rule to 4K, as bench.py
K[0, 0] *= np.float32(W / 640.0); K[0, 2] *= np.float32(W / 640.0)
K[1, 1] *= np.float32(H / 480.0); K[1, 2] *= np.float32(H / 480.0)
distinct, poses = synth.make_board_stream(D, ids, obj, K.reshape(-1), width=W, height=H, seed=4711, device="cuda")
for f in range(0, D, 4):   # two cells of marker f / 4 mod 24 take the opposite colour
    k = (f // 4) % len(ids)
    quad = synth.project(K.astype(np.float64), poses[f][0], poses[f][1], obj[k] * UNIT)
    Hm = synth._homography([(0, 0), (7, 0), (7, 7), (0, 7)], [tuple(p) for p in quad])
    bits = synth.marker_bits(ids[k])
    img = distinct[f].to(torch.float32)
    for cy, cx in ((2, 2), (4, 3)):
        cell = []
        for u, v in ((cx, cy), (cx + 1, cy), (cx + 1, cy + 1), (cx, cy + 1)):
            p = Hm @ np.array([u, v, 1.0])
            cell.append(p[:2] / p[2])
        synth._paint_quad(img, np.array(cell), np.full((1, 1), 25.0 if bits[cy, cx] else 228.0, np.float32), 1, 0)
    distinct[f] = img.round().clamp(0, 255).to(torch.uint8)
frames = distinct.repeat((N + D - 1) // D, 1, 1)[:N].contiguous()
del distinct
torch.cuda.synchronize()
h = capi.Handle(W, H, max_batch=N)
stream = torch.cuda.ExternalStream(h.get_stream())
out = torch.zeros((N, CAP * 96), dtype=torch.uint8, device="cuda")
cnt = torch.zeros(N, dtype=torch.int32, device="cuda")
torch.cuda.synchronize()


def timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record(stream)
    r = fn()
    e1.record(stream)
    e1.synchronize()
    return e0.elapsed_time(e1), r


t_board, t_rec = [], []
for i in range(a.warmup + a.runs):
    h.detect_batch_device(frames.data_ptr(), N, W, H, out.data_ptr(), CAP, cnt.data_ptr(), K=K, marker_size=SIZE)
    h.batch_status()
    tb, before = timed(lambda: h.board_detect_batch(N, ids, obj, board["info_type"], K, [0.0] * 5, SIZE))
    tr, (_, _, rec, after) = timed(lambda: h.board_recover_batch(N, ids, obj, board["info_type"], K, [0.0] * 5, SIZE, cap=0))
    if i >= a.warmup:
        t_board.append(tb), t_rec.append(tr)
missing = sum(len(ids) - b["n_markers"] for b in before)
print(json.dumps({"frames": N, "distinct_frames": D, "width": W, "height": H, "runs": a.runs,
                  "board_detect_batch_ms": round(float(np.median(t_board)), 3), "board_recover_batch_ms": round(float(np.median(t_rec)), 3),
                  "runs_board_ms": [round(t, 3) for t in t_board], "runs_recover_ms": [round(t, 3) for t in t_rec],
                  "members_missing": int(missing), "members_recovered": int(rec.sum()),
                  "share_recovered": round(float(rec.sum()) / max(missing, 1), 4),
                  "frames_with_a_recovery": int((rec > 0).sum()), "members_after": int(sum(b["n_markers"] for b in after))}))
h.close()
