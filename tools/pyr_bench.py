#!/usr/bin/env python3
"""What MarkerDetector::pyrDown(level) buys on a stream, and what its reduction kernel costs.

--mode detect (default): in one process, N device-resident 1080p frames of synth.make_stream, warmed, alternating, event-timed runs of
detect_batch at levels 0, 1 and 2 (the median of --runs per level), and per level the frames whose ids equal the rendered ids.
--mode kernel: arucohip_pyr_down (one level, device to device) on the same frames beside a device-to-device hipMemcpyAsync of the same
read-plus-written bytes, both event-timed in this process; run it under `rocprofv3 --kernel-trace --stats -- python tools/pyr_bench.py
--mode kernel` for pyr_down_kernel's own time. Bytes are algorithmic, counted from shapes: 1.25 W H per frame and level.
Prints one JSON line."""
import argparse
import ctypes as C
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

from aruco_amd import capi, synth

HBM_PEAK_TBPS = 8.0   # MI355X specification

ap = argparse.ArgumentParser()
ap.add_argument("--mode", choices=["detect", "kernel"], default="detect")
ap.add_argument("--frames", type=int, default=1024)
ap.add_argument("--runs", type=int, default=5)
ap.add_argument("--warmup", type=int, default=2)
a = ap.parse_args()
assert torch.cuda.is_available(), "pyr_bench.py needs a GPU"
W, H, N, CAP = 1920, 1080, a.frames, 64
frames, truth = synth.make_stream(N, seed=4711, device="cuda")
torch.cuda.synchronize()
h = capi.Handle(W, H, max_batch=N)
stream = torch.cuda.ExternalStream(h.get_stream())


def timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record(stream)
    fn()
    e1.record(stream)
    e1.synchronize()
    return e0.elapsed_time(e1)


if a.mode == "detect":
    out = torch.zeros((N, CAP * 96), dtype=torch.uint8, device="cuda")
    cnt = torch.zeros(N, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    levels = (0, 1, 2)
    times = {l: [] for l in levels}
    exact = {}

    def run(level):
        h.set_pyr_down(level)
        return timed(lambda: h.detect_batch_device(frames.data_ptr(), N, W, H, out.data_ptr(), CAP, cnt.data_ptr()))

    for i in range(a.warmup + a.runs):
        for l in levels:   # alternating: every level sees the same drift of the machine
            ms = run(l)
            if i >= a.warmup:
                times[l].append(ms)
    for l in levels:
        run(l)
        h.batch_status()
        torch.cuda.synchronize()
        arr = np.frombuffer(out.cpu().numpy().tobytes(), dtype=capi.MARKER_DTYPE).reshape(N, CAP)
        n = cnt.cpu().numpy()
        exact[l] = sum(1 for f in range(N) if sorted(int(m["id"]) for m in arr[f, :max(n[f], 0)]) == sorted(int(t["id"]) for t in truth[f]))
    res = {"mode": "detect", "frames": N, "width": W, "height": H, "runs": a.runs}
    for l in levels:
        ms = float(np.median(times[l]))
        res["level%d" % l] = {"ms_per_batch": round(ms, 3), "frames_per_s": round(N / ms * 1e3, 1), "runs_ms": [round(t, 3) for t in times[l]],
                              "frames_with_exactly_the_rendered_ids": exact[l]}
    print(json.dumps(res))
else:
    hip = None
    for line in open("/proc/self/maps"):   # the HIP runtime this process already uses
        if "libamdhip64" in line:
            hip = C.CDLL(line.split()[-1])
            break
    assert hip is not None
    hip.hipMemcpyAsync.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int, C.c_void_p]
    wo, ho = (W + 1) // 2, (H + 1) // 2
    dst = torch.zeros((N, ho, wo), dtype=torch.uint8, device="cuda")
    nbytes = N * (W * H + wo * ho)              # read plus written
    half = nbytes // 2                          # a copy of `half` bytes reads and writes as much
    ca = torch.zeros(half, dtype=torch.uint8, device="cuda")
    cb = torch.zeros(half, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    sp = C.c_void_p(h.get_stream())

    def copy():
        assert hip.hipMemcpyAsync(C.c_void_p(cb.data_ptr()), C.c_void_p(ca.data_ptr()), half, 3, sp) == 0   # 3 = hipMemcpyDeviceToDevice

    def pyr():
        h.pyr_down_device(frames.data_ptr(), N, W, H, 1, dst.data_ptr())

    tp, tc = [], []
    for i in range(a.warmup + a.runs):
        p, c = timed(pyr), timed(copy)
        if i >= a.warmup:
            tp.append(p), tc.append(c)
    mp, mc = float(np.median(tp)), float(np.median(tc))
    print(json.dumps({"mode": "kernel", "frames": N, "bytes_read_plus_written": nbytes, "pyr_down_ms": round(mp, 4), "copy_ms": round(mc, 4),
                      "pyr_down_tb_per_s": round(nbytes / mp / 1e9, 3), "copy_tb_per_s": round(2 * half / mc / 1e9, 3),
                      "pyr_down_rate_over_copy_rate": round(mc / mp, 3), "share_of_8_tb_per_s_peak": round(nbytes / mp / 1e9 / HBM_PEAK_TBPS, 3),
                      "runs_pyr_ms": [round(t, 4) for t in tp], "runs_copy_ms": [round(t, 4) for t in tc]}))
h.close()
