#!/usr/bin/env python3
"""Time of HRM dictionary generation on the device: arucohip_hrm_create_dictionary for the shapes of the reference's shipped
dictionaries (n = 5, 6, 8 with 100 markers) and n = 8 with 1000 markers, timed with device events after warm-up; the median of
--runs. For each: candidates examined, candidates per second, windows and host synchronisations. --host-ref adds the NumPy
restatement's host time for the smallest case (tests/hrm_ref.py, not the reference's own speed). The per-kernel split comes from a
separate `rocprofv3 --kernel-trace --stats -- python tools/hrm_bench.py` run."""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

from aruco_amd import capi

ap = argparse.ArgumentParser()
ap.add_argument("--runs", type=int, default=5)
ap.add_argument("--warmup", type=int, default=1)
ap.add_argument("--seed", type=int, default=12345)
ap.add_argument("--cases", default="5x100,6x100,8x100,8x1000")
ap.add_argument("--host-ref", action="store_true")
a = ap.parse_args()
torch.cuda.init()
h = capi.Handle(64, 64)
stream = torch.cuda.ExternalStream(h.get_stream())
for case in a.cases.split(","):
    n, size = (int(x) for x in case.split("x"))
    times, first = [], None
    for i in range(a.warmup + a.runs):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(stream)
        codes, tau0, examined = h.hrm_create_dictionary(n, size, a.seed)
        e1.record(stream)
        e1.synchronize()
        first = first if first is not None else codes.tobytes()
        assert codes.tobytes() == first
        if i >= a.warmup:
            times.append(e0.elapsed_time(e1))
    ms = float(np.median(times))
    c = h.debug_hrm_counters()
    row = {"n": n, "size": size, "seed": a.seed, "tau0": tau0, "examined": examined, "ms": round(ms, 3),
           "candidates_per_s": round(examined / ms * 1e3, 1), "windows": c["windows"], "host_syncs": c["syncs"],
           "tau_decrements": c["decrements"], "runs_ms": [round(t, 3) for t in times]}
    if a.host_ref and case == a.cases.split(",")[0]:
        from tests import hrm_ref as hr

        t = time.perf_counter()
        ref = hr.create_dictionary(n, size, a.seed)
        row["numpy_restatement_host_s"] = round(time.perf_counter() - t, 3)
        assert ref[0].tobytes() == first and ref[1:] == (tau0, examined)
    print(json.dumps(row), flush=True)
h.close()
