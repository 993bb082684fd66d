#!/usr/bin/env python3
"""The host model's scipy solve (tests/rig_ref.py) on the detections that tools/rig_bench.py --dump wrote: one timed solve of the rig
calibration from the model's own start values (trf with the Jacobian's sparsity; a dense numeric Jacobian of 810 unknowns by 196 608
residuals does not finish in reasonable time). Needs no GPU. Prints one JSON line: seconds, rms, how far the result is from the device's."""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np

from tests import rig_ref as rr
from tests.planar_ref import rodrigues

ap = argparse.ArgumentParser()
ap.add_argument("dump")
a = ap.parse_args()
z = np.load(a.dump)
nc = len(z["rvecs"])
cams = [{"K": z["K"].astype(np.float64), "dist": None} for _ in range(nc)]
ninstants = (int(z["view"].max()) + nc) // nc
views = rr.select((z["view"], z["id"], z["corners"]), cams, z["ids"], z["obj"], ninstants, 1)
sv = rr.start_values(views, nc, ninstants)
inst = [t for t in range(ninstants) if sv["used"][t]]
prob = rr.Problem(views, cams, z["obj"], nc, inst, sv["calibrated"])
x0 = prob.pack(sv["T"], sv["poses"])
t0 = time.perf_counter()
x = prob.solve(x0, method="trf", sparse=True)
seconds = time.perf_counter() - t0
T = [None] * nc
for c, Tk in zip([0] + prob.cams, prob.transforms(x)[0]):
    T[c] = Tk
dev = [(rodrigues(r), t) for r, t in zip(z["rvecs"], z["tvecs"])]
print(json.dumps({"unknowns": len(x0), "residuals": 2 * len(prob.pt), "instants_used": len(inst), "solve_seconds": round(seconds, 2), "rms_px": prob.rms(x),
                  "device_rms_px": float(z["rms"]), "device_against_scipy_m": rr.cam_dev(dev, T, z["obj"])}))
