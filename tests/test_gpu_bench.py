"""bench.py on the GPU at a small size: --steps is the number of timed steps the result line reports, --dump-outputs writes the
results of the last timed step - the same markers the library returns for those frames when it is called directly - and --full adds
what a plain run leaves out."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.gpu
def test_bench_dump_outputs_are_the_last_steps_results(tmp_path):
    import torch

    from aruco_amd import capi, synth

    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "WORLD_SIZE", "LOCAL_RANK")}
    # 64 distinct frames in batches of 32: the third step (the last) runs frames 0..31 again
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "3", "--warmup", "1", "--batch", "32",
                        "--frames", "64", "--no-cpu-baseline", "--no-latency", "--no-legs", "--dump-outputs", str(tmp_path)],
                       stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, env=env, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [l for l in r.stdout.splitlines() if l.strip()]
    assert len(lines) == 1
    doc = json.loads(lines[0])
    assert doc["steps"] == 3 and doc["ms_per_step"] > 0 and doc["config"]["frames_per_step_per_gpu"] == 32
    d = {f[:-4]: np.load(str(tmp_path / f)) for f in os.listdir(str(tmp_path))}
    assert all(v.dtype in (np.float32, np.float64) for v in d.values())
    assert np.array_equal(d["frame_index"], np.arange(32)) and d["ids"].shape == (32, 64)

    frames, truth = synth.make_stream(64, seed=4711, device="cuda")
    fr = frames[:32].cpu().numpy()
    del frames
    torch.cuda.synchronize()
    h = capi.Handle(1920, 1080, max_batch=32)
    try:
        ref = h.detect_batch_host(fr, cap=64)
    finally:
        h.close()
    assert sum(len(m) for m in ref) >= 0.9 * sum(len(t) for t in truth[:32])
    for f, m in enumerate(ref):
        n = len(m)
        assert d["counts"][f] == n and (d["ids"][f, n:] == -1).all()
        assert np.array_equal(d["ids"][f, :n], m["id"])
        assert np.allclose(d["corners"][f, :n].reshape(n, 8), m["corners"], rtol=0, atol=1e-4)


@pytest.mark.gpu
def test_bench_full_adds_what_a_plain_run_leaves_out():
    """A plain run prints the headline and the workload it was measured on; --full (here without its CPU baseline, latency and child legs)
    adds the figures of the passes after the timed region, the roofline and the per-kernel times."""
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "WORLD_SIZE", "LOCAL_RANK")}
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "3", "--warmup", "1", "--batch", "32", "--frames", "32"]
    docs = []
    for extra in ([], ["--full", "--no-cpu-baseline", "--no-latency", "--no-legs"]):
        r = subprocess.run(cmd + extra, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, env=env, timeout=600)
        assert r.returncode == 0, r.stderr[-3000:]
        lines = [l for l in r.stdout.splitlines() if l.strip()]
        assert len(lines) == 1
        docs.append(json.loads(lines[0]))
    plain, full = docs
    for k in ("metric", "unit", "higher_is_better", "dtype", "steps", "warmup", "n_gpus"):
        assert plain[k] == full[k]
    assert plain["value"] > 0 and plain["ms_per_step"] > 0 and plain["config"]["frames_per_step_per_gpu"] == 32
    assert not {"roofline", "kernel_ms_per_launch", "kernel_ms_isolated"} & set(plain)
    assert full["roofline"]["avg_launch_ms"] > 0 and full["kernel_ms_isolated"]["threshold_kernel"] > 0
