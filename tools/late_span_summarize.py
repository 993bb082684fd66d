#!/usr/bin/env python3
"""The late walker generations of a pipeline lane, from a rocprofv3 kernel trace of the pipelined bench (tools/trace_overlap.sh).

Per main stream (a stream that runs threshold kernels) the kernels in start order; a batch is walker_kernel, its walker_long_kernel launches
and the kernel behind them (contour_quad_kernel, or late_quad_kernel = the late walks and contour_quad's first pass in one launch).
Per batch, steady-state window:
  generations    walker_long_kernel launches of the batch
  late span      start of generation 4 - end of the last generation (a build whose late walks run inside late_quad_kernel has none)
  beside         kernels of OTHER streams running during the late span: time-weighted mean, and the share of the span with two or more
  quad           duration of the kernel behind the generations, and of a second contour_quad_kernel behind that one (the late borders' pass)
and the in-stream gap in front of every kernel kind. Usage: late_span_summarize.py kernel_trace.csv [generations in front of the late ones = 3]"""
import collections
import csv
import statistics
import sys


def short(name):
    return name.split("(")[0].replace("void ", "").replace("ah::", "").split("<")[0]


def stats(v, scale=1e3, unit="us"):
    v = sorted(v)
    if not v:
        return "n 0"
    return "n %4d  median %8.1f  mean %8.1f  p90 %8.1f  max %8.1f %s" % (len(v), statistics.median(v) / scale, sum(v) / len(v) / scale, v[int(0.9 * (len(v) - 1))] / scale, v[-1] / scale, unit)


rows = list(csv.DictReader(open(sys.argv[1])))
early = int(sys.argv[2]) if len(sys.argv) > 2 else 3
key = "Stream_Id" if rows and "Stream_Id" in rows[0] and len(set(r["Stream_Id"] for r in rows)) > 1 else "Queue_Id"
streams = collections.defaultdict(list)
for r in rows:
    streams[r[key]].append((int(r["Start_Timestamp"]), int(r["End_Timestamp"]), short(r["Kernel_Name"])))
for v in streams.values():
    v.sort()
mains = {s: v for s, v in streams.items() if any("threshold" in k for _, _, k in v)}
thr = sorted(st for v in mains.values() for st, _, k in v if "threshold" in k)
lo, hi = thr[len(thr) // 4], thr[(3 * len(thr)) // 4]
print("streams told apart by %s; %d main streams; steady-state window %.3f ms" % (key, len(mains), (hi - lo) / 1e6))

gaps = collections.defaultdict(list)
for v in mains.values():
    for (s0, e0, k0), (s1, e1, k1) in zip(v, v[1:]):
        if lo <= s1 < hi and "threshold" not in k1 and not k1.startswith("__amd_rocclr_fill"):
            gaps[k1].append(s1 - e0)
print("in-stream gap in front of a kernel (main streams):")
for k, g in sorted(gaps.items()):
    print("  %-28s %s" % (k, stats(g)))


def beside(m, a, b):
    """time-weighted mean number of other streams' kernels in [a, b) and the share of it with two or more"""
    ev = []
    for s, v in streams.items():
        if s == m:
            continue
        for st, en, _ in v:
            if en > a and st < b:
                ev.append((max(st, a), 1)), ev.append((min(en, b), -1))
    ev.sort()
    depth, last, area, two = 0, a, 0, 0
    for t, d in ev:
        area += depth * (t - last)
        if depth >= 2:
            two += t - last
        last, depth = t, depth + d
    return area / max(1, b - a), two / max(1, b - a)


ngen, span, mean_beside, two_share, quad, quad2 = [], [], [], [], collections.defaultdict(list), []
for m, v in mains.items():
    i = 0
    while i < len(v):
        if v[i][2] != "walker_kernel" or not (lo <= v[i][0] < hi):
            i += 1
            continue
        j = i + 1
        while j < len(v) and v[j][2] == "walker_long_kernel":
            j += 1
        gens = v[i + 1:j]
        ngen.append(len(gens))
        if len(gens) > early:
            a, b = gens[early][0], gens[-1][1]
            span.append(b - a)
            mb, ts = beside(m, a, b)
            mean_beside.append(mb), two_share.append(ts)
        if j < len(v):
            quad[v[j][2]].append(v[j][1] - v[j][0])
            if j + 1 < len(v) and v[j + 1][2] == "contour_quad_kernel":
                quad2.append(v[j + 1][1] - v[j + 1][0])
        i = j
print("per lane batch (%d batches in the window):" % len(ngen))
print("  generations (walker_long_kernel launches)  %s" % (", ".join("%d: %d batches" % kv for kv in sorted(collections.Counter(ngen).items()))))
print("  late span      %s" % stats(span))
if span:
    print("  beside it      mean kernels of other streams %.2f; two or more during %.1f %% of it (worst batch %.1f %%)"
          % (sum(mean_beside) / len(mean_beside), 100.0 * sum(two_share) / len(two_share), 100.0 * max(two_share)))
for k, d in sorted(quad.items()):
    print("  %-14s %s" % (k.replace("_kernel", ""), stats(d)))
print("  second quad    %s" % stats(quad2))
