#!/usr/bin/env python3
"""What the walker fork's two event hops cost, from a rocprofv3 kernel trace of the pipelined bench (tools/trace_overlap.sh).

Per main stream (a stream that runs threshold kernels) the kernels in start order; the side stream that belongs to it is the one whose
kernels all lie between a snapshot_kernel's end and the start of the second contour_quad_kernel behind it. Per batch, steady-state window:
  snapshot gap   start of snapshot_kernel - end of the kernel in front of it in its stream (an ordinary in-stream gap, for comparison)
  fork hop       start of the first late walker_long_kernel (side stream) - end of snapshot_kernel (where the fork event is recorded)
  late chain     end of the last late generation - start of the first
  join gap       start of contour_quad pass 2 - max(end of pass 1, end of the last late generation)
  pass-1 slack   end of the last late generation - end of pass 1 (> 0: the main stream sits waiting for the side stream that long)
and, for every build, the in-stream gap in front of every kernel kind (median / mean / p90). A build without the fork has no snapshot_kernel
and one contour_quad_kernel per batch; only the in-stream table is printed for it. Usage: fork_gap_summarize.py kernel_trace.csv"""
import collections
import csv
import statistics
import sys


def short(name):
    return name.split("(")[0].replace("void ", "").replace("ah::", "").split("<")[0]


def stats(v):
    v = sorted(v)
    if not v:
        return "n 0"
    return "n %4d  median %8.1f  mean %8.1f  p90 %8.1f  max %8.1f us" % (len(v), statistics.median(v) / 1e3, sum(v) / len(v) / 1e3, v[int(0.9 * (len(v) - 1))] / 1e3, v[-1] / 1e3)


rows = list(csv.DictReader(open(sys.argv[1])))
key = "Stream_Id" if rows and "Stream_Id" in rows[0] and len(set(r["Stream_Id"] for r in rows)) > 1 else "Queue_Id"
print("streams told apart by %s%s" % (key, "" if key == "Stream_Id" else " (no stream ids in this trace: streams that share a hardware queue are merged, figures are approximate)"))
streams = collections.defaultdict(list)
for r in rows:
    streams[r[key]].append((int(r["Start_Timestamp"]), int(r["End_Timestamp"]), short(r["Kernel_Name"])))
for v in streams.values():
    v.sort()
mains = {s: v for s, v in streams.items() if any("threshold" in k for _, _, k in v)}
sides = {s: v for s, v in streams.items() if s not in mains and all(k == "walker_long_kernel" for _, _, k in v)}
thr = sorted(st for v in mains.values() for st, _, k in v if "threshold" in k)
lo, hi = thr[len(thr) // 4], thr[(3 * len(thr)) // 4]
print("%d main streams, %d side streams, %d other; steady-state window %.3f ms" % (len(mains), len(sides), len(streams) - len(mains) - len(sides), (hi - lo) / 1e6))

# in-stream gap in front of every kernel kind (same stream, previous kernel's end -> this start; the first kernel of a batch is left out)
gaps = collections.defaultdict(list)
for v in mains.values():
    for (s0, e0, k0), (s1, e1, k1) in zip(v, v[1:]):
        if lo <= s1 < hi and "threshold" not in k1 and not k1.startswith("__amd_rocclr_fill"):
            gaps[k1].append(s1 - e0)
print("in-stream gap in front of a kernel (main streams):")
for k, g in sorted(gaps.items()):
    print("  %-28s %s" % (k, stats(g)))

batches = []   # (main, snapshot index)
for m, v in mains.items():
    for i, (s, e, k) in enumerate(v):
        if k == "snapshot_kernel" and lo <= s < hi:
            cq = [j for j in range(i + 1, min(i + 4, len(v))) if v[j][2] == "contour_quad_kernel"]
            if len(cq) >= 2:
                batches.append((m, i, cq[0], cq[1]))
if not batches:
    print("no snapshot_kernel in the window: this build does not fork; contour_quad_kernel launches per threshold launch: %.2f"
          % (sum(1 for v in mains.values() for s, _, k in v if k == "contour_quad_kernel" and lo <= s < hi) / max(1, sum(1 for t in thr if lo <= t < hi))))
    sys.exit(0)
# the side stream of each main stream
pair = {}
for m, v in mains.items():
    wins = [(v[i][1], v[p2][0]) for mm, i, p1, p2 in batches if mm == m]
    best = None
    for x, xv in sides.items():
        inside = sum(1 for s, e, _ in xv if any(a <= s and e <= b for a, b in wins))
        span = sum(1 for s, e, _ in xv if wins and wins[0][0] <= s <= wins[-1][1])
        if span and (best is None or inside / span > best[0]):
            best = (inside / span, x, inside, span)
    if best:
        pair[m] = best[1]
        print("  main %s <- side %s (%d of its %d launches inside this stream's fork..join windows)" % (m, best[1], best[2], best[3]))
snap_gap, fork_hop, chain, join_gap, slack, nlate = [], [], [], [], [], []
for m, i, p1, p2 in batches:
    v = mains[m]
    S, P1, P2 = v[i], v[p1], v[p2]
    late = [(s, e) for s, e, _ in sides.get(pair.get(m), []) if S[1] <= s and e <= P2[0]]
    snap_gap.append(S[0] - v[i - 1][1])
    if not late:
        continue
    nlate.append(len(late))
    fork_hop.append(late[0][0] - S[1])
    chain.append(late[-1][1] - late[0][0])
    join_gap.append(P2[0] - max(P1[1], late[-1][1]))
    slack.append(late[-1][1] - P1[1])
print("per batch with a fork (%d batches, %.1f late walker_long launches each):" % (len(batches), sum(nlate) / max(1, len(nlate))))
print("  snapshot gap  %s" % stats(snap_gap))
print("  fork hop      %s" % stats(fork_hop))
print("  late chain    %s" % stats(chain))
print("  join gap      %s" % stats(join_gap))
print("  pass-1 slack  %s   (batches in which the main stream waited for the side stream: %d)" % (stats(slack), sum(1 for x in slack if x > 0)))
