#!/usr/bin/env python3
"""Reads a rocprofv3 kernel trace (csv) of bench.py and reports, per hardware queue, which streams and kernels ran on it, whether the
range coder (k_rcs) shares a queue with anything else, and how long front-end streams stood still while a k_rcs of another stream
was in flight on their own queue.  usage: trace_queues.py DIR_OR_CSV [label]"""
import collections
import csv
import glob
import os
import sys

src = sys.argv[1]
label = sys.argv[2] if len(sys.argv) > 2 else src
files = [src] if os.path.isfile(src) else sorted(glob.glob(os.path.join(src, "**", "*kernel_trace.csv"), recursive=True))
if not files:
    sys.exit(f"no kernel trace under {src}")
rows = []
for f in files:
    with open(f, newline="") as fh:
        for r in csv.DictReader(fh):
            rows.append(r)
cols = list(rows[0].keys())
has_stream = "Stream_Id" in cols
K = []
for r in rows:
    name = r["Kernel_Name"].replace("(anonymous namespace)::", "").replace("void ", "").split("(")[0].split(" [")[0].strip()
    K.append((int(r["Start_Timestamp"]), int(r["End_Timestamp"]), r["Queue_Id"], r["Stream_Id"] if has_stream else "?", name))
K.sort()
is_rc = lambda n: n.startswith("k_rcs")
rcs = [k for k in K if is_rc(k[4])]
print(f"== {label}: {len(K)} kernels, {len(rcs)} k_rcs launches, columns {cols}")
if not rcs:
    sys.exit(0)
# the timed region: after the warm-up's launches (one per instance; instances = distinct streams with a k_rcs, else 4)
n_inst = len({k[3] for k in rcs}) if has_stream else 4
t0 = sorted(k[1] for k in rcs)[n_inst - 1] if len(rcs) > n_inst else K[0][0]
t1 = max(k[1] for k in K)
W = [k for k in K if k[0] >= t0]
n_steps = max(1, sum(1 for k in W if is_rc(k[4])) // n_inst)
print(f"timed window {(t1 - t0) / 1e6:.1f} ms, {n_inst} instances, {n_steps} steps -> {(t1 - t0) / 1e6 / n_steps:.1f} ms per step")
byq = collections.defaultdict(list)
for k in W:
    byq[k[2]].append(k)
rc_queues = {k[2] for k in W if is_rc(k[4])}
print("-- queues")
for q in sorted(byq, key=lambda x: int(x) if x.isdigit() else 0):
    ks = byq[q]
    streams = sorted({k[3] for k in ks})
    rc_streams = sorted({k[3] for k in ks if is_rc(k[4])})
    names = collections.Counter(k[4] for k in ks)
    top = ", ".join(f"{n} x{c}" for n, c in names.most_common(6))
    busy = sum(k[1] - k[0] for k in ks) / 1e6
    print(f"queue {q}: streams {streams} (k_rcs from {rc_streams}); {len(ks)} kernels, {busy:.0f} ms of kernel time; {top}")
shared = [q for q in rc_queues if any(not is_rc(k[4]) for k in byq[q])]
print(f"k_rcs queues: {sorted(rc_queues)}; shared with other kernels: {sorted(shared) if shared else 'none'}")
# gaps: on each queue, in each front-end stream (all kernels but k_rcs), the time between one kernel's end and the next one's start
# that falls inside a k_rcs of ANOTHER stream on the SAME queue; and inside any k_rcs at all (what an instance waits for its own coder is in there)
tot_same = 0.0; tot_gap = 0.0
all_rc = [(k[0], k[1], k[2], k[3]) for k in W if is_rc(k[4])]


def overlap(a, b, ivs):
    s = 0
    for x, y in ivs:
        lo, hi = max(a, x), min(b, y)
        if hi > lo:
            s += hi - lo
    return s


print("-- front-end streams: gaps of more than 1 ms between consecutive kernels")
fe = collections.defaultdict(list)
own_id = {}
for k in W:
    if not is_rc(k[4]):
        fe[(k[2], k[3])].append(k)
for (q, s), ks in sorted(fe.items()):
    if len(ks) < 50:
        continue
    ks.sort()
    same = [(a, b) for a, b, qq, ss in all_rc if qq == q and ss != s]
    own = [(a, b) for a, b, qq, ss in all_rc if ss == s or (not has_stream and qq == q)]
    other = [(a, b) for a, b, qq, ss in all_rc if ss != s]
    g_tot = g_same = g_other = g_own = 0
    for i in range(len(ks) - 1):
        a, b = ks[i][1], ks[i + 1][0]
        if b - a > 1_000_000:
            # the instance's own coder: the k_rcs that starts within 2 ms of this gap's start; waiting for it is the algorithm's
            mine = [r for r in all_rc if 0 <= r[0] - a < 2_000_000 or (r[0] <= a < r[1] and (r[2], r[3]) == own_id.get((q, s)))]
            a2 = a
            if mine:
                own_id[(q, s)] = (mine[0][2], mine[0][3]); a2 = min(b, max(a, mine[0][1])); g_own += a2 - a
            g_tot += b - a
            if b > a2:
                g_same += min(b - a2, overlap(a2, b, [(x, y) for x, y, qq, ss in all_rc if qq == q and ss != s and not (mine and (x, y, qq, ss) == mine[0])]))
                g_other += min(b - a2, overlap(a2, b, [(x, y) for x, y, qq, ss in all_rc if not (mine and (x, y, qq, ss) == mine[0])]))
    print(f"queue {q} stream {s}: {len(ks)} kernels; gaps {g_tot / 1e6 / n_steps:.1f} ms/step: {g_own / 1e6 / n_steps:.1f} waiting for the instance's own k_rcs, "
          f"after that {g_same / 1e6 / n_steps:.1f} under a foreign k_rcs ON THIS QUEUE ({g_other / 1e6 / n_steps:.1f} under a foreign k_rcs anywhere)")
    tot_same += g_same; tot_gap += g_tot
print(f"sum over front-end streams: gaps {tot_gap / 1e6 / n_steps:.1f} ms/step, behind another stream's k_rcs on the same queue {tot_same / 1e6 / n_steps:.1f} ms/step")
# how much of the window has no front-end kernel running at all
iv = sorted((k[0], k[1]) for k in W if not is_rc(k[4]))
cov = 0; cur_a, cur_b = iv[0]
for a, b in iv[1:]:
    if a > cur_b:
        cov += cur_b - cur_a; cur_a, cur_b = a, b
    else:
        cur_b = max(cur_b, b)
cov += cur_b - cur_a
print(f"no front-end kernel of any instance running: {(t1 - t0 - cov) / 1e6 / n_steps:.1f} ms per step of {(t1 - t0) / 1e6 / n_steps:.1f}")
rc_ms = [(k[1] - k[0]) / 1e6 for k in W if is_rc(k[4])]
print(f"k_rcs: {len(rc_ms)} launches, mean {sum(rc_ms) / len(rc_ms):.1f} ms, min {min(rc_ms):.1f}, max {max(rc_ms):.1f}")
