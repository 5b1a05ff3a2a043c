#!/usr/bin/env python3
"""Launches per iteration and the share of skipped station slots of the device-resident LMI loop, from a rocprofv3 kernel
trace of `tests/cpp/_build/lmi_loop_runner_hip device <n> <m> <J> <optim|feas> <iters>` (a run of its own):

  rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- tests/cpp/_build/lmi_loop_runner_hip device 24 300 2 optim 200 > RUN.json
  python tools/lmi_loop_trace.py DIR --active-slots N        (N = "active_block_slots" of the runner's JSON line)

The runner first runs the host-driven loop, whose walk is the device loop's to the bit, and prints how many block calls it
made: that is the exact number N of block slots of the device loop that were not skipped.  A block slot is the run of
kernels from a k_ll_gate to the next k_ll_station; the trace does not show the gate's verdict, so the N slots whose
k_ldlt_diag kernels took longest in total are taken as the active ones (a skipped slot's are empty launches), and the
line reports the two durations on either side of that cut (`diag_us_last_active`, `diag_us_first_skipped`) so that a
cut through a dense region shows.  Iterations are counted by k_ll_close.  Prints one JSON line."""
import argparse
import csv
import glob
import json
import os
import sys

ap = argparse.ArgumentParser()
ap.add_argument("dir")
ap.add_argument("--active-slots", type=int, required=True)
args = ap.parse_args()
rows = []
for f in glob.glob(os.path.join(args.dir, "**", "*kernel_trace.csv"), recursive=True):
    for r in csv.DictReader(open(f)):
        name = r["Kernel_Name"]
        if "ellhip::" not in name:
            continue
        rows.append((int(r["Start_Timestamp"]), int(r["End_Timestamp"]), name.split("ellhip::")[1].split("(")[0].split("<")[0]))
rows.sort()
gates = [i for i, r in enumerate(rows) if r[2] == "k_ll_gate"]
closes = [i for i, r in enumerate(rows) if r[2] == "k_ll_close"]
if not gates or not closes or closes[-1] < gates[0]:
    sys.exit(f"no device loop in the trace under {args.dir} ({len(rows)} ellhip kernels)")
loop = rows[gates[0]:closes[-1] + 1]
iters = sum(1 for r in loop if r[2] == "k_ll_close")
busy = sum(e - s for s, e, _ in loop)
span = loop[-1][1] - loop[0][0]
groups = []
i = 0
while i < len(loop):
    if loop[i][2] != "k_ll_gate":
        i += 1
        continue
    j = i
    while j < len(loop) and loop[j][2] != "k_ll_station":
        j += 1
    if j == len(loop):
        break  # a truncated slot at the end of the trace
    groups.append(loop[i:j + 1])
    i = j + 1
if not 0 <= args.active_slots <= len(groups):
    sys.exit(f"--active-slots {args.active_slots} but the trace has {len(groups)} block slots")
diag = [sum(e - s for s, e, nm in g if nm == "k_ldlt_diag") for g in groups]
order = sorted(range(len(groups)), key=lambda k: -diag[k])
skipped = [groups[k] for k in order[args.active_slots:]]
skip_busy = sum(e - s for g in skipped for s, e, _ in g)
skip_span = sum(g[-1][1] - g[0][0] for g in skipped)
skip_launches = sum(len(g) for g in skipped)
print(json.dumps({
    "trace": "lmi_loop", "iterations_enqueued": iters, "kernel_launches": len(loop),
    "launches_per_iteration": round(len(loop) / iters, 2), "block_slots": len(groups), "active_block_slots": args.active_slots,
    "skipped_block_slots": len(skipped), "launches_in_skipped_slots_share": round(skip_launches / len(loop), 4),
    "kernel_time_us": round(busy / 1e3, 1), "skipped_kernel_time_share": round(skip_busy / busy, 4),
    "loop_span_us": round(span / 1e3, 1), "skipped_span_share": round(skip_span / span, 4),
    "diag_us_last_active": round(diag[order[args.active_slots - 1]] / 1e3, 2) if args.active_slots else None,
    "diag_us_first_skipped": round(diag[order[args.active_slots]] / 1e3, 2) if skipped else None}))
