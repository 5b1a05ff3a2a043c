"""The batched device-resident bsearch (include/ellhip_batch_bsearch.h) beside two baselines: one JSON
line per (n, B, space).

  python tools/batch_bsearch_bench.py [--n 2,5,16] [--batches 1024,16384,262144] [--spaces ell,stable] [--reps 20]
                                      [--warmup 3] [--host-reps 3] [--out FILE]

Workload (tests/batch_bsearch_reference.py: family): the first 40 members of the seeded family repeated to B, whole solves
from new_with_scalar(100, xc0) over the interval (-50, 50) with outer options (2000, 1e-8) and inner options (2000, 1e-8).

  (a) device  ellhip_batch_linfeas_bsearch (or _stable): host clock around the whole call (state up, the launches, the
              result copies); median of --reps calls after --warmup calls, with min and max.
  (b) host    the host-driven form a user has with ellhip_batch_linfeas_feas alone: bisection in numpy, each probe a fresh
              batch handle built from the getters, then set_target, feas, set_xc.  Median of --host-reps calls after one.
  (c) cpu     tools/batch_bsearch_cpu.cpp: one CPU thread over the 40 distinct members (best of its passes), scaled by
              nothing: its rates are per second of one thread.

The three forms must agree in every bit of feasible, niter, upper and rounds before a rate is printed.  The clone's share of
a call is given as computed bytes: 8 n^2 per probe and problem."""
from __future__ import annotations

import argparse
import json
import os
import statistics
import struct
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

DISTINCT = 40
INNER = (2000, 1e-8)
CPU_PASSES = 3


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.int64)


def new_handles(pkg, stable, a, c, xc0, kappa):
    cls = pkg.EllStableBatch if stable else pkg.EllBatch
    return cls.new_with_scalar(np.full(xc0.shape[0], kappa), xc0, device=0), pkg.BatchLinFeasProblem(a, c, device=0)


def device_run(pkg, ref, stable, a, c, xc0):
    batch, prob = new_handles(pkg, stable, a, c, xc0, ref.KAPPA)
    batch.synchronize()
    t0 = time.perf_counter()
    feasible, niter, upper, rounds, ends = prob.bsearch(batch, *ref.INTERVAL, *INNER, *ref.OUTER)
    return time.perf_counter() - t0, (feasible.astype(np.int64), niter, upper, rounds)


def host_run(pkg, ref, stable, a, c, xc0):
    batch, prob = new_handles(pkg, stable, a, c, xc0, ref.KAPPA)
    batch.synchronize()
    B, cls = batch.B, type(batch)
    lower, upper = np.full(B, ref.INTERVAL[0]), np.full(B, ref.INTERVAL[1])
    u_orig, rounds, niter_out = upper.copy(), np.zeros(B, np.int64), ref.OUTER[0]
    t0 = time.perf_counter()
    for niter in range(ref.OUTER[0]):
        tau = (upper - lower) / 2.0
        stop = tau < ref.OUTER[1]
        assert stop.all() or not stop.any()
        if stop.all():
            niter_out = niter
            break
        gamma = lower + tau
        probe = cls.new_with_matrix(batch.kappa, batch.mq, batch.xc(), device=0)
        prob.set_target(gamma)
        x, has, k, _ = prob.feas(probe, *INNER)
        has = has.astype(bool)
        rounds += k + (k < INNER[0])
        batch.set_xc(np.where(has[:, None], x, batch.xc()))
        upper = np.where(has, gamma, upper)
        lower = np.where(has, lower, gamma)
    dt = time.perf_counter() - t0
    return dt, ((upper != u_orig).astype(np.int64), np.full(B, niter_out, np.int64), upper, rounds)


def cpu_run(pkg, ref, stable, n, D):
    from oracle import oracle as O
    O.lib()  # builds oracle/libell_oracle.so when needed
    odir = os.path.join(ROOT, "oracle")
    a, c, xc0 = ref.tables(n, D)
    J = a.shape[1]
    with tempfile.TemporaryDirectory() as tmp:
        exe, fin, fout = (os.path.join(tmp, f) for f in ("batch_bsearch_cpu", "in.bin", "out.bin"))
        subprocess.check_call(["g++", "-std=c++17", "-O2", "-ffp-contract=off", "-I", odir, "-o", exe,
                               os.path.join(ROOT, "tools", "batch_bsearch_cpu.cpp"), "-L" + odir, "-lell_oracle",
                               "-Wl,-rpath," + odir, "-lm"])
        with open(fin, "wb") as f:
            f.write(struct.pack("<7q5d", D, n, J, int(stable), CPU_PASSES, INNER[0], ref.OUTER[0], INNER[1], ref.OUTER[1],
                                ref.INTERVAL[0], ref.INTERVAL[1], ref.KAPPA))
            for b in range(D):
                f.write(a[b].tobytes() + c[b].tobytes() + xc0[b].tobytes())
        line = json.loads(subprocess.run([exe, fin, fout], check=True, capture_output=True, text=True).stdout)
        raw = np.fromfile(fout, dtype=np.float64).reshape(D, 4)
    return line, (raw[:, 0].astype(np.int64), raw[:, 1].astype(np.int64), raw[:, 2].copy(), raw[:, 3].astype(np.int64))


def same(what, got, want):
    for name, u, v in zip(("feasible", "niter", "upper", "rounds"), got, want):
        eq = np.array_equal(bits(u), bits(v)) if u.dtype == np.float64 else np.array_equal(u, v)
        assert eq, f"device and {what} disagree ({name})"


def bench(pkg, ref, n, B, stable, args):
    D = min(DISTINCT, B)
    cpu, cpu_res = cpu_run(pkg, ref, stable, n, D)
    which = np.arange(B) % D
    a, c, xc0 = (np.ascontiguousarray(t[which]) for t in ref.tables(n, D))
    times = []
    for rep in range(args.warmup + args.reps):
        dt, mine = device_run(pkg, ref, stable, a, c, xc0)
        if rep >= args.warmup:
            times.append(dt)
    same("CPU", mine, tuple(r[which] for r in cpu_res))
    host_times = []
    for rep in range(1 + args.host_reps):
        dt, theirs = host_run(pkg, ref, stable, a, c, xc0)
        if rep >= 1:
            host_times.append(dt)
    same("host-driven form", mine, theirs)
    probes, rounds = int(mine[1].sum()), int(mine[3].sum())
    med, host = statistics.median(times), statistics.median(host_times)
    return {"bench": "batch_bsearch", "n": n, "J": int(a.shape[1]), "B": B, "space": "stable" if stable else "ell",
            "distinct": D, "probes": probes, "rounds": rounds, "rounds_max": int(mine[3].max()),
            "device_s": {"median": med, "min": min(times), "max": max(times), "reps": len(times)},
            "device_probes_per_s": probes / med, "device_rounds_per_s": rounds / med,
            "host_s": {"median": host, "min": min(host_times), "max": max(host_times), "reps": len(host_times)},
            "host_probes_per_s": probes / host, "host_rounds_per_s": rounds / host, "over_host": host / med,
            "cpu_probes_per_s": cpu["probes_per_s"], "cpu_rounds_per_s": cpu["rounds_per_s"],
            "over_cpu_one_thread": (rounds / med) / cpu["rounds_per_s"], "clone_bytes": 8 * n * n * probes}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", default="2,5,16")
    ap.add_argument("--batches", default="1024,16384,262144")
    ap.add_argument("--spaces", default="ell,stable")
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--host-reps", type=int, default=3)
    ap.add_argument("--out", default=None, help="append the JSON lines to this file as well")
    args = ap.parse_args()
    import ellalgo_rs_amd as pkg
    import batch_bsearch_reference as ref
    if pkg.capi.load().ellhip_device_count() <= 0:
        raise SystemExit("no HIP device: the batched bsearch has no CPU path")
    for n in (int(v) for v in args.n.split(",")):
        for space in args.spaces.split(","):
            for B in (int(v) for v in args.batches.split(",")):
                line = json.dumps(bench(pkg, ref, n, B, space == "stable", args))
                print(line, flush=True)
                if args.out:
                    with open(args.out, "a") as f:
                        f.write(line + "\n")


if __name__ == "__main__":
    main()
