"""The batched device-resident bsearch (include/ellhip_batch_bsearch.h; on streamed handles
include/ellhip_batch_bsearch_streamed.h, section 9.15) beside two baselines: one JSON line per (n, B, space).

  python tools/batch_bsearch_bench.py [--engine lds|streamed] [--n 2,5,16] [--batches 1024,16384,262144]
                                      [--shapes 129:1536,256:512,1024:256] [--spaces ell,stable | --space stable]
                                      [--reps 20] [--warmup 3] [--host-reps 3] [--out FILE]

Workload (tests/batch_bsearch_reference.py: family): the first 40 members of the seeded family repeated to B, whole solves
from new_with_scalar(100, xc0).  --engine lds: every n of --n at every B of --batches, over the interval (-50, 50) with outer
options (2000, 1e-8) and inner options (2000, 1e-8).  --engine streamed: the (n, B) pairs of --shapes on streamed handles;
with (-50, 50) every probe of the family is feasible at once from n = 64 up, so these take the intervals and options of
tests/batch_bsearch_streamed_cases.py, which straddle the optimum: (-400, 0) with inner (40, 1e-8) and outer (10, 1e-8) up
to n = 192, (-600, 0) with (40, 1e-8) and (8, 1e-8) up to n = 512, (-3000, 0) with (10, 1e-8) and (5, 1e-8) above.

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
CPU_PASSES = 3


class Work:
    """the options of one solve and the engine it runs on"""

    def __init__(self, ref, n, streamed):
        self.streamed = streamed
        if not streamed:
            self.interval, self.inner, self.outer = ref.INTERVAL, (2000, 1e-8), ref.OUTER
        elif n <= 192:
            self.interval, self.inner, self.outer = (-400.0, 0.0), (40, 1e-8), (10, 1e-8)
        elif n <= 512:
            self.interval, self.inner, self.outer = (-600.0, 0.0), (40, 1e-8), (8, 1e-8)
        else:
            self.interval, self.inner, self.outer = (-3000.0, 0.0), (10, 1e-8), (5, 1e-8)


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.int64)


def new_handles(pkg, work, stable, a, c, xc0, kappa):
    if work.streamed:
        cls = pkg.EllStableBatchStreamed if stable else pkg.EllBatchStreamed
        prob = pkg.BatchLinFeasProblem.streamed(a, c, device=0)
    else:
        cls = pkg.EllStableBatch if stable else pkg.EllBatch
        prob = pkg.BatchLinFeasProblem(a, c, device=0)
    return cls.new_with_scalar(np.full(xc0.shape[0], kappa), xc0, device=0), prob


def device_run(pkg, ref, work, stable, a, c, xc0):
    batch, prob = new_handles(pkg, work, stable, a, c, xc0, ref.KAPPA)
    batch.synchronize()
    t0 = time.perf_counter()
    feasible, niter, upper, rounds, ends = prob.bsearch(batch, *work.interval, *work.inner, *work.outer)
    return time.perf_counter() - t0, (feasible.astype(np.int64), niter, upper, rounds)


def host_run(pkg, ref, work, stable, a, c, xc0):
    batch, prob = new_handles(pkg, work, stable, a, c, xc0, ref.KAPPA)
    batch.synchronize()
    B, cls = batch.B, type(batch)
    INNER = work.inner
    lower, upper = np.full(B, work.interval[0]), np.full(B, work.interval[1])
    u_orig, rounds, niter_out = upper.copy(), np.zeros(B, np.int64), work.outer[0]
    t0 = time.perf_counter()
    for niter in range(work.outer[0]):
        tau = (upper - lower) / 2.0
        stop = tau < work.outer[1]
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


def cpu_run(pkg, ref, work, stable, n, D):
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
            f.write(struct.pack("<7q5d", D, n, J, int(stable), CPU_PASSES, work.inner[0], work.outer[0], work.inner[1],
                                work.outer[1], work.interval[0], work.interval[1], ref.KAPPA))
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
    work = Work(ref, n, args.engine == "streamed")
    cpu, cpu_res = cpu_run(pkg, ref, work, stable, n, D)
    which = np.arange(B) % D
    a, c, xc0 = (np.ascontiguousarray(t[which]) for t in ref.tables(n, D))
    times = []
    for rep in range(args.warmup + args.reps):
        dt, mine = device_run(pkg, ref, work, stable, a, c, xc0)
        if rep >= args.warmup:
            times.append(dt)
    same("CPU", mine, tuple(r[which] for r in cpu_res))
    host_times = []
    for rep in range(1 + args.host_reps):
        dt, theirs = host_run(pkg, ref, work, stable, a, c, xc0)
        if rep >= 1:
            host_times.append(dt)
    same("host-driven form", mine, theirs)
    probes, rounds = int(mine[1].sum()), int(mine[3].sum())
    med, host = statistics.median(times), statistics.median(host_times)
    return {"bench": "batch_bsearch", "engine": args.engine, "interval": work.interval, "inner": work.inner,
            "outer": work.outer, "n": n, "J": int(a.shape[1]), "B": B, "space": "stable" if stable else "ell",
            "distinct": D, "probes": probes, "rounds": rounds, "rounds_max": int(mine[3].max()),
            "device_s": {"median": med, "min": min(times), "max": max(times), "reps": len(times)},
            "device_probes_per_s": probes / med, "device_rounds_per_s": rounds / med,
            "host_s": {"median": host, "min": min(host_times), "max": max(host_times), "reps": len(host_times)},
            "host_probes_per_s": probes / host, "host_rounds_per_s": rounds / host, "over_host": host / med,
            "cpu_probes_per_s": cpu["probes_per_s"], "cpu_rounds_per_s": cpu["rounds_per_s"],
            "over_cpu_one_thread": (rounds / med) / cpu["rounds_per_s"], "clone_bytes": 8 * n * n * probes}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--engine", choices=("lds", "streamed"), default="lds")
    ap.add_argument("--shapes", default="129:1536,256:512,1024:256", help="--engine streamed: n:B pairs")
    ap.add_argument("--space", default=None, help="one space; overrides --spaces")
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
    if args.engine == "streamed":
        shapes = [tuple(int(v) for v in pair.split(":")) for pair in args.shapes.split(",")]
    else:
        shapes = [(int(n), int(B)) for n in args.n.split(",") for B in args.batches.split(",")]
    spaces = [args.space] if args.space else args.spaces.split(",")
    for n in dict.fromkeys(n for n, _ in shapes):
        for space in spaces:
            for B in (B for m, B in shapes if m == n):
                line = json.dumps(bench(pkg, ref, n, B, space == "stable", args))
                print(line, flush=True)
                if args.out:
                    with open(args.out, "a") as f:
                        f.write(line + "\n")


if __name__ == "__main__":
    main()
