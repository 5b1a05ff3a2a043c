"""The batched device-resident LMI loop against the two other ways to solve the same instances: one JSON line.

  python tools/batch_lmi_bench.py [--reps 5] [--warmup 1] [--scale 1.0] [--skip-host] [--space ell|stable]
                                  [--max-iters 2000] [--shapes]

Workloads (tests/batch_lmi_reference.py): family A, the perturbed reference problem (n = 3, blocks 2x2 and 3x3), at
B = 4096, tol 1e-20; family B (n = 16, three 12x12 blocks) at B = 1024, tol 1e-8.  Ell::new_with_scalar(10, 0),
max_iters 2000.  --scale shrinks both B for a quick look.

Per workload:
  device   ellhip_batch_lmi_optim: host clock around the whole call (state reset, gamma up, every launch, results down;
           handles are created outside the clock); --warmup calls, then --reps timed ones, each on fresh handles.
           solves/s = B / t, iterations/s = rounds / t with rounds = the oracle + update rounds the instances ran
           (niter + 1 for an instance the status or the tolerance stopped).  Median, min and max are reported.
  cpu      the same instances through the CPU helper (RoundRobinLmi + optim over the CPU oracle), one thread, once
  host     what the engine offered before the device loop: the host computes every cut with the CPU oracle and calls
           ellhip_batch_update with K = 1 per iteration (get_xc, B oracle calls, one launch; an instance that has
           stopped receives a no-op cut, beta = +inf).  Once, after a warm-up on 8 instances.
The three paths must agree bit for bit on niter and gamma; the tool checks it.

--space stable runs the same three forms on EllStable spaces (include/ellhip_batch_stable_loops.h): the device loop on an
EllStableBatch, the CPU helper over the CPU oracle's EllStable, and the host-driven form over ellhip_batch_update on an
EllStableBatch (a stopped instance receives a cut that fails, beta = +inf).  --shapes replaces the two workloads by the
table shapes n = 3 (family A), n = 16 with 12x12 blocks and n = 32 with 24x24 blocks; --max-iters caps every run.
"""
from __future__ import annotations

import argparse
import json
import math
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def new_batch(pkg, B, n, stable):
    return (pkg.EllStableBatch if stable else pkg.EllBatch).new_with_scalar(np.full(B, 10.0), np.zeros((B, n)), device=0)


def device_run(pkg, ref, problems, max_iters, tol, stable=False):
    mat_f, mat_b, c = ref.stack(problems)
    B, n = c.shape
    prob = pkg.BatchLmiProblem(mat_f, mat_b, c, device=0)
    batch = new_batch(pkg, B, n, stable)
    t0 = time.perf_counter()
    x_best, has, niter, gamma, status = prob.optim(batch, math.inf, max_iters, tol)
    return time.perf_counter() - t0, niter, gamma, status


def host_run(pkg, ref, problems, max_iters, tol, stable=False):
    """the form that needs no device loop: CPU oracle per instance, ellhip_batch_update with K = 1 per iteration"""
    B, n = len(problems), len(problems[0][2])
    omegas = [ref.RoundRobinLmi(fs, bs, c) for fs, bs, c in problems]
    batch = new_batch(pkg, B, n, stable)
    gamma = np.full(B, math.inf)
    niter = np.full(B, max_iters, dtype=np.int64)
    live = np.ones(B, dtype=bool)
    kinds = np.zeros((1, B), dtype=np.int32)
    grads = np.ones((1, B, n))
    beta = np.full((1, B), math.inf)
    t0 = time.perf_counter()
    for it in range(max_iters):
        if not live.any():
            break
        xc = batch.xc()
        for b in np.flatnonzero(live):
            (g, be), station, gamma[b] = omegas[b].assess_optim(xc[b], gamma[b])
            kinds[0, b] = 1 if station == omegas[b].J + 1 else 0
            grads[0, b] = g
            beta[0, b] = be
        status, tsq = batch.update(kinds, grads, beta)
        stop = live & ((status[0] != 0) | (tsq[0] < tol))
        niter[stop] = it
        live &= ~stop
        kinds[0, stop], grads[0, stop], beta[0, stop] = 0, 1.0, math.inf
    return time.perf_counter() - t0, niter, gamma


def cpu_run(ref, problems, max_iters, tol, stable=False):
    t0 = time.perf_counter()
    if stable:
        runs = []
        for fs, bs, c in problems:
            space = ref.O.OracleEllStable.new_with_scalar(10.0, np.zeros(len(c)))
            _, niter, gamma, _ = ref.optim(space, ref.RoundRobinLmi(fs, bs, c), math.inf, max_iters, tol)
            runs.append(dict(niter=niter, gamma=gamma))
    else:
        runs, _, _ = ref.run_optim(problems, max_iters, tol)
    dt = time.perf_counter() - t0
    return dt, np.array([r["niter"] for r in runs], dtype=np.int64), np.array([r["gamma"] for r in runs])


def rounds_of(niter, max_iters):
    return int(np.sum(np.where(niter < max_iters, niter + 1, niter)))


def bench(pkg, ref, name, problems, max_iters, tol, reps, warmup, skip_host, stable=False):
    B = len(problems)
    for _ in range(warmup):
        device_run(pkg, ref, problems, max_iters, tol, stable)
    times = []
    for _ in range(reps):
        dt, niter, gamma, status = device_run(pkg, ref, problems, max_iters, tol, stable)
        times.append(dt)
    rounds = rounds_of(niter, max_iters)
    med = statistics.median(times)
    out = {"workload": name, "space": "stable" if stable else "ell", "max_iters": max_iters, "B": B, "n": len(problems[0][2]), "m": [int(f.shape[1]) for f in problems[0][0]],
           "tol": tol, "niter_min": int(niter.min()), "niter_max": int(niter.max()), "rounds": rounds,
           "device_s": {"median": med, "min": min(times), "max": max(times), "reps": reps},
           "device_solves_per_s": B / med, "device_iters_per_s": rounds / med}
    dt, niter_c, gamma_c = cpu_run(ref, problems, max_iters, tol, stable)
    assert np.array_equal(niter_c, niter) and np.array_equal(gamma_c, gamma), "device loop and CPU helper disagree"
    out.update(cpu_s=dt, cpu_solves_per_s=B / dt, cpu_iters_per_s=rounds / dt)
    if not skip_host:
        host_run(pkg, ref, problems[:8], max_iters, tol, stable)
        dt, niter_h, gamma_h = host_run(pkg, ref, problems, max_iters, tol, stable)
        assert np.array_equal(niter_h, niter) and np.array_equal(gamma_h, gamma), "device loop and host-driven form disagree"
        out.update(host_s=dt, host_solves_per_s=B / dt, host_iters_per_s=rounds / dt, device_over_host=dt / med)
    out["device_over_cpu"] = out["cpu_s"] / med
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--scale", type=float, default=1.0)
    ap.add_argument("--skip-host", action="store_true")
    ap.add_argument("--space", choices=("ell", "stable"), default="ell")
    ap.add_argument("--max-iters", type=int, default=2000)
    ap.add_argument("--shapes", action="store_true")
    args = ap.parse_args()
    stable, mi = args.space == "stable", args.max_iters
    import ellalgo_rs_amd as pkg
    import batch_lmi_reference as ref
    if pkg.capi.load().ellhip_device_count() <= 0:
        raise SystemExit("no HIP device: the batched LMI loop has no CPU path")
    ba, bb = max(1, int(4096 * args.scale)), max(1, int(1024 * args.scale))
    work = [("family_a", [ref.family_a(s) for s in range(ba)], 1e-20),
            ("family_b_16_12_3", [ref.family_b(s, 16, 12, 3) for s in range(bb)], 1e-8)]
    if args.shapes:
        work.append(("family_b_32_24_2", [ref.family_b(s, 32, 24, 2) for s in range(bb)], 1e-6))
    res = [bench(pkg, ref, name, problems, mi, tol, args.reps, args.warmup, args.skip_host, stable)
           for name, problems, tol in work]
    print(json.dumps({"bench": "batch_lmi", "results": res}))


if __name__ == "__main__":
    main()
