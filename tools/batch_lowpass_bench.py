"""The batched device-resident low-pass design loop against the two other ways to solve the same instances: one JSON line.

  python tools/batch_lowpass_bench.py [--shapes 16:16384,32:4096,32:65536,64:1024] [--reps 3] [--warmup 1]
                                      [--host-b 64] [--skip-host] [--space ell|stable]

Workload (tests/batch_lowpass_reference.py: family): B specifications of one filter length n, wp = 0.08 + 0.01 (s % 6),
ws = wp + 0.08 + 0.01 (s % 3), d = 0.02 + 0.01 (s % 6), limits ((1 - d)^2, (1 + d)^2, 0.1); Ell::new_with_scalar(40, 0),
max_iters 50000, tol 1e-14, gamma starts at sp_sq.  The family has six distinct members, so the CPU side solves six
instances and the rates below follow from them.

Per shape:
  device   ellhip_batch_lowpass_optim: host clock around the whole call (state reset, gamma up, every launch, results
           down; handles are created outside the clock); --warmup calls, then --reps timed ones, each on fresh handles.
           iterations/s = rounds / t with rounds = the oracle + update rounds the instances ran (niter + 1 for an
           instance the status or the tolerance stopped).  Median, min and max are reported.
  cpu      the CPU oracle's own loop (oracle.OracleLowpass.cutting_plane_optim over OracleEll), one thread: the six
           distinct members are timed once each and the rate is their rounds over their time (what a one-thread sweep
           over all B would run at).  rows_per_iter: row . x products per oracle call, from the CPU oracle's counter.
  host     what the engine offered before the device loop: the host computes every cut with the CPU oracle and calls
           ellhip_batch_update with K = 1 per iteration (get_xc, one oracle call per live instance, one launch; an
           instance that has stopped receives a no-op cut, beta = +inf).  On the first --host-b instances, once.
Every device result must equal the CPU's bit for bit (niter, gamma, status, x_best), and so must the host-driven form;
the tool checks it.

--space stable runs the same three forms on EllStable spaces (include/ellhip_batch_stable_loops.h): the device loop on an
EllStableBatch, the CPU oracle's loop over its EllStable, and the host-driven form over ellhip_batch_update on an
EllStableBatch (a stopped instance receives a cut that fails, beta = +inf).
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

MAX_ITERS, TOL, KAPPA = 50000, 1e-14, 40.0
STABLE = False  # --space stable


def new_batch(pkg, n, B):
    return (pkg.EllStableBatch if STABLE else pkg.EllBatch).new_with_scalar(np.full(B, KAPPA), np.zeros((B, n)), device=0)


def fresh(ref, n, consts):
    omega, space = ref.fresh(n, consts)
    if STABLE:
        space = ref.O.OracleEllStable.new_with_scalar(KAPPA, np.zeros(n))
    return omega, space


def rounds_of(niter):
    return int(np.sum(np.where(niter < MAX_ITERS, niter + 1, niter)))


def device_run(pkg, ref, n, B):
    consts = [ref.family(s) for s in range(B)]
    prob = pkg.BatchLowpassProblem(n, *ref.columns(consts), device=0)
    batch = new_batch(pkg, n, B)
    gamma0 = np.array([c[4] for c in consts])
    t0 = time.perf_counter()
    x_best, has, niter, gamma, status = prob.optim(batch, gamma0, MAX_ITERS, TOL)
    return time.perf_counter() - t0, x_best, niter, gamma, status


def cpu_run(ref, n):
    """the six distinct members, one thread -> (records, seconds, rounds, rows visited)"""
    recs, secs, rounds, rows = [], 0.0, 0, 0
    for s in range(6):
        consts = ref.family(s)
        omega, space = fresh(ref, n, consts)
        t0 = time.perf_counter()
        xb, niter, gamma, status = omega.cutting_plane_optim(space, consts[4], MAX_ITERS, TOL)
        secs += time.perf_counter() - t0
        recs.append(dict(x_best=xb, niter=niter, gamma=gamma, status=status))
        rounds += niter + 1 if niter < MAX_ITERS else niter
        # the rows the walk visits, call by call, on a second oracle (the loop above is the timed one)
        omega2, space2 = fresh(ref, n, consts)
        g2 = consts[4]
        for _ in range(rounds_of(np.array([niter]))):
            x = np.array(space2.xc)
            try:
                (g, (b0, b1)), shrunk, g2 = omega2.assess_optim(x, g2)
            except IndexError:
                break
            rows += omega2.s.rows_visited
            space2.update(1 if shrunk else 0, g, b0, b1)
    return recs, secs, rounds, rows


def host_run(pkg, ref, n, B):
    """the form that needs no device loop: CPU oracle per instance, ellhip_batch_update with K = 1 per iteration"""
    consts = [ref.family(s) for s in range(B)]
    omegas = [ref.O.OracleLowpass(n, *c) for c in consts]
    batch = new_batch(pkg, n, B)
    gamma = np.array([c[4] for c in consts])
    niter = np.full(B, MAX_ITERS, dtype=np.int64)
    live = np.ones(B, dtype=bool)
    kinds = np.zeros((1, B), dtype=np.int32)
    grads = np.ones((1, B, n))
    beta0 = np.full((1, B), math.inf)
    beta1 = np.full((1, B), math.nan)
    t0 = time.perf_counter()
    for it in range(MAX_ITERS):
        if not live.any():
            break
        xc = batch.xc()
        for b in np.flatnonzero(live):
            (g, (b0, b1)), shrunk, gamma[b] = omegas[b].assess_optim(xc[b], gamma[b])
            kinds[0, b] = 1 if shrunk else 0
            grads[0, b] = g
            beta0[0, b] = b0
            beta1[0, b] = math.nan if b1 is None else b1
        status, tsq = batch.update(kinds, grads, beta0, beta1)
        stop = live & ((status[0] != 0) | (tsq[0] < TOL))
        niter[stop] = it
        live &= ~stop
        kinds[0, stop], grads[0, stop], beta0[0, stop], beta1[0, stop] = 0, 1.0, math.inf, math.nan
    return time.perf_counter() - t0, niter, gamma


def bench(pkg, ref, n, B, reps, warmup, host_b, skip_host):
    recs, cpu_s, cpu_rounds, cpu_rows = cpu_run(ref, n)
    for _ in range(warmup):
        device_run(pkg, ref, n, B)
    times = []
    for _ in range(reps):
        dt, x_best, niter, gamma, status = device_run(pkg, ref, n, B)
        times.append(dt)
    for b in range(B):
        r = recs[b % 6]
        assert niter[b] == r["niter"] and gamma[b] == r["gamma"] and status[b] == r["status"], f"device and CPU disagree at {b}"
        if r["x_best"] is None:  # (EllStable: the family's members end NoSoln before a best point)
            assert STABLE and np.isnan(x_best[b]).all(), f"device and CPU disagree at {b}"
        else:
            assert np.array_equal(x_best[b], r["x_best"]), f"device and CPU disagree at {b}"
    rounds = rounds_of(niter)
    med = statistics.median(times)
    cpu_rate = cpu_rounds / cpu_s
    out = {"space": "stable" if STABLE else "ell", "n": n, "B": B, "niter_min": int(niter.min()), "niter_max": int(niter.max()), "rounds": rounds,
           "rows_per_iter": cpu_rows / cpu_rounds,
           "device_s": {"median": med, "min": min(times), "max": max(times), "reps": reps},
           "device_iters_per_s": rounds / med, "device_solves_per_s": B / med,
           "cpu_s_six_members": cpu_s, "cpu_iters_per_s": cpu_rate, "device_over_cpu": rounds / med / cpu_rate}
    if not skip_host:
        hb = min(B, host_b)
        host_run(pkg, ref, n, min(hb, 6))
        dt, niter_h, gamma_h = host_run(pkg, ref, n, hb)
        assert np.array_equal(niter_h, niter[:hb]) and np.array_equal(gamma_h, gamma[:hb]), "device and host-driven form disagree"
        host_rate = rounds_of(niter_h) / dt
        out.update(host_B=hb, host_s=dt, host_iters_per_s=host_rate, device_over_host=rounds / med / host_rate)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="16:16384,32:4096,32:65536,64:1024")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--host-b", type=int, default=64)
    ap.add_argument("--skip-host", action="store_true")
    ap.add_argument("--space", choices=("ell", "stable"), default="ell")
    args = ap.parse_args()
    global STABLE
    STABLE = args.space == "stable"
    import ellalgo_rs_amd as pkg
    import batch_lowpass_reference as ref
    if pkg.capi.load().ellhip_device_count() <= 0:
        raise SystemExit("no HIP device: the batched lowpass loop has no CPU path")
    res = []
    for shape in args.shapes.split(","):
        n, B = (int(v) for v in shape.split(":"))
        res.append(bench(pkg, ref, n, B, args.reps, args.warmup, args.host_b, args.skip_host))
    print(json.dumps({"bench": "batch_lowpass", "results": res}))


if __name__ == "__main__":
    main()
