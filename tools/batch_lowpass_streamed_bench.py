"""The batched device-resident low-pass design loop on a streamed batch handle (include/ellhip_batch_lowpass_streamed.h)
against the two other ways to run the same sweep at filter lengths past 128: one JSON line per shape.

  python tools/batch_lowpass_streamed_bench.py [--space ell|stable] [--shapes 129:1536:300,256:1536:200,512:768:150,1024:256:100]
                                               [--reps 3] [--warmup 1] [--host-b 16] [--chunks 256] [--out FILE]

A shape is n:B:max_iters.  Workload (tests/batch_lowpass_reference.py: family): B specifications of one filter length n,
wp = 0.08 + 0.01 (s % 6), ws = wp + 0.08 + 0.01 (s % 3), d = 0.02 + 0.01 (s % 6), limits ((1 - d)^2, (1 + d)^2, 0.1);
Ell::new_with_scalar(40, 0), tol 1e-14, gamma starts at sp_sq, cut off at max_iters so that a call lasts seconds.  The
family has six distinct members, so the CPU side solves six instances.

Three forms, run alternately (device, cpu, host, device, ...) --warmup times unrecorded and then --reps times:
  device   ellhip_batch_lowpass_optim_streamed: host clock around the whole call (state reset, gamma up, every launch,
           results down) on fresh spaces; the oracle handle is made once per shape (its table is 2 * 15 n^2 * 8 bytes) and
           reset between calls.  One entry per value of --chunks (iterations per launch: with 1 no sweep carries the next
           product, so chunk 1 against chunk 256 is the gain of the fused order).
  cpu      the CPU oracle's own loop (oracle.OracleLowpass.cutting_plane_optim over OracleEll), one thread, the six members
           one after the other; the clock excludes building the oracles.
  host     the form a streamed handle offered before: the host computes every cut with the CPU oracle and calls
           ellhip_batch_update with K = 1 per iteration (get_xc, one oracle call per live instance, one launch of 24 n^2
           bytes per instance), on the first --host-b instances.
Rates are rounds per second, rounds = the oracle + update rounds the instances ran.  Before anything is timed the device
result (every chunk) and the host-driven result must equal the CPU's bit for bit: niter, gamma, status, x_best.

rows_per_iter: row . x products per oracle call, from the CPU oracle's counter, averaged over the six members.  Byte model
per instance and round: 16 n^2 (+ 8 n^2 once per launch) of matrix, 8 n per visited row of the transposed table, 8 n for the
gradient row; model_bytes_per_round and the bandwidth the measured device rate implies under it are printed.

--space stable runs the same three forms on EllStable spaces (include/ellhip_batch_lowpass_streamed_stable.h, DESIGN section
9.9): the device form is ellhip_batch_lowpass_optim_streamed_stable on an EllStableBatchStreamed, the CPU loop runs over
OracleEllStable::new_with_scalar(40, 0), the host-driven form calls ellhip_batch_update on a streamed EllStable handle.  On
these spaces the family ends with NoSoln after about 1.1 n ... 1.7 n rounds, so the default shapes are
129:1536:50000,256:512:50000 (complete runs) and 512:512:300,1024:512:90 (cut off).  Byte model per instance and round:
24 n^2 of packed buffer (no fusion, nothing once per launch), the oracle's bytes as above."""
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

TOL, KAPPA = 1e-14, 40.0


def rounds_of(niter, max_iters):
    niter = np.asarray(niter)
    return int(np.sum(np.where(niter < max_iters, niter + 1, niter)))


STABLE = False  # --space stable


def new_spaces(pkg, n, B):
    cls = pkg.EllStableBatchStreamed if STABLE else pkg.EllBatchStreamed
    return cls.new_with_scalar(np.full(B, KAPPA), np.zeros((B, n)), device=0)


def fresh(ref, n, consts):
    """a CPU oracle and its CPU space"""
    if not STABLE:
        return ref.fresh(n, consts)
    return ref.O.OracleLowpass(n, *consts), ref.O.OracleEllStable.new_with_scalar(KAPPA, np.zeros(n))


def device_run(pkg, prob, gamma0, max_iters, chunk):
    prob.reset()
    prob.set_chunk(chunk)
    batch = new_spaces(pkg, prob.n, prob.B)
    batch.synchronize()
    t0 = time.perf_counter()
    x_best, has, niter, gamma, status = prob.optim(batch, gamma0, max_iters, TOL)
    return time.perf_counter() - t0, dict(x_best=x_best, has=has, niter=niter, gamma=gamma, status=status)


def cpu_run(ref, n, max_iters):
    """the six distinct members, one thread -> (records, seconds)"""
    pairs = [fresh(ref, n, ref.family(s)) for s in range(6)]
    recs = []
    t0 = time.perf_counter()
    for s, (omega, space) in enumerate(pairs):
        xb, niter, gamma, status = omega.cutting_plane_optim(space, ref.family(s)[4], max_iters, TOL)
        recs.append(dict(x_best=xb, niter=niter, gamma=gamma, status=status))
    return recs, time.perf_counter() - t0


def cpu_rows(ref, n, recs, max_iters):
    """the rows the walk visits, call by call, on a second oracle per member -> rows per oracle call"""
    rows = calls = 0
    for s, r in enumerate(recs):
        omega, space = fresh(ref, n, ref.family(s))
        gamma = ref.family(s)[4]
        for _ in range(rounds_of([r["niter"]], max_iters)):
            (g, (b0, b1)), shrunk, gamma = omega.assess_optim(np.array(space.xc), gamma)
            rows += omega.s.rows_visited
            calls += 1
            space.update(1 if shrunk else 0, g, b0, b1)
    return rows / calls


def host_run(pkg, ref, n, B, max_iters):
    """CPU oracle per instance, ellhip_batch_update with K = 1 per iteration on a streamed handle; an instance that has
    stopped receives a cut that fails (beta = +inf)"""
    consts = [ref.family(s) for s in range(B)]
    omegas = [ref.O.OracleLowpass(n, *c) for c in consts]
    batch = new_spaces(pkg, n, B)
    gamma = np.array([c[4] for c in consts])
    niter = np.full(B, max_iters, dtype=np.int64)
    live = np.ones(B, dtype=bool)
    kinds = np.zeros((1, B), dtype=np.int32)
    grads = np.ones((1, B, n))
    beta0 = np.full((1, B), math.inf)
    beta1 = np.full((1, B), math.nan)
    t0 = time.perf_counter()
    for it in range(max_iters):
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


def assert_equal_to_cpu(got, recs, what):
    for b in range(len(got["niter"])):
        r = recs[b % 6]
        ok = got["niter"][b] == r["niter"] and got["gamma"][b] == r["gamma"] and got["status"][b] == r["status"]
        ok = ok and (np.isnan(got["x_best"][b]).all() if r["x_best"] is None else np.array_equal(got["x_best"][b], r["x_best"]))
        assert ok, f"{what} and CPU disagree at instance {b}"


def summary(times):
    return {"median": statistics.median(times), "min": min(times), "max": max(times), "reps": len(times)}


def bench(pkg, ref, n, B, max_iters, reps, warmup, host_b, chunks):
    consts = [ref.family(s) for s in range(B)]
    gamma0 = np.array([c[4] for c in consts])
    prob = pkg.BatchLowpassProblem.streamed(n, *ref.columns(consts), device=0)
    hb = min(B, host_b)
    dev_t = {c: [] for c in chunks}
    cpu_t, host_t = [], []
    for rep in range(warmup + reps):
        keep = rep >= warmup
        gots = {}
        for c in chunks:
            dt, got = device_run(pkg, prob, gamma0, max_iters, c)
            gots[c] = got
            if keep:
                dev_t[c].append(dt)
        recs, dt = cpu_run(ref, n, max_iters)
        if keep:
            cpu_t.append(dt)
        ht, niter_h, gamma_h = host_run(pkg, ref, n, hb, max_iters)
        if keep:
            host_t.append(ht)
        if rep == 0:  # bit for bit, before anything is recorded (a tool run with --warmup 0 records the checked run)
            for c in chunks:
                assert_equal_to_cpu(gots[c], recs, f"device (chunk {c})")
            want = [recs[b % 6] for b in range(hb)]
            assert np.array_equal(niter_h, [r["niter"] for r in want]) and np.array_equal(gamma_h, [r["gamma"] for r in want]), \
                "host-driven form and CPU disagree"
    rounds = rounds_of(got["niter"], max_iters)
    cpu_rounds = rounds_of([r["niter"] for r in recs], max_iters)
    host_rounds = rounds_of(niter_h, max_iters)
    rows = cpu_rows(ref, n, recs, max_iters)
    cpu_rate = {k: cpu_rounds / v for k, v in summary(cpu_t).items() if k != "reps"}
    host_rate = {k: host_rounds / v for k, v in summary(host_t).items() if k != "reps"}
    out = {"bench": "batch_lowpass_streamed_stable" if STABLE else "batch_lowpass_streamed", "n": n, "B": B, "max_iters": max_iters, "rounds": rounds,
           "niter_min": int(got["niter"].min()), "niter_max": int(got["niter"].max()), "rows_per_iter": rows,
           "cpu_s_six_members": summary(cpu_t), "cpu_iters_per_s": cpu_rate["median"],
           "host_B": hb, "host_s": summary(host_t), "host_iters_per_s": host_rate["median"], "device": {}}
    fastest_baseline = max(cpu_rounds / min(cpu_t) * 16, host_rounds / min(host_t))
    for c in chunks:
        s = summary(dev_t[c])
        rate = rounds / s["median"]
        launches = max(1, -(-max_iters // c))
        matrix = 24.0 * n * n if STABLE else 16.0 * n * n + 8.0 * n * n * launches / max_iters
        model = matrix + 8.0 * n * rows + 8.0 * n
        out["device"][str(c)] = {
            "s": s, "iters_per_s": rate, "solves_per_s": B / s["median"], "over_cpu_one_thread": rate / cpu_rate["median"],
            "over_host": rate / host_rate["median"],
            "slowest_rep_over_fastest_baseline_rep": (rounds / s["max"]) / fastest_baseline,  # baseline: 16 x CPU, or host
            "model_bytes_per_round": model, "model_matrix_share": matrix / model, "model_GB_per_s": rate * model / 1e9}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--space", choices=("ell", "stable"), default="ell")
    ap.add_argument("--shapes", default=None,
                    help="default 129:1536:300,256:1536:200,512:768:150,1024:256:100 "
                         "(--space stable: 129:1536:50000,256:512:50000,512:512:300,1024:512:90)")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--host-b", type=int, default=16)
    ap.add_argument("--chunks", default="256")
    ap.add_argument("--out", default=None, help="append the JSON lines to this file as well")
    args = ap.parse_args()
    global STABLE
    STABLE = args.space == "stable"
    if args.shapes is None:
        args.shapes = ("129:1536:50000,256:512:50000,512:512:300,1024:512:90" if STABLE
                       else "129:1536:300,256:1536:200,512:768:150,1024:256:100")
    import ellalgo_rs_amd as pkg
    import batch_lowpass_reference as ref
    if pkg.capi.load().ellhip_device_count() <= 0:
        raise SystemExit("no HIP device: the batched lowpass loop has no CPU path")
    chunks = [int(c) for c in args.chunks.split(",")]
    for shape in args.shapes.split(","):
        n, B, max_iters = (int(v) for v in shape.split(":"))
        line = json.dumps(bench(pkg, ref, n, B, max_iters, args.reps, args.warmup, args.host_b, chunks))
        print(line, flush=True)
        if args.out:
            with open(args.out, "a") as f:
                f.write(line + "\n")


if __name__ == "__main__":
    main()
