"""The batched device-resident max-cut loops (include/ellhip_batch_maxcut.h) beside three baselines:
one JSON line per shape.

  python tools/batch_maxcut_bench.py [--space ell|stable] [--n 16,128,129,256,512,1024] [--batches 16384,2048,1536,1536,768,256]
                                     [--iters 40,60,60,40,20,10] [--distinct 16] [--reps 5] [--warmup 2] [--seconds 0.5]
                                     [--out FILE]

A shape is (n, B).  n <= 128 runs on the LDS engine (ellhip_batch_maxcut_optim / _optim_stable), n past it on the streamed
one (_optim_streamed / _optim_streamed_stable).  Workload (tests/batch_maxcut_reference.py: weights): the "mixed" table of
member 0 at that n, shared by every problem, from --distinct starting centres (members 0, 1, ..) repeated to B;
new_with_scalar(100, xc0), gamma = -inf, tol 1e-8, cut off at the n's --iters: a fixed round count, which most members run
in full.

  device   the loop entry point of the engine: host clock around the whole call (state reset, gamma up, the launches, results
           down) on fresh spaces; the oracle handle is made once per shape.  --warmup calls, then --reps: median, min, max.
  (a) cpu  tools/batch_maxcut_cpu.c: the CPU oracle's update and a literal restatement of the oracle in a plain C loop, one
           thread, over the distinct problems.
  (b) host the host-driven form on the same kind of handle: per iteration ellhip_batch_get_xc, one wide
           ellhip_batch_maxcut_assess_optim (the same device oracle) and one ellhip_batch_update with K = 1, for all B
           problems.  Once per shape, after three warm-up iterations.
  (c) plain the engine's own update rate at the same (n, B), cut inputs resident in HBM, K = 8 cuts per launch
           (tools/batch_streamed_bench.py: DevArrays, window), in the same process.
Rates are rounds per second (oracle + update), all problems together.  Before a rate is printed the device result must
equal (a) and (b) bit for bit: niter, has_best, gamma, x_best.  oracle_share is 1 - device rate / plain K = 8 rate: the part
of a round the plain update does not account for.  chain: the n (n-1) / 2 dependent adds of one cut value."""
from __future__ import annotations

import argparse
import json
import math
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
sys.path.insert(0, os.path.join(ROOT, "tools"))

TOL, KAPPA, NMAX_LDS = 1e-8, 100.0, 128
STABLE = False  # --space stable


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.int64)


def batch_class(pkg, n):
    if n <= NMAX_LDS:
        return pkg.EllStableBatch if STABLE else pkg.EllBatch
    return pkg.EllStableBatchStreamed if STABLE else pkg.EllBatchStreamed


def new_spaces(pkg, xc0, kappa=KAPPA):
    B, n = xc0.shape
    return batch_class(pkg, n).new_with_scalar(np.full(B, kappa), xc0, device=0)


def device_run(pkg, prob, xc0, max_iters):
    batch = new_spaces(pkg, xc0)
    batch.synchronize()
    t0 = time.perf_counter()
    x_best, has, niter, gamma, status = prob.optim(batch, -math.inf, max_iters, TOL)
    return time.perf_counter() - t0, x_best, has, niter, gamma


def cpu_run(w, xc0, max_iters):
    """tools/batch_maxcut_cpu.c over the distinct problems -> (its JSON line, niter, has_best, gamma, x_best)"""
    from oracle import oracle as O
    O.lib()  # builds oracle/libell_oracle.so when needed
    odir = os.path.join(ROOT, "oracle")
    D, n = xc0.shape
    with tempfile.TemporaryDirectory() as tmp:
        exe, fin, fout = (os.path.join(tmp, f) for f in ("batch_maxcut_cpu", "in.bin", "out.bin"))
        subprocess.check_call(["gcc", "-std=c99", "-O2", "-ffp-contract=off", "-D_POSIX_C_SOURCE=199309L", "-I", odir, "-o", exe,
                               os.path.join(ROOT, "tools", "batch_maxcut_cpu.c"), "-L" + odir, "-lell_oracle",
                               "-Wl,-rpath," + odir, "-lm"])
        with open(fin, "wb") as f:
            f.write(struct.pack("<3qd", D, n, max_iters, TOL) + np.ascontiguousarray(w).tobytes() +
                    np.ascontiguousarray(xc0).tobytes())
        line = json.loads(subprocess.run([exe, fin, fout] + (["stable"] if STABLE else []), check=True, capture_output=True,
                                         text=True).stdout)
        raw = np.fromfile(fout, dtype=np.float64).reshape(D, n + 3)
    return line, raw[:, 0].copy().view(np.int64), raw[:, 1].copy().view(np.int64), raw[:, 2].copy(), raw[:, 3:].copy()


def host_run(pkg, prob, xc0, max_iters):
    """(b): the oracle on the device, one call per iteration, and ellhip_batch_update with K = 1; a problem that has stopped
    receives a cut that fails (beta = +inf)"""
    B, n = xc0.shape
    batch = new_spaces(pkg, xc0)
    gamma = np.full(B, -math.inf)
    x_best = np.zeros((B, n))
    has = np.zeros(B, dtype=np.int64)
    niter = np.full(B, max_iters, dtype=np.int64)
    live = np.ones(B, dtype=bool)
    kinds = np.zeros((1, B), dtype=np.int32)
    beta0 = np.zeros((1, B))
    t0 = time.perf_counter()
    for it in range(max_iters):
        if not live.any():
            break
        xc = batch.xc()
        grad, beta, shrunk, g, _ = prob.assess_optim(xc, gamma)
        gamma[live] = g[live]
        best = live & shrunk
        x_best[best] = xc[best]
        has[best] = 1
        grads = grad[None]
        beta0[0] = beta
        kinds[0] = shrunk
        grads[0, ~live], beta0[0, ~live], kinds[0, ~live] = 1.0, math.inf, 0
        status, tsq = batch.update(kinds, grads, beta0)
        stop = live & ((status[0] != 0) | (tsq[0] < TOL))
        niter[stop] = it
        live &= ~stop
    return time.perf_counter() - t0, x_best, has, niter, gamma


def plain_rate(pkg, sb, n, B, seconds):
    """(c): updates/s of the engine on B spaces from the identity, central cuts resident in HBM, K = 8"""
    batch = batch_class(pkg, n).new_with_scalar(np.ones(B), np.zeros((B, n)), device=0)
    dev = sb.DevArrays(pkg, B, n, np.random.default_rng(n))
    try:
        rate = sb.window(lambda: dev.launch(batch, sb.KMAX), batch.synchronize, sb.KMAX * B, seconds)
        dev.check_status(sb.KMAX, "plain update, K = 8")
    finally:
        dev.free()
    return rate


def same(what, got, want):
    for name, a, b in zip(("niter", "has_best", "gamma", "x_best"), got, want):
        eq = np.array_equal(bits(a), bits(b)) if a.dtype == np.float64 else np.array_equal(a, b)
        assert eq, f"device and {what} disagree ({name})"


def bench(pkg, ref, sb, n, B, max_iters, args):
    D = min(args.distinct, B)
    w = ref.weights(0, n, "mixed")[0]
    xc_d = np.stack([ref.weights(s, n, "mixed")[1] for s in range(D)])
    cpu, c_niter, c_has, c_gamma, c_x = cpu_run(w, xc_d, max_iters)
    which = np.arange(B) % D
    xc0 = np.ascontiguousarray(xc_d[which])
    prob = pkg.BatchMaxcutProblem(w, B, device=0)
    times = []
    for rep in range(args.warmup + args.reps):
        dt, x_best, has, niter, gamma = device_run(pkg, prob, xc0, max_iters)
        if rep >= args.warmup:
            times.append(dt)
    x_best = np.where(has[:, None] != 0, x_best, 0.0)   # rows without a best point: zeros, as the other two forms leave them
    mine = (niter, has.astype(np.int64), gamma, x_best)
    same("CPU", mine, (c_niter[which], c_has[which], c_gamma[which], c_x[which]))
    host_run(pkg, prob, xc0, min(3, max_iters))   # (warm-up: the assess kernel's first launch)
    host_s, x_h, has_h, niter_h, gamma_h = host_run(pkg, prob, xc0, max_iters)
    same("host-driven form", mine, (niter_h, has_h, gamma_h, x_h))
    del prob
    plain = plain_rate(pkg, sb, n, B, args.seconds)
    ran = np.where(niter < max_iters, niter + 1, niter)   # rounds per problem; a launch lasts as long as its longest member
    rounds = int(np.sum(ran))
    med = statistics.median(times)
    rate = rounds / med
    host_rate = rounds / host_s
    return {"bench": "batch_maxcut", "space": "stable" if STABLE else "ell", "engine": "lds" if n <= NMAX_LDS else "streamed",
            "n": n, "B": B, "table": "shared", "distinct": D, "max_iters": max_iters, "rounds": rounds,
            "niter_min": int(niter.min()), "niter_max": int(niter.max()),
            "device_s": {"median": med, "min": min(times), "max": max(times), "reps": len(times)},
            "device_rounds_per_s": rate, "s_per_round": med / int(ran.max()),
            "cpu_rounds_per_s": cpu["iters_per_s"], "over_cpu_one_thread": rate / cpu["iters_per_s"],
            "host_s": host_s, "host_rounds_per_s": host_rate, "over_host": rate / host_rate,
            "plain_updates_per_s_K8": plain, "oracle_share": 1.0 - rate / plain, "chain": n * (n - 1) // 2}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--space", choices=("ell", "stable"), default="ell")
    ap.add_argument("--n", default="16,128,129,256,512,1024")
    ap.add_argument("--batches", default="16384,2048,1536,1536,768,256", help="B per n")
    ap.add_argument("--iters", default="40,60,60,40,20,10", help="max_iters per n")
    ap.add_argument("--distinct", type=int, default=16)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--seconds", type=float, default=0.5, help="window of the plain update rate")
    ap.add_argument("--out", default=None, help="append the JSON lines to this file as well")
    args = ap.parse_args()
    global STABLE
    STABLE = args.space == "stable"
    ns = [int(v) for v in args.n.split(",")]
    batches = [int(v) for v in args.batches.split(",")]
    iters = [int(v) for v in args.iters.split(",")]
    if not len(ns) == len(batches) == len(iters):
        raise SystemExit("--n, --batches and --iters must have the same length")
    import ellalgo_rs_amd as pkg
    import batch_maxcut_reference as ref
    import batch_streamed_bench as sb
    if pkg.capi.load().ellhip_device_count() <= 0:
        raise SystemExit("no HIP device: the batched max-cut loop has no CPU path")
    for n, B, max_iters in zip(ns, batches, iters):
        line = json.dumps(bench(pkg, ref, sb, n, B, max_iters, args))
        print(line, flush=True)
        if args.out:
            with open(args.out, "a") as f:
                f.write(line + "\n")


if __name__ == "__main__":
    main()
