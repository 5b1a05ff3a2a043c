"""The batched device-resident profit loops (include/ellhip_batch_profit.h) beside two baselines: one JSON
line per (kind, space, B).

  python tools/batch_profit_bench.py [--kinds plain,robust,discrete] [--spaces ell,stable] [--batches 1024,16384,262144]
                                     [--distinct 64] [--reps 5] [--warmup 2] [--out FILE]

Workload (tests/batch_profit_reference.py: family): the first --distinct members of the seeded family repeated to B, each
from new_with_scalar(100, xc0), gamma = 0, the reference's default options (2000 iterations, tolerance 1e-20): whole solves,
69 to 104 rounds for the plain kind, 18 to 51 for the discrete one; a launch lasts as long as its longest member.

  device   ellhip_batch_profit_optim / _optim_q (or _stable): host clock around the whole call (state reset, gamma up, the
           launches, results down) on fresh spaces; the oracle handle is made anew for every call, outside the clock (its
           cursors are part of the solve).  --warmup calls, then --reps: median, min, max.
  (a) cpu  tools/batch_profit_cpu.cpp: the CPU oracle's update and a restatement of the oracles and both drivers with the same
           exp / log, one thread, over the distinct problems, 100 passes.
  (b) host the host-driven form on the same kind of handle: per iteration ellhip_batch_get_xc, one wide
           ellhip_batch_profit_assess_optim / _assess_optim_q and one ellhip_batch_update with K = 1, for all B problems, the
           driver's rules in numpy on the host.  Once per shape, after three warm-up iterations.
Rates are rounds per second (oracle + update), all problems together.  Before a rate is printed the device result must equal
(a) and (b) bit for bit: niter, has_best, gamma, x_best."""
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

KAPPA = 100.0
CPU_PASSES = 100   # the distinct problems take a few milliseconds once


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.int64)


def new_spaces(pkg, stable, xc0):
    cls = pkg.EllStableBatch if stable else pkg.EllBatch
    return cls.new_with_scalar(np.full(xc0.shape[0], KAPPA), xc0, device=0)


def new_problem(pkg, kind, fam, which):
    params, a, v, vparams, _ = fam
    return pkg.BatchProfitProblem(kind, params[which], a[which], v[which], vparams[which] if kind == 1 else None, device=0)


def device_run(pkg, ref, kind, stable, fam, which, xc0):
    prob = new_problem(pkg, kind, fam, which)
    batch = new_spaces(pkg, stable, xc0)
    batch.synchronize()
    t0 = time.perf_counter()
    x_best, has, niter, gamma, status = (prob.optim_q if kind == 2 else prob.optim)(batch, 0.0, ref.MAX_ITERS, ref.TOL)
    return time.perf_counter() - t0, x_best, has, niter, gamma


def cpu_run(pkg, ref, kind, stable, fam, D):
    """tools/batch_profit_cpu.cpp over the distinct problems -> (its JSON line, niter, has_best, gamma, x_best)"""
    from oracle import oracle as O
    O.lib()  # builds oracle/libell_oracle.so when needed
    odir = os.path.join(ROOT, "oracle")
    cst = np.zeros((D, 8))
    for b in range(D):
        om = ref.make_oracle(kind, tuple(fam[0][b]), fam[1][b], fam[2][b], tuple(fam[3][b]))
        core = om.omega if hasattr(om, "omega") else om
        cst[b] = [core.log_p_scale, core.log_k, *core.price_out, fam[1][b][0], fam[1][b][1], *getattr(om, "uie", (0.0, 0.0))]
    with tempfile.TemporaryDirectory() as tmp:
        exe, fin, fout = (os.path.join(tmp, f) for f in ("batch_profit_cpu", "in.bin", "out.bin"))
        subprocess.check_call(["g++", "-std=c++17", "-O2", "-ffp-contract=off", "-I", odir, "-I", pkg.build.CSRC, "-o", exe,
                               os.path.join(ROOT, "tools", "batch_profit_cpu.cpp"), "-L" + odir, "-lell_oracle",
                               "-Wl,-rpath," + odir, "-lm"])
        with open(fin, "wb") as f:
            f.write(struct.pack("<5qd", D, kind, ref.MAX_ITERS, int(stable), CPU_PASSES, ref.TOL) + cst.tobytes() +
                    np.ascontiguousarray(fam[4][:D]).tobytes())
        line = json.loads(subprocess.run([exe, fin, fout], check=True, capture_output=True, text=True).stdout)
        raw = np.fromfile(fout, dtype=np.float64).reshape(D, 5)
    return line, raw[:, 0].copy().view(np.int64), raw[:, 1].copy().view(np.int64), raw[:, 2].copy(), raw[:, 3:].copy()


def host_run(pkg, ref, kind, stable, fam, which, xc0, max_iters):
    """(b): the oracle on the device, one call per iteration, and ellhip_batch_update with K = 1; a problem that has stopped
    receives a cut that fails (beta = +inf)"""
    B, q = xc0.shape[0], kind == 2
    prob = new_problem(pkg, kind, fam, which)
    batch = new_spaces(pkg, stable, xc0)
    gamma = np.zeros(B)
    x_best = np.zeros((B, 2))
    has = np.zeros(B, dtype=np.int64)
    niter = np.full(B, max_iters, dtype=np.int64)
    live = np.ones(B, dtype=bool)
    retry = np.zeros(B, dtype=np.int32)
    kinds = np.zeros((1, B), dtype=np.int32)
    beta0 = np.zeros((1, B))
    t0 = time.perf_counter()
    for it in range(max_iters):
        if not live.any():
            break
        xc = batch.xc()
        if q:
            grad, beta, shrunk, x_q, more, g = prob.assess_optim_q(xc, gamma, retry)
        else:
            grad, beta, shrunk, g = prob.assess_optim(xc, gamma)
            x_q = xc
        gamma[live] = g[live]
        best = live & shrunk
        x_best[best] = x_q[best]
        has[best] = 1
        grads = grad[None]
        beta0[0] = beta
        kinds[0] = 2 if q else shrunk
        grads[0, ~live], beta0[0, ~live] = (1.0, 0.0), math.inf
        status, tsq = batch.update(kinds, grads, beta0)
        st = status[0]
        if q:   # src/cutting_plane.rs:347-371
            retry[best | (st == 0)] = 0
            end = live & ((st == 1) | ((st == 2) & ~more))
            retry[live & (st == 2) & more] = 1
            stop = end | (live & (tsq[0] < ref.TOL))
        else:
            stop = live & ((st != 0) | (tsq[0] < ref.TOL))
        niter[stop] = it
        live &= ~stop
    return time.perf_counter() - t0, x_best, has, niter, gamma


def same(what, got, want):
    for name, a, b in zip(("niter", "has_best", "gamma", "x_best"), got, want):
        eq = np.array_equal(bits(a), bits(b)) if a.dtype == np.float64 else np.array_equal(a, b)
        assert eq, f"device and {what} disagree ({name})"


def bench(pkg, ref, name, stable, B, args):
    kind = ref.KINDS[name]
    fam = ref.family()
    D = min(args.distinct, B, ref.FAMILY_B)
    cpu, c_niter, c_has, c_gamma, c_x = cpu_run(pkg, ref, kind, stable, fam, D)
    which = np.arange(B) % D
    xc0 = np.ascontiguousarray(fam[4][which])
    times = []
    for rep in range(args.warmup + args.reps):
        dt, x_best, has, niter, gamma = device_run(pkg, ref, kind, stable, fam, which, xc0)
        if rep >= args.warmup:
            times.append(dt)
    x_best = np.where(has[:, None] != 0, x_best, 0.0)   # rows without a best point: zeros, as the other two forms leave them
    mine = (niter, has.astype(np.int64), gamma, x_best)
    same("CPU", mine, (c_niter[which], c_has[which], c_gamma[which], c_x[which]))
    host_run(pkg, ref, kind, stable, fam, which, xc0, 3)   # (warm-up: the assess kernel's first launch)
    host_s, x_h, has_h, niter_h, gamma_h = host_run(pkg, ref, kind, stable, fam, which, xc0, ref.MAX_ITERS)
    same("host-driven form", mine, (niter_h, has_h, gamma_h, x_h))
    ran = np.where(niter < ref.MAX_ITERS, niter + 1, niter)   # rounds per problem
    rounds = int(np.sum(ran))
    med = statistics.median(times)
    rate, host_rate = rounds / med, rounds / host_s
    return {"bench": "batch_profit", "kind": name, "space": "stable" if stable else "ell", "B": B, "distinct": D,
            "rounds": rounds, "niter_min": int(niter.min()), "niter_max": int(niter.max()),
            "device_s": {"median": med, "min": min(times), "max": max(times), "reps": len(times)},
            "device_rounds_per_s": rate, "s_per_round": med / int(ran.max()),
            "cpu_rounds_per_s": cpu["iters_per_s"], "over_cpu_one_thread": rate / cpu["iters_per_s"],
            "host_s": host_s, "host_rounds_per_s": host_rate, "over_host": rate / host_rate}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--kinds", default="plain,robust,discrete")
    ap.add_argument("--spaces", default="ell,stable")
    ap.add_argument("--batches", default="1024,16384,262144")
    ap.add_argument("--distinct", type=int, default=64)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=None, help="append the JSON lines to this file as well")
    args = ap.parse_args()
    import ellalgo_rs_amd as pkg
    import batch_profit_reference as ref
    if pkg.capi.load().ellhip_device_count() <= 0:
        raise SystemExit("no HIP device: the batched profit loop has no CPU path")
    for name in args.kinds.split(","):
        for space in args.spaces.split(","):
            for B in (int(v) for v in args.batches.split(",")):
                line = json.dumps(bench(pkg, ref, name, space == "stable", B, args))
                print(line, flush=True)
                if args.out:
                    with open(args.out, "a") as f:
                        f.write(line + "\n")


if __name__ == "__main__":
    main()
