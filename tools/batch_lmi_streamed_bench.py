"""The batched device-resident LMI loop on streamed batch handles (include/ellhip_batch_lmi_streamed.h)
beside its baselines: one JSON line per shape.

  python tools/batch_lmi_streamed_bench.py [--space ell|stable] [--shared] [--n 129,256,512,1024] [--m 8,64]
                                           [--batches 1536,1536,768,256] [--iters 60,40,24,12] [--reps 3] [--warmup 1]
                                           [--seconds 0.5] [--pencil-cap-gib 4] [--out FILE]

A shape is (n, M, B): one M x M block per problem, B per n as tools/batch_lowpass_streamed_bench.py chooses it (--space
stable: 1536, 512, 512, 512), so the device is full.  Workload (tests/batch_lmi_streamed_cases.py): the six starts
t = 0 ... 6 around the boundary of the feasible set over three problems, repeated to B -- runs that pass every station, cut
at the objective, and cut at the block early and late in the factorisation, as a sweep of real solves mixes them.  Every
problem has its own pencil, or with --shared all read the pencil of problem 0 (their B matrices, objectives and starts
differ).  Without --shared B is lowered until the pencils fit --pencil-cap-gib.  cutting_plane_optim, gamma = +inf, tol 0,
cut off at the n's --iters, so every problem runs every round.

  device   ellhip_batch_lmi_optim_streamed / _streamed_stable: host clock around the whole call (state reset, gamma up, the
           launches, results down) on fresh spaces; the oracle handle is made once per shape.  --warmup calls, then --reps.
  (a) cpu  the CPU loop (tests/batch_lmi_reference.py over the CPU oracle's C library, called from Python), one thread, over
           the distinct problems.
  (b) host the host-driven form on the same kind of streamed handle: per iteration ellhip_batch_get_xc, one wide
           ellhip_batch_lmi_assess_optim (the same device oracle, one workgroup per problem) and one ellhip_batch_update with
           K = 1, for all B problems.  Once per shape, after two warm-up iterations.
  (c) plain the streamed engine's own update rate at the same (n, B), cut inputs resident in HBM, K = 8 cuts per launch
           (tools/batch_streamed_bench.py: DevArrays, window), in the same process.
Rates are rounds per second (oracle + update), all problems together.  Before a rate is printed the device result must equal
(a) and (b) bit for bit: niter, gamma, x_best, idx.  oracle_share = 1 - device rate / plain K = 8 rate: the part of a round
that the plain update does not account for (0 where the loop is as fast as the plain engine).

Model printed beside the measurements, per problem and round: 16 n^2 bytes of matrix (Ell) or 24 n^2 (EllStable) and
4 M (M + 1) n bytes of pencil for one visit of the block."""
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
sys.path.insert(0, os.path.join(ROOT, "tools"))

STABLE = False  # --space stable


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.int64)


def batch_class(pkg):
    return pkg.EllStableBatchStreamed if STABLE else pkg.EllBatchStreamed


def device_run(pkg, prob, kappa, xc, max_iters):
    prob.idx = None
    spaces = batch_class(pkg).new_with_scalar(kappa, xc, device=0)
    spaces.synchronize()
    t0 = time.perf_counter()
    x_best, has, niter, gamma, status = prob.optim(spaces, math.inf, max_iters, 0.0)
    return time.perf_counter() - t0, x_best, has, niter, gamma, prob.idx


def host_run(pkg, prob, kappa, xc, max_iters):
    """(b): the oracle on the device, one call per iteration, and ellhip_batch_update with K = 1; a problem that has stopped
    receives a cut that fails (beta = +inf)"""
    B, n, J = prob.B, prob.n, prob.J
    prob.idx = None
    spaces = batch_class(pkg).new_with_scalar(kappa, xc, device=0)
    gamma = np.full(B, math.inf)
    x_best = np.full((B, n), np.nan)
    has = np.zeros(B, dtype=np.int32)
    niter = np.full(B, max_iters, dtype=np.int64)
    live = np.ones(B, dtype=bool)
    kinds = np.zeros((1, B), dtype=np.int32)
    beta0 = np.zeros((1, B))
    t0 = time.perf_counter()
    for it in range(max_iters):
        if not live.any():
            break
        x = spaces.xc()
        grad, beta, station, g = prob.assess_optim(x, gamma)
        gamma = np.where(live, g, gamma)   # (a stopped problem's oracle state is no longer compared)
        shrunk = live & (station == J + 1)
        x_best[shrunk] = x[shrunk]
        has[shrunk] = 1
        grads = grad[None]
        beta0[0] = beta
        kinds[0] = np.where(station == J + 1, 1, 0)   # central cut where every station passed, else a bias cut
        grads[0, ~live], beta0[0, ~live], kinds[0, ~live] = 1.0, math.inf, 0
        status, tsq = spaces.update(kinds, grads, beta0)
        stop = live & ((status[0] != 0) | (tsq[0] < 0.0))
        niter[stop] = it
        live &= ~stop
    return time.perf_counter() - t0, x_best, has, niter, gamma


def plain_rate(pkg, sb, n, B, seconds):
    """(c): updates/s of the streamed engine on B spaces from the identity, central cuts resident in HBM, K = 8"""
    batch = batch_class(pkg).new_with_scalar(np.ones(B), np.zeros((B, n)), device=0)
    dev = sb.DevArrays(pkg, B, n, np.random.default_rng(n))
    try:
        rate = sb.window(lambda: dev.launch(batch, sb.KMAX), batch.synchronize, sb.KMAX * B, seconds)
        dev.check_status(sb.KMAX, "plain update, K = 8")
    finally:
        dev.free()
    return rate


def bench(pkg, cases, sb, n, M, B, max_iters, args):
    ms = (M,)
    who = cases.members(n)
    D = len(who)
    if not args.shared:
        B = max(D, min(B, int(args.pencil_cap_gib * (1 << 30)) // (12 * n * M * M)))
    B -= B % D
    mat_f, mat_b, c, kappa, xc = cases.stack(n, ms, who)
    # (a) the CPU loop, one thread
    t0 = time.perf_counter()
    recs = []
    for b, (seed, t) in enumerate(who):
        fs, bs, cc = cases.problem(seed, n, ms)
        if args.shared:
            fs = cases.problem(who[0][0], n, ms)[0]
        recs.append(cases.run((fs, bs, cc), cases.cpu_space(STABLE, kappa[b], xc[b]), feas=False, max_iters=max_iters, tol=0.0))
    cpu_s = time.perf_counter() - t0
    cpu_rounds = sum(len(r["stations"]) for r in recs)
    reps = B // D
    tile = lambda a: np.tile(a, (reps,) + (1,) * (a.ndim - 1))
    if args.shared:
        prob = pkg.BatchLmiProblem.streamed([f[0] for f in mat_f], [tile(m_) for m_ in mat_b], tile(c), shared=True, device=0)
    else:
        prob = pkg.BatchLmiProblem.streamed([tile(f) for f in mat_f], [tile(m_) for m_ in mat_b], tile(c), device=0)
    kappa, xc = tile(kappa), tile(xc)
    times = []
    for rep in range(args.warmup + args.reps):
        dt, x_best, has, niter, gamma, idx = device_run(pkg, prob, kappa, xc, max_iters)
        if rep >= args.warmup:
            times.append(dt)
    which = np.arange(B) % D
    want_x = np.stack([np.full(n, np.nan) if r["x"] is None else r["x"] for r in recs])
    assert np.array_equal(niter, np.array([r["niter"] for r in recs])[which]), "device and CPU disagree (niter)"
    assert np.array_equal(bits(gamma), bits(np.array([r["gamma"] for r in recs])[which])), "device and CPU disagree (gamma)"
    assert np.array_equal(np.isnan(x_best), np.isnan(want_x[which])), "device and CPU disagree (has_best)"
    assert np.array_equal(bits(np.nan_to_num(x_best)), bits(np.nan_to_num(want_x[which]))), "device and CPU disagree (x_best)"
    assert np.array_equal(idx, np.array([r["idx"] for r in recs], dtype=np.int32)[which]), "device and CPU disagree (idx)"
    host_run(pkg, prob, kappa, xc, min(2, max_iters))   # (warm-up: the wide assess kernel's first launch)
    host_s, x_h, has_h, niter_h, gamma_h = host_run(pkg, prob, kappa, xc, max_iters)
    assert np.array_equal(niter_h, niter), "device and host-driven form disagree (niter)"
    assert np.array_equal(bits(gamma_h), bits(gamma)), "device and host-driven form disagree (gamma)"
    assert np.array_equal(bits(np.nan_to_num(x_h)), bits(np.nan_to_num(x_best))), "device and host-driven form disagree (x_best)"
    del prob
    plain = plain_rate(pkg, sb, n, B, args.seconds)
    ran = np.where(niter < max_iters, niter + 1, niter)
    rounds = int(np.sum(ran))
    med = statistics.median(times)
    rate = rounds / med
    matrix = (24.0 if STABLE else 16.0) * n * n
    pencil = 4.0 * M * (M + 1) * n
    kinds = [s for r in recs for s in r["stations"]]
    return {"bench": "batch_lmi_streamed", "space": "stable" if STABLE else "ell", "n": n, "M": M, "B": B,
            "pencil": "shared" if args.shared else "per-problem", "distinct": D, "max_iters": max_iters, "rounds": rounds,
            "block_cuts": kinds.count(0), "objective_cuts": kinds.count(1), "passed": kinds.count(2),
            "device_s": {"median": med, "min": min(times), "max": max(times), "reps": len(times)},
            "device_rounds_per_s": rate, "s_per_round": med / int(ran.max()),
            "cpu_rounds_per_s": cpu_rounds / cpu_s, "over_cpu_one_thread": rate / (cpu_rounds / cpu_s),
            "host_s": host_s, "host_rounds_per_s": rounds / host_s, "over_host": host_s / med,
            "plain_updates_per_s_K8": plain, "over_plain_K8": rate / plain, "oracle_share": max(0.0, 1.0 - rate / plain),
            "model_bytes_per_round": matrix + pencil, "model_matrix_share": matrix / (matrix + pencil),
            "model_GB_per_s": rate * (matrix + pencil) / 1e9}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--space", choices=("ell", "stable"), default="ell")
    ap.add_argument("--shared", action="store_true", help="one pencil for every problem")
    ap.add_argument("--n", default="129,256,512,1024")
    ap.add_argument("--m", default="8,64")
    ap.add_argument("--batches", default=None, help="B per n; default 1536,1536,768,256 (--space stable: 1536,512,512,512)")
    ap.add_argument("--iters", default="60,40,24,12", help="max_iters per n")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--seconds", type=float, default=0.5, help="window of the plain update rate")
    ap.add_argument("--pencil-cap-gib", type=float, default=4.0)
    ap.add_argument("--out", default=None, help="append the JSON lines to this file as well")
    args = ap.parse_args()
    global STABLE
    STABLE = args.space == "stable"
    ns = [int(v) for v in args.n.split(",")]
    if args.batches is None:
        args.batches = "1536,512,512,512" if STABLE else "1536,1536,768,256"
    batches = [int(v) for v in args.batches.split(",")]
    iters = [int(v) for v in args.iters.split(",")]
    if not len(ns) == len(batches) == len(iters):
        raise SystemExit("--n, --batches and --iters must have the same length")
    import ellalgo_rs_amd as pkg
    import batch_lmi_streamed_cases as cases
    import batch_streamed_bench as sb
    if pkg.capi.load().ellhip_device_count() <= 0:
        raise SystemExit("no HIP device: the batched LMI loop has no CPU path")
    for n, B, max_iters in zip(ns, batches, iters):
        for M in (int(v) for v in args.m.split(",")):
            line = json.dumps(bench(pkg, cases, sb, n, M, B, max_iters, args))
            print(line, flush=True)
            if args.out:
                with open(args.out, "a") as f:
                    f.write(line + "\n")


if __name__ == "__main__":
    main()
